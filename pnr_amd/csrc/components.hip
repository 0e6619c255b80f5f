// components.hip -- 3-D connected components of the traced u8 volume (pnr_label_components / pnr_despeckle_volume).  The rule
// (include/pnr_hip.h): foreground V >= t, 6- or 26-neighbours, a component's `first` is its smallest linear index, the kept components
// are numbered in ascending `first`.  Everything is an integer minimum, sum or maximum: no schedule changes a bit.
//
// A union-find that always links the larger root to the smaller index, so the root of a set is its `first`:
//   cc_local    one work-group per CC_TX x CC_TY x CC_TZ tile: the foreground flags go to LDS as "own index or NONE", every voxel unites
//               with its backward neighbours inside the tile (LDS atomic minimum), then writes one u32 link: the global index of its
//               tile-local root, NONE for background.
//   cc_merge    the voxels on tile faces unite with their backward neighbours in other tiles:  find both roots; equal -> done;
//               old = atomicMin(&link[hi], lo); old == hi -> done; else go on with (old, lo).  No thread waits for another one's write;
//               every walk follows strictly decreasing links, so every loop is bounded.  Links are read with relaxed agent-scope atomic
//               loads; a stale link is still an ancestor, and the returned value of the atomic is the truth.
//   cc_flatten  (a kernel boundary later) every voxel's link becomes its root; the roots of every CC_CHUNK voxels are counted.
//   cc_number   the roots in raster order get 0..K_all-1 (the host has scanned the chunk counts): id[root] and root[id].
//   cc_stats    one work-group per tile again: the voxels are grouped by root in an LDS table (open addressing, bounded probing),
//               the tile's partial statistics are packed LDS integers, and every (work-group, root) adds them to the component's
//               words once: one atomic per statistic, never one per voxel.
//   cc_finish   label = number of the kept component of the voxel's root (0: background or dropped); despeckle: V or 0.
// The host takes the sizes, drops what is below min_size and numbers the rest in the same order.
#include "components.h"
#include "call.h"
#include "grid.h"
#include "volume.h"
#include <cstring>

namespace {

using pnr::CC_CHUNK;
using pnr::CC_TX;
using pnr::CC_TY;
using pnr::CC_TZ;

constexpr int TPB = CC_TX * CC_TY;  // threads of a work-group: one slice of the tile
constexpr int TILE = TPB * CC_TZ;   // voxels of a tile
constexpr int NWAVES = TPB / 64;
constexpr unsigned NONE = 0xffffffffu; // the link of a background voxel (N <= 2^32 - 2: never an index)
// the packing of cc_stats: size (11 bits) | sum << 11; sx | sy << 15; one bit per local x; one bit per local y | local z << 8
static_assert(TPB == 256 && CC_TX == 32 && CC_TY == 8 && TILE == 1024, "cc_stats packs a tile's partial sums into 32-bit LDS words");
static_assert(CC_CHUNK == TPB * 16, "a lane of cc_flatten / cc_number owns 16 voxels of a chunk");

struct Tiles {
    const uint8_t *V;
    unsigned *link;
    int w, h, l;
    int tiles_x, tiles_y;
    int t;      // foreground: V >= t
    int conn26; // 0: the 3 backward face neighbours, 1: all 13
};

using Origin = pnr::TileAt;
__device__ __forceinline__ Origin tile_origin(const Tiles &a) { return pnr::tile_origin(blockIdx.x, a.tiles_x, a.tiles_y, CC_TX, CC_TY, CC_TZ); }
__device__ __forceinline__ long long vox(const Tiles &a, int x, int y, int z) { return pnr::voxel_index(a.w, a.h, x, y, z); }

// is (dx, dy, dz) one of the backward offsets of the connectivity?  (constant after unrolling, up to conn26)
__device__ __forceinline__ bool backward(int dx, int dy, int dz, int conn26)
{
    const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
    const int axes = (dx != 0) + (dy != 0) + (dz != 0);
    return before && (axes == 1 || conn26);
}

__device__ __forceinline__ unsigned lds_find(unsigned *lab, unsigned a)
{
    for (;;) {
        const unsigned p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == a) return a;
        a = p;
    }
}

__device__ __forceinline__ void lds_unite(unsigned *lab, unsigned a, unsigned b)
{
    for (;;) {
        a = lds_find(lab, a), b = lds_find(lab, b);
        if (a == b) return;
        const unsigned hi = max(a, b), lo = min(a, b);
        const unsigned old = atomicMin(&lab[hi], lo);
        if (old == hi) return;
        a = old, b = lo;
    }
}

__global__ __launch_bounds__(TPB) void cc_local(Tiles a)
{
    __shared__ unsigned lab[TILE];
    const Origin o = tile_origin(a);
    const int lx = threadIdx.x % CC_TX, ly = threadIdx.x / CC_TX, x = o.x0 + lx, y = o.y0 + ly;
    const bool inxy = x < a.w && y < a.h;
    unsigned fg = 0;
#pragma unroll
    for (int k = 0; k < CC_TZ; k++) {
        const int z = o.z0 + k;
        const bool f = inxy && z < a.l && (int)a.V[vox(a, x, y, z)] >= a.t;
        fg |= (unsigned)f << k;
        lab[k * TPB + threadIdx.x] = f ? (unsigned)(k * TPB + threadIdx.x) : NONE;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_TZ; k++) {
        if (!((fg >> k) & 1u)) continue;
        const unsigned li = (unsigned)(k * TPB) + threadIdx.x;
#pragma unroll
        for (int dz = -1; dz <= 0; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (!backward(dx, dy, dz, a.conn26)) continue;
                    const int nx = lx + dx, ny = ly + dy, nk = k + dz;
                    if (nx < 0 || nx >= CC_TX || ny < 0 || ny >= CC_TY || nk < 0) continue;
                    const unsigned lj = (unsigned)(nk * TPB + ny * CC_TX + nx);
                    if (__hip_atomic_load(&lab[lj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != NONE) lds_unite(lab, li, lj);
                }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_TZ; k++) {
        const int z = o.z0 + k;
        if (!inxy || z >= a.l) continue;
        unsigned out = NONE;
        if ((fg >> k) & 1u) {
            const unsigned r = lds_find(lab, (unsigned)(k * TPB) + threadIdx.x);
            out = (unsigned)vox(a, o.x0 + (int)(r % CC_TX), o.y0 + (int)((r / CC_TX) % CC_TY), o.z0 + (int)(r / TPB));
        }
        a.link[vox(a, x, y, z)] = out;
    }
}

__device__ __forceinline__ unsigned g_find(unsigned *link, unsigned a)
{
    for (;;) {
        const unsigned p = __hip_atomic_load(link + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == a) return a;
        a = p;
    }
}

__device__ __forceinline__ void g_unite(unsigned *link, unsigned a, unsigned b)
{
    for (;;) {
        a = g_find(link, a), b = g_find(link, b);
        if (a == b) return;
        const unsigned hi = max(a, b), lo = min(a, b);
        const unsigned old = atomicMin(link + hi, lo);
        if (old == hi) return;
        a = old, b = lo;
    }
}

__global__ __launch_bounds__(TPB) void cc_merge(Tiles a)
{
    const Origin o = tile_origin(a);
    const int lx = threadIdx.x % CC_TX, ly = threadIdx.x / CC_TX, x = o.x0 + lx, y = o.y0 + ly;
    if (x >= a.w || y >= a.h) return;
#pragma unroll
    for (int k = 0; k < CC_TZ; k++) {
        const int z = o.z0 + k;
        if (z >= a.l) break;
        const bool face = lx == 0 || lx == CC_TX - 1 || ly == 0 || ly == CC_TY - 1 || k == 0;
        if (!face) continue;
        const long long g = vox(a, x, y, z);
        if (a.link[g] == NONE) continue; // (background stays background: a plain load will do)
#pragma unroll
        for (int dz = -1; dz <= 0; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (!backward(dx, dy, dz, a.conn26)) continue;
                    const int nlx = lx + dx, nly = ly + dy, nk = k + dz;
                    const bool other = nlx < 0 || nlx >= CC_TX || nly < 0 || nly >= CC_TY || nk < 0;
                    const int nx = x + dx, ny = y + dy, nz = z + dz;
                    if (!other || nx < 0 || nx >= a.w || ny < 0 || ny >= a.h || nz < 0) continue;
                    const long long n = vox(a, nx, ny, nz);
                    if (__hip_atomic_load(a.link + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != NONE) g_unite(a.link, (unsigned)g, (unsigned)n);
                }
    }
}

// a work-group owns the chunk [b * CC_CHUNK, ...), a wave a contiguous quarter of it, a lane the voxels base + 64 k + lane
__global__ __launch_bounds__(TPB) void cc_flatten(unsigned *link, long long N, unsigned *counts)
{
    __shared__ unsigned part[NWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * CC_CHUNK + (long long)wave * (CC_CHUNK / NWAVES);
    unsigned cnt = 0;
    for (int k = 0; k < CC_CHUNK / TPB; k++) {
        const long long v = base + 64 * k + lane;
        bool root = false;
        if (v < N) {
            const unsigned p = link[v];
            if (p != NONE) {
                root = p == (unsigned)v;
                const unsigned r = g_find(link, p);
                if (r != p) link[v] = r; // (a walk through v meets the old or the new link: both are ancestors)
            }
        }
        cnt += (unsigned)__popcll(__ballot(root));
    }
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int i = 0; i < NWAVES; i++) s += part[i];
        counts[blockIdx.x] = s;
    }
}

// offsets: the exclusive scan of cc_flatten's counts.  id[root] = its rank among the roots in raster order, roots[rank] = root.
__global__ __launch_bounds__(TPB) void cc_number(const unsigned *link, long long N, const unsigned *offsets, unsigned *id, unsigned *roots)
{
    __shared__ unsigned part[NWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * CC_CHUNK + (long long)wave * (CC_CHUNK / NWAVES);
    unsigned bits = 0, cnt = 0;
    for (int k = 0; k < CC_CHUNK / TPB; k++) {
        const long long v = base + 64 * k + lane;
        const bool root = v < N && link[v] == (unsigned)v;
        bits |= (unsigned)root << k;
        cnt += (unsigned)__popcll(__ballot(root));
    }
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    unsigned run = offsets[blockIdx.x];
    for (int i = 0; i < wave; i++) run += part[i];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < CC_CHUNK / TPB; k++) {
        const bool root = (bits >> k) & 1u;
        const unsigned long long m = __ballot(root);
        if (root) {
            const long long v = base + 64 * k + lane;
            const unsigned r = run + (unsigned)__popcll(m & below);
            id[v] = r;
            roots[r] = (unsigned)v;
        }
        run += (unsigned)__popcll(m);
    }
}

struct Stats { // per component of the full numbering (K entries each)
    unsigned *size;
    unsigned long long *sum, *sx, *sy, *sz;
    unsigned *mn, *mx; // x | y | z, K each
    unsigned *vmax;
    long long K;
};

__global__ __launch_bounds__(TPB) void cc_stats(Tiles a, const unsigned *id, Stats s)
{
    __shared__ unsigned key[TILE], A[TILE], B[TILE], Cz[TILE], Dx[TILE], Eyz[TILE], F[TILE];
    const Origin o = tile_origin(a);
    const int lx = threadIdx.x % CC_TX, ly = threadIdx.x / CC_TX, x = o.x0 + lx, y = o.y0 + ly;
#pragma unroll
    for (int k = 0; k < CC_TZ; k++) {
        const int e = k * TPB + threadIdx.x;
        key[e] = NONE, A[e] = B[e] = Cz[e] = Dx[e] = Eyz[e] = F[e] = 0;
    }
    __syncthreads();
    if (x < a.w && y < a.h) {
#pragma unroll
        for (int k = 0; k < CC_TZ; k++) {
            const int z = o.z0 + k;
            if (z >= a.l) break;
            const long long g = vox(a, x, y, z);
            const unsigned R = a.link[g];
            if (R == NONE) continue;
            unsigned e = (R * 2654435761u) >> 22; // (at most TILE / 2 ... TILE distinct roots: the table always has the slot)
            for (int probe = 0; probe < TILE; probe++) {
                const unsigned old = atomicCAS(&key[e], NONE, R);
                if (old == NONE || old == R) break;
                e = (e + 1) & (TILE - 1);
            }
            const unsigned v = a.V[g];
            atomicAdd(&A[e], 1u | (v << 11));
            atomicAdd(&B[e], (unsigned)lx | ((unsigned)ly << 15));
            atomicAdd(&Cz[e], (unsigned)k);
            atomicOr(&Dx[e], 1u << lx);
            atomicOr(&Eyz[e], (1u << ly) | (1u << (8 + k)));
            atomicMax(&F[e], v);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_TZ; k++) {
        const int e = k * TPB + threadIdx.x;
        const unsigned R = key[e];
        if (R == NONE) continue;
        const long long c = id[R];
        const unsigned n = A[e] & 2047u, ym = Eyz[e] & 255u, zm = Eyz[e] >> 8;
        atomicAdd(&s.size[c], n);
        atomicAdd(&s.sum[c], (unsigned long long)(A[e] >> 11));
        atomicAdd(&s.sx[c], (unsigned long long)(B[e] & 32767u) + (unsigned long long)n * (unsigned)o.x0);
        atomicAdd(&s.sy[c], (unsigned long long)(B[e] >> 15) + (unsigned long long)n * (unsigned)o.y0);
        atomicAdd(&s.sz[c], (unsigned long long)Cz[e] + (unsigned long long)n * (unsigned)o.z0);
        atomicMin(&s.mn[c], (unsigned)(o.x0 + __ffs(Dx[e]) - 1));
        atomicMin(&s.mn[s.K + c], (unsigned)(o.y0 + __ffs(ym) - 1));
        atomicMin(&s.mn[2 * s.K + c], (unsigned)(o.z0 + __ffs(zm) - 1));
        atomicMax(&s.mx[c], (unsigned)(o.x0 + 31 - __clz(Dx[e])));
        atomicMax(&s.mx[s.K + c], (unsigned)(o.y0 + 31 - __clz(ym)));
        atomicMax(&s.mx[2 * s.K + c], (unsigned)(o.z0 + 31 - __clz(zm)));
        atomicMax(&s.vmax[c], F[e]);
    }
}

// four voxels per lane and step.  link (padded to 16 bytes) becomes the label where write_label; out (nullable) receives V with the
// dropped components cleared.  newid == NULL: every component is kept, label = id + 1.
__global__ __launch_bounds__(TPB) void cc_finish(unsigned *link, const unsigned *id, const unsigned *newid, const uint8_t *V, uint8_t *out, int write_label,
                                                 long long N)
{
    const long long groups = (N + 3) >> 2, stride = (long long)gridDim.x * TPB;
    const bool vword = out && ((uintptr_t)V & 3) == 0;
    for (long long g = (long long)blockIdx.x * TPB + threadIdx.x; g < groups; g += stride) {
        const long long i0 = 4 * g;
        const int k = (int)min(4ll, N - i0);
        const uint4 q = ((const uint4 *)link)[g];
        unsigned p[4] = {q.x, q.y, q.z, q.w}, L[4];
        bool drop[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool fg = e < k && p[e] != NONE;
            L[e] = 0;
            if (fg) {
                const unsigned c = id[p[e]];
                L[e] = newid ? newid[c] : c + 1u;
            }
            drop[e] = fg && L[e] == 0;
        }
        if (write_label) ((uint4 *)link)[g] = make_uint4(L[0], L[1], L[2], L[3]);
        if (out) {
            if (vword && k == 4) {
                unsigned wd = ((const unsigned *)V)[g];
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (drop[e]) wd &= ~(255u << (8 * e));
                ((unsigned *)out)[g] = wd; // (out is an allocation of its own: 4-byte aligned)
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (e < k) out[i0 + e] = drop[e] ? (uint8_t)0 : V[i0 + e];
            }
        }
    }
}

} // namespace

int pnr_components_run(pnr_ctx *c, const char *who, const pnr_components_opts &o, pnr_components_info *info, int32_t *label_out, pnr_component *comps,
                       int64_t cap, pnr::DevBuf<uint8_t> *despeckled)
{
    const int64_t N = c->N;
    const int w = (int)c->w, h = (int)c->h, l = (int)c->l;
    const int tiles_x = (w + CC_TX - 1) / CC_TX, tiles_y = (h + CC_TY - 1) / CC_TY, tiles_z = (l + CC_TZ - 1) / CC_TZ;
    const int64_t tiles = (int64_t)tiles_x * tiles_y * tiles_z, chunks = (N + CC_CHUNK - 1) / CC_CHUNK;
    PNR_REQUIRE(tiles < (1LL << 31), PNR_E_ARG, "%s: volume extent too large", who);
    // device buffers of the call: the links (later the labels) | the ids of the roots | the chunk counts | the byte sum
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_link = buf.add<unsigned>((size_t)N + 4), d_id = buf.add<unsigned>((size_t)N), d_cnt = buf.add<unsigned>((size_t)chunks);
    const auto d_sum = buf.add<unsigned long long>(1);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::DevBuf<uint8_t> d_out;
    if (despeckled && (rc = pnr::dev_alloc(d_out, (size_t)N, who, "for the despeckled volume"))) return rc;
    int t = o.thr;
    if (o.thr < 0 && (rc = pnr_mean_threshold(c, who, "components_threshold", c->d_img, N, d_sum, &t))) return rc; // the global mean
    pnr::Call call(c, who);
    const Tiles ta{c->d_img, d_link, w, h, l, tiles_x, tiles_y, t, o.connectivity == 26 ? 1 : 0};
    call.timed("components_local", cc_local, dim3((unsigned)tiles), dim3(TPB), ta);
    call.timed("components_merge", cc_merge, dim3((unsigned)tiles), dim3(TPB), ta);
    call.timed("components_flatten", cc_flatten, dim3((unsigned)chunks), dim3(TPB), d_link, (long long)N, d_cnt);
    // the chunk counts become their exclusive scan
    std::vector<unsigned> cnt((size_t)chunks);
    call.down(cnt.data(), d_cnt);
    if ((rc = call.finish())) return rc;
    const int64_t K = pnr::exclusive_scan_counts(cnt); // every component, the small ones included
    // the full numbering, the statistics, and what min_size keeps
    pnr::CallBuf sbuf;
    const size_t k = (size_t)K;
    const auto s_roots = sbuf.add<unsigned>(k), s_new = sbuf.add<unsigned>(k), s_size = sbuf.add<unsigned>(k); // (zeroed from s_size up to s_mn)
    const auto s_sum = sbuf.add<unsigned long long>(4 * k);
    const auto s_mx = sbuf.add<unsigned>(3 * k), s_vmax = sbuf.add<unsigned>(k), s_mn = sbuf.add<unsigned>(3 * k);
    std::vector<unsigned> size, newid;
    int64_t n_fg = 0, n_comp = 0, n_small = 0, vox_small = 0, largest = 0;
    if (K > 0) {
        if ((rc = sbuf.alloc(who))) return rc;
        const Stats sa{s_size, s_sum, s_sum + k, s_sum + 2 * k, s_sum + 3 * k, s_mn, s_mx, s_vmax, (long long)K};
        call.up(d_cnt, cnt.data());
        call.fill((char *)s_size.get(), 0, s_mn.off - s_size.off);
        call.fill(s_mn, 0xff);
        call.timed("components_number", cc_number, dim3((unsigned)chunks), dim3(TPB), d_link, (long long)N, d_cnt, d_id, s_roots);
        call.timed("components_stats", cc_stats, dim3((unsigned)tiles), dim3(TPB), ta, d_id, sa);
        size.resize(k);
        call.down(size.data(), s_size);
        if ((rc = call.finish())) return rc;
        newid.resize(k);
        for (size_t i = 0; i < k; i++) {
            const int64_t n = size[i];
            n_fg += n;
            if (n >= o.min_size) {
                newid[i] = (unsigned)++n_comp;
                largest = std::max(largest, n);
            } else {
                newid[i] = 0;
                n_small++, vox_small += n;
            }
        }
    }
    PNR_REQUIRE(!label_out || n_comp <= 0x7fffffffLL, PNR_E_ARG, "%s: %lld components do not fit the 32-bit labels", who, (long long)n_comp);
    if (info) *info = pnr_components_info{N, n_fg, n_comp, n_small, vox_small, largest, t, 0};
    const int64_t fill = comps ? std::min(cap, n_comp) : 0;
    if (fill > 0) {
        std::vector<unsigned> roots(k), box(k * 7); // mx (3 K) | vmax (K) | mn (3 K)
        std::vector<unsigned long long> sums(k * 4);
        call.down(roots.data(), s_roots);
        call.down(sums.data(), s_sum);
        call.down(box.data(), s_mx);
        call.down(box.data() + 3 * k, s_vmax);
        call.down(box.data() + 4 * k, s_mn);
        if ((rc = call.finish())) return rc;
        int64_t j = 0;
        for (size_t i = 0; i < k && j < fill; i++) {
            if (!newid[i]) continue;
            pnr_component &q = comps[j++];
            q.first = roots[i], q.size = size[i], q.sum = (int64_t)sums[i];
            q.sx = (int64_t)sums[k + i], q.sy = (int64_t)sums[2 * k + i], q.sz = (int64_t)sums[3 * k + i];
            q.x0 = (int32_t)box[4 * k + i], q.y0 = (int32_t)box[5 * k + i], q.z0 = (int32_t)box[6 * k + i];
            q.x1 = (int32_t)box[i], q.y1 = (int32_t)box[k + i], q.z1 = (int32_t)box[2 * k + i];
            q.vmax = (int32_t)box[3 * k + i], q.pad = 0;
        }
    }
    if (!label_out && !despeckled) return PNR_OK;
    const unsigned *d_new = nullptr;
    if (n_small > 0) {
        d_new = s_new;
        call.up(s_new, newid.data());
    }
    const long long groups = (N + 3) >> 2;
    call.timed("components_finish", cc_finish, dim3(pnr::grid_blocks((groups + TPB - 1) / TPB)), dim3(TPB), d_link, d_id, d_new, c->d_img, d_out.get(),
               label_out ? 1 : 0, (long long)N);
    if (label_out) call.down(label_out, d_link.get(), (size_t)N);
    if ((rc = call.finish())) return rc;
    if (despeckled) *despeckled = std::move(d_out);
    return PNR_OK;
}
