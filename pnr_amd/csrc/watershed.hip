// watershed.hip -- the marker-controlled watershed of the traced u8 volume (pnr_watershed).  The rule (include/pnr_hip.h): every voxel of
// the mask V >= t carries a key K = (M, D) as the u32 M << 24 | D; a marker voxel p holds (R(p), 0) for good; stepping from s to a mask
// neighbour t gives g(K(s), t) = (R(t), 1) where the relief rises above M(s), else (M(s), D(s) + 1), D saturating; K(t) is the minimum
// of g along all C-paths from the markers.  g is monotone and strictly increasing, so the keys are found from above: the markers at
// their keys, everything else at NONE, and every visit replaces a key by the minimum of itself and g of its neighbours' keys.  A key held
// at any time is that of a real path, so keys only fall, a stale neighbour key is still an upper bound, and when no key can fall the
// minimum holds everywhere.  The label is a SECOND relaxation over the settled keys: L(t) = the smallest L(s) over the tight neighbours
// (g(K(s), t) == K(t)); tight edges rise strictly in K, so that recursion has one solution and labels only fall towards it.  (One pass
// with the label in the low bits of the key would not do: (M, D, L) is not monotone across a rise of the relief.)  Order, tiling and
// launch cuts decide the number of visits, never a bit.
//
//   ws_init     points: a thread per point -- the centre voxel; one inside the mask takes the label with an atomic minimum (the label
//               volume was filled with ones), the others are counted as dropped.  voxels: a thread per voxel -- the relief byte
//               (255 - V without a caller's relief), the first key (a marker inside the mask: R << 24, else NONE), the label (0: none),
//               the kept marker labels appended to a list a wave at a time (for n_regions), markers outside the mask counted.
//   ws_flood    pass 1, a work-group per listed tile.  It loads the keys of the tile and its halo of 1 and the relief of the tile into LDS
//               (outside the mask or the volume: NONE, relief BLOCKED), then iterates in LDS: a thread owns a line and runs g forward and
//               backward along it -- the x rows, the y columns, (C = 6, 26) the z columns, the halo cell in front of a line as the first
//               source --, which carries a key any distance along an axis in one pass; with C = 8 or 26 one step over the full
//               neighbourhood follows (g is monotone: g of the smallest neighbouring key), reads and writes separated by a barrier.  It
//               stops when an iteration changed nothing or after `iters` iterations.  Changed keys are stored; no atomic touches a voxel.
//   ws_label    pass 2, the same with the keys read-only and the labels relaxed over the tight edges.  The rounds, the flags and who
//               marks whom: tilework.h; in round 1 of either pass every tile is listed.
//   ws_finish   the levels (M of the reached voxels, 0 elsewhere) over the relief bytes, and the statistics as block partials with one
//               set of atomics per work-group.
// The LDS rows are WS_TX + 3 cells apart: an odd pitch, so that the 32 lanes that each scan an x row meet 32 different banks.
#include "watershed.h"
#include "call.h"
#include "grid.h"
#include "tilework.h"
#include "volume.h"
#include <algorithm>
#include <vector>

namespace {

using pnr::WS_TPB;
using pnr::WS_TX;
using pnr::WS_TY;
using pnr::WS_TZ;
typedef unsigned long long u64;

constexpr unsigned NONE = ~0u;       // the key (255, 2^24 - 1): outside the mask, or not reached
constexpr unsigned DMASK = 0xffffffu;
constexpr unsigned BLOCKED = 0x100u; // the staged relief of a cell that is not a mask voxel of the tile
constexpr int HX = WS_TX + 2, HY = WS_TY + 2, HZ = WS_TZ + 2, PX = HX + 1, SXY = PX * HY, CELLS = SXY * HZ;
constexpr int RTPB = WS_TX * WS_TY; // threads of a relaxation work-group
constexpr int AUTO_ITERS = 64;      // LDS iterations per tile visit (option ws_iters = 0)
static_assert(pnr::tile_shape_ok<WS_TX, WS_TY, WS_TZ, WS_TPB>());
static_assert(PX % 2 == 1, "an odd pitch");
using Dims = pnr::TileDims;

// g(K(s), t) for a mask voxel t of relief r
__device__ inline unsigned step(unsigned ks, unsigned r)
{
    if (r > (ks >> 24)) return r << 24 | 1u;
    return (ks & DMASK) == DMASK ? ks : ks + 1u;
}

struct InitArgs {
    const uint8_t *V;
    uint8_t *R;   // the relief: uploaded (own_relief) or written here
    unsigned *key;
    int *L;       // in: the marker labels (> 0; the points' minimum, or the caller's volume); out: 0 where no marker is kept
    const float *xyz; // non-NULL: the point form of the kernel
    const int *label;
    long long n, N;
    int w, h, l, t, own_relief;
    int *mlist;
    u64 *cnt; // dropped | kept marker voxels
};

__global__ __launch_bounds__(WS_TPB) void ws_init(InitArgs a)
{
    const long long i = (long long)blockIdx.x * WS_TPB + threadIdx.x;
    if (a.xyz) {
        if (i >= a.n) return;
        const float px = a.xyz[3 * i], py = a.xyz[3 * i + 1], pz = a.xyz[3 * i + 2];
        long long g = -1;
        if (pnr::finite3(px, py, pz)) {
            g = pnr::centre_voxel(a.w, a.h, a.l, px, py, pz);
            if ((int)a.V[g] < a.t) g = -1;
        }
        if (g < 0) atomicAdd(&a.cnt[0], 1ull);
        else atomicMin((unsigned *)&a.L[g], (unsigned)(a.label ? a.label[i] : (int)(i + 1)));
        return;
    }
    const bool in = i < a.N; // (no early return: the ballots see whole waves)
    bool keep = false, drop = false;
    int lab = 0;
    if (in) {
        const unsigned v = a.V[i];
        const unsigned r = a.own_relief ? (unsigned)a.R[i] : 255u - v;
        lab = a.L[i];
        const bool mask = (int)v >= a.t, marker = lab > 0;
        keep = marker && mask, drop = marker && !mask;
        if (!a.own_relief) a.R[i] = (uint8_t)r;
        a.key[i] = keep ? r << 24 : NONE;
        a.L[i] = keep ? lab : 0;
    }
    const u64 bk = __ballot(keep), bd = __ballot(drop);
    const int lane = threadIdx.x & 63;
    if (bk) {
        const int first = __ffsll((long long)bk) - 1;
        long long base = 0;
        if (lane == first) base = (long long)atomicAdd(&a.cnt[1], (u64)__popcll(bk));
        base = __shfl(base, first, 64);
        if (keep) a.mlist[base + __popcll(bk & ((1ull << lane) - 1ull))] = lab; // (at most as many as the host counted markers)
    }
    if (bd && lane == __ffsll((long long)bd) - 1) atomicAdd(&a.cnt[0], (u64)__popcll(bd));
}

struct RelaxArgs {
    const uint8_t *V;
    const uint8_t *R;
    unsigned *key;
    unsigned *L;     // ws_label only
    const int *list; // the tiles of this launch
    int *flag_next;
    Dims d;
    int t, iters, conn;
};

// the cell of (cx, cy, cz), halo included
__device__ inline int cell_at(int cx, int cy, int cz) { return (cz * HY + cy) * PX + cx; }

// g forward and backward along the N cells base, base + stride, ...; the cells in front of both ends are the halo.  Returns whether a key fell.
template <int N>
__device__ inline int flood_line(unsigned *sk, const unsigned short *sr, int base, int stride)
{
    int ch = 0;
    unsigned p = sk[base - stride];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int cell = base + k * stride;
        const unsigned r = sr[cell], k0 = sk[cell];
        const unsigned kn = r < BLOCKED ? min(k0, step(p, r)) : k0;
        if (kn != k0) sk[cell] = kn, ch = 1;
        p = kn;
    }
    p = sk[base + N * stride];
#pragma unroll
    for (int k = N - 1; k >= 0; k--) {
        const int cell = base + k * stride;
        const unsigned r = sr[cell], k0 = sk[cell];
        const unsigned kn = r < BLOCKED ? min(k0, step(p, r)) : k0;
        if (kn != k0) sk[cell] = kn, ch = 1;
        p = kn;
    }
    return ch;
}

// the labels along the tight edges of a line, forward and backward.  Returns whether a label fell.
template <int N>
__device__ inline int label_line(const unsigned *sk, unsigned *sl, const uint8_t *sr, int base, int stride)
{
    int ch = 0;
    unsigned pk = sk[base - stride], pl = sl[base - stride];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int cell = base + k * stride;
        const unsigned kc = sk[cell];
        unsigned l0 = sl[cell];
        if (kc != NONE && pl < l0 && step(pk, sr[cell]) == kc) sl[cell] = l0 = pl, ch = 1;
        pk = kc, pl = l0;
    }
    pk = sk[base + N * stride], pl = sl[base + N * stride];
#pragma unroll
    for (int k = N - 1; k >= 0; k--) {
        const int cell = base + k * stride;
        const unsigned kc = sk[cell];
        unsigned l0 = sl[cell];
        if (kc != NONE && pl < l0 && step(pk, sr[cell]) == kc) sl[cell] = l0 = pl, ch = 1;
        pk = kc, pl = l0;
    }
    return ch;
}

__global__ __launch_bounds__(RTPB) void ws_flood(RelaxArgs a)
{
    __shared__ unsigned sk[CELLS];       // the keys; NONE: outside the mask or the volume
    __shared__ unsigned short sr[CELLS]; // the relief of the tile's own mask voxels; BLOCKED: every other cell (its key is never written)
    __shared__ unsigned touched;
    const Dims d = a.d;
    const int tile = a.list[blockIdx.x];
    const pnr::TileAt o = pnr::tile_origin((unsigned)tile, d.ntx, d.nty, WS_TX, WS_TY, WS_TZ);
    if (threadIdx.x == 0) touched = 0;
    pnr::stage_cells<WS_TX, WS_TY, WS_TZ>(d, o, [&](int cx, int cy, int cz, bool inside, long long g, bool own_cell) {
        unsigned k = NONE, r = BLOCKED;
        if (inside && (int)a.V[g] >= a.t) {
            k = __hip_atomic_load(&a.key[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (another tile may be writing its keys)
            if (own_cell) r = a.R[g];
        }
        const int cell = cell_at(cx, cy, cz);
        sk[cell] = k, sr[cell] = (unsigned short)r;
    });
    __syncthreads();
    const int lx = threadIdx.x % WS_TX, ly = threadIdx.x / WS_TX;
    const int own = cell_at(lx + 1, ly + 1, 1); // the cell of the thread's voxel z = 0; z + 1 is SXY further
    unsigned first[WS_TZ];
#pragma unroll
    for (int z = 0; z < WS_TZ; z++) first[z] = sk[own + z * SXY];
    const bool with_z = a.conn == 6 || a.conn == 26, with_diag = a.conn == 8 || a.conn == 26, diag_z = a.conn == 26;
    int again = 0;
    for (int it = 0; it < a.iters; it++) {
        int changed = 0;
        for (int line = threadIdx.x; line < WS_TY * WS_TZ; line += RTPB) // the x rows
            changed |= flood_line<WS_TX>(sk, sr, cell_at(1, line % WS_TY + 1, line / WS_TY + 1), 1);
        __syncthreads();
        for (int line = threadIdx.x; line < WS_TX * WS_TZ; line += RTPB) // the y columns
            changed |= flood_line<WS_TY>(sk, sr, cell_at(line % WS_TX + 1, 1, line / WS_TX + 1), PX);
        __syncthreads();
        if (with_z) {
            changed |= flood_line<WS_TZ>(sk, sr, own, SXY); // the thread's own z column
            __syncthreads();
        }
        if (with_diag) {
            unsigned m[HZ]; // the smallest key over the 9 columns around the thread's, per plane of the tile and its halo
#pragma unroll
            for (int q = 0; q < HZ; q++) m[q] = NONE;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int col = own - SXY + dy * PX + dx; // the neighbouring column's cell at z = -1
#pragma unroll
                    for (int q = 0; q < HZ; q++) m[q] = min(m[q], sk[col + q * SXY]);
                }
            unsigned nw[WS_TZ];
#pragma unroll
            for (int z = 0; z < WS_TZ; z++) {
                const unsigned best = diag_z ? min(m[z], min(m[z + 1], m[z + 2])) : m[z + 1]; // (holds the voxel's own key: g of it is above it)
                const unsigned r = sr[own + z * SXY];
                nw[z] = r < BLOCKED ? step(best, r) : NONE;
            }
            __syncthreads(); // every read of this step is done
#pragma unroll
            for (int z = 0; z < WS_TZ; z++)
                if (nw[z] < sk[own + z * SXY]) sk[own + z * SXY] = nw[z], changed = 1;
        }
        again = __syncthreads_or(changed); // ... and every write
        if (!again) break;
    }
    unsigned mine = 0;
#pragma unroll
    for (int z = 0; z < WS_TZ; z++) {
        const unsigned cur = sk[own + z * SXY];
        if (cur != first[z]) { // (a mask voxel inside the volume: the others stay NONE)
            const long long g = pnr::voxel_index(d.w, d.h, o.x0 + lx, o.y0 + ly, o.z0 + z);
            __hip_atomic_store(&a.key[g], cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mine |= pnr::halo_bits<WS_TX, WS_TY, WS_TZ>(lx, ly, z);
        }
    }
    pnr::mark_tiles(a.flag_next, d, o, tile, touched, mine, again);
}

__global__ __launch_bounds__(RTPB) void ws_label(RelaxArgs a)
{
    __shared__ unsigned sk[CELLS]; // the settled keys, read only; NONE: outside the mask or the volume, or not reached
    __shared__ unsigned sl[CELLS]; // the labels; NONE: none yet
    __shared__ uint8_t sr[CELLS];  // the relief of the tile's own cells
    __shared__ unsigned touched;
    const Dims d = a.d;
    const int tile = a.list[blockIdx.x];
    const pnr::TileAt o = pnr::tile_origin((unsigned)tile, d.ntx, d.nty, WS_TX, WS_TY, WS_TZ);
    if (threadIdx.x == 0) touched = 0;
    pnr::stage_cells<WS_TX, WS_TY, WS_TZ>(d, o, [&](int cx, int cy, int cz, bool inside, long long g, bool) {
        unsigned k = NONE, lab = NONE, r = 0;
        if (inside) {
            k = a.key[g]; // (NONE outside the mask)
            if (k != NONE) {
                lab = __hip_atomic_load(&a.L[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (another tile may be writing its labels)
                if (lab == 0) lab = NONE;
                r = a.R[g];
            }
        }
        const int cell = cell_at(cx, cy, cz);
        sk[cell] = k, sl[cell] = lab, sr[cell] = (uint8_t)r;
    });
    __syncthreads();
    const int lx = threadIdx.x % WS_TX, ly = threadIdx.x / WS_TX;
    const int own = cell_at(lx + 1, ly + 1, 1);
    unsigned first[WS_TZ], kown[WS_TZ], rown[WS_TZ];
#pragma unroll
    for (int z = 0; z < WS_TZ; z++) first[z] = sl[own + z * SXY], kown[z] = sk[own + z * SXY], rown[z] = sr[own + z * SXY];
    const bool with_z = a.conn == 6 || a.conn == 26, with_diag = a.conn == 8 || a.conn == 26, diag_z = a.conn == 26;
    int again = 0;
    for (int it = 0; it < a.iters; it++) {
        int changed = 0;
        for (int line = threadIdx.x; line < WS_TY * WS_TZ; line += RTPB) // the x rows
            changed |= label_line<WS_TX>(sk, sl, sr, cell_at(1, line % WS_TY + 1, line / WS_TY + 1), 1);
        __syncthreads();
        for (int line = threadIdx.x; line < WS_TX * WS_TZ; line += RTPB) // the y columns
            changed |= label_line<WS_TY>(sk, sl, sr, cell_at(line % WS_TX + 1, 1, line / WS_TX + 1), PX);
        __syncthreads();
        if (with_z) {
            changed |= label_line<WS_TZ>(sk, sl, sr, own, SXY);
            __syncthreads();
        }
        if (with_diag) {
            unsigned best[WS_TZ];
#pragma unroll
            for (int z = 0; z < WS_TZ; z++) best[z] = NONE;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int col = own - SXY + dy * PX + dx;
                    unsigned kq[HZ], lq[HZ];
#pragma unroll
                    for (int q = 0; q < HZ; q++) kq[q] = sk[col + q * SXY], lq[q] = sl[col + q * SXY];
#pragma unroll
                    for (int z = 0; z < WS_TZ; z++)
#pragma unroll
                        for (int dz = -1; dz <= 1; dz++) {
                            if (dz != 0 && !diag_z) continue;
                            const int q = z + 1 + dz; // (the voxel itself is never tight: g of its key is above it)
                            if (kown[z] != NONE && step(kq[q], rown[z]) == kown[z]) best[z] = min(best[z], lq[q]);
                        }
                }
            __syncthreads(); // every read of this step is done
#pragma unroll
            for (int z = 0; z < WS_TZ; z++)
                if (best[z] < sl[own + z * SXY]) sl[own + z * SXY] = best[z], changed = 1;
        }
        again = __syncthreads_or(changed); // ... and every write
        if (!again) break;
    }
    unsigned mine = 0;
#pragma unroll
    for (int z = 0; z < WS_TZ; z++) {
        const unsigned cur = sl[own + z * SXY];
        if (cur != first[z]) { // (a reached voxel inside the volume: the others stay NONE)
            const long long g = pnr::voxel_index(d.w, d.h, o.x0 + lx, o.y0 + ly, o.z0 + z);
            __hip_atomic_store(&a.L[g], cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mine |= pnr::halo_bits<WS_TX, WS_TY, WS_TZ>(lx, ly, z);
        }
    }
    pnr::mark_tiles(a.flag_next, d, o, tile, touched, mine, again);
}

// st (zeroed by the host): n_mask | n_reached | m_max | d_max | 1 + the largest level with a saturated D (0: none).  level (nullable):
// M of the reached voxels, 0 elsewhere (it may be the relief volume: every byte is read by no other thread).
__global__ __launch_bounds__(WS_TPB) void ws_finish(const uint8_t *V, const unsigned *key, uint8_t *level, long long N, Dims d, int t, int conn, u64 *st)
{
    __shared__ u64 part[5 * (WS_TPB / 64)];
    const long long stride = (long long)gridDim.x * WS_TPB;
    u64 w[5] = {0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * WS_TPB + threadIdx.x; i < N; i += stride) {
        const unsigned k = key[i];
        const bool mask = (int)V[i] >= t, reached = k != NONE;
        w[0] += mask, w[1] += reached;
        if (reached) {
            w[2] = max(w[2], (u64)(k >> 24)), w[3] = max(w[3], (u64)(k & DMASK));
            if ((k & DMASK) == DMASK) w[4] = max(w[4], (u64)(k >> 24) + 1);
            if (k == NONE - 1) { // (255, 2^24 - 2): a mask neighbour without a key is a voxel whose D saturated
                const int x = (int)(i % d.w), y = (int)(i / d.w % d.h), z = (int)(i / ((long long)d.w * d.h));
                for (int n = 0; n < 27; n++) {
                    const int dx = n % 3 - 1, dy = n / 3 % 3 - 1, dz = n / 9 - 1, nz = (dx != 0) + (dy != 0) + (dz != 0);
                    if (nz == 0 || ((conn == 4 || conn == 8) && dz) || ((conn == 4 || conn == 6) && nz != 1)) continue;
                    const int qx = x + dx, qy = y + dy, qz = z + dz;
                    if (qx < 0 || qx >= d.w || qy < 0 || qy >= d.h || qz < 0 || qz >= d.l) continue;
                    const long long g = pnr::voxel_index(d.w, d.h, qx, qy, qz);
                    if ((int)V[g] >= t && key[g] == NONE) w[4] = 256;
                }
            }
        }
        if (level) level[i] = reached ? (uint8_t)(k >> 24) : (uint8_t)0;
    }
#pragma unroll
    for (int k = 0; k < 5; k++)
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const u64 other = (u64)__shfl_xor((long long)w[k], sh, 64);
            w[k] = k >= 2 ? max(w[k], other) : w[k] + other;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 5; k++) part[5 * wave + k] = w[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WS_TPB / 64; i++)
            for (int k = 0; k < 5; k++) w[k] = k >= 2 ? max(w[k], part[5 * i + k]) : w[k] + part[5 * i + k];
        for (int k = 0; k < 2; k++)
            if (w[k]) atomicAdd(&st[k], w[k]);
        for (int k = 2; k < 5; k++)
            if (w[k]) atomicMax(&st[k], w[k]);
    }
}

} // namespace

int pnr_watershed_run(pnr_ctx *c, const char *who, const pnr_watershed_opts &o, const uint8_t *relief, const pnr_ws_markers &m, pnr_watershed_info *info, int32_t *label_out,
                      uint8_t *level_out)
{
    const int64_t N = c->N;
    Dims d;
    int rc = pnr::tile_dims<WS_TX, WS_TY, WS_TZ>(c, who, d);
    if (rc) return rc;
    const int64_t tiles = d.tiles(), vblocks = (N + WS_TPB - 1) / WS_TPB;
    const bool points = m.vol == nullptr;
    const int64_t cap = points ? std::min(m.n_src, N) : m.n_pos; // the kept marker voxels at most
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_key = buf.add<unsigned>((size_t)N);
    const auto d_lab = buf.add<int>((size_t)N);
    const auto d_rel = buf.add<uint8_t>((size_t)N);
    pnr::TileRounds rounds(c, who, buf, d);
    const auto d_word = buf.add<u64>(1), d_cnt = buf.add<u64>(2), d_st = buf.add<u64>(5);
    const auto d_sxyz = buf.add<float>(points ? (size_t)m.n_src * 3 : 0);
    const auto d_slab = buf.add<int>(points && m.src_label ? (size_t)m.n_src : 0);
    const auto d_mlist = buf.add<int>((size_t)cap);
    if ((rc = buf.alloc(who)) || (rc = rounds.pin())) return rc;
    int t = o.thr;
    if (o.thr < 0 && (rc = pnr_mean_threshold(c, who, "watershed_init", c->d_img, N, d_word, &t))) return rc; // the global mean
    pnr::Call call(c, who);
    call.fill(d_cnt, 0);
    if (relief) call.up(d_rel, relief);
    InitArgs ia{c->d_img, d_rel.get(), d_key.get(), d_lab.get(), nullptr, nullptr, 0, (long long)N, d.w, d.h, d.l, t, relief ? 1 : 0, d_mlist.get(), d_cnt.get()};
    if (points) {
        call.fill(d_lab, 0xff);
        call.up(d_sxyz, m.src_xyz);
        if (m.src_label) call.up(d_slab, m.src_label);
        InitArgs pa = ia;
        pa.xyz = d_sxyz.get(), pa.label = m.src_label ? d_slab.get() : nullptr, pa.n = (long long)m.n_src;
        call.timed("watershed_init", ws_init, dim3((unsigned)((m.n_src + WS_TPB - 1) / WS_TPB)), dim3(WS_TPB), pa);
    } else call.up(d_lab, m.vol);
    call.timed("watershed_init", ws_init, dim3((unsigned)vblocks), dim3(WS_TPB), ia);
    const int iters = c->opt.ws_iters > 0 ? c->opt.ws_iters : AUTO_ITERS;
    pnr::TileRounds::Tally done[2];
    c->ws_rounds = c->ws_visits = 0;
    for (int pass = 0; pass < 2; pass++) {
        rounds.seed_all(call);
        // (a key falls at most 2^32 times; the bound only ends a loop that a fault keeps alive)
        rc = rounds.run(call, "watershed_compact", pnr::tiles_per_launch(c->opt.ws_tiles_per_launch), 256 * N + tiles + 16, pass + 1, [&](const int *list, int64_t n, int *flag_next) {
            const RelaxArgs ra{c->d_img, d_rel.get(), d_key.get(), (unsigned *)d_lab.get(), list, flag_next, d, t, iters, o.connectivity};
            if (pass == 0) call.timed("watershed_flood", ws_flood, dim3((unsigned)n), dim3(RTPB), ra);
            else call.timed("watershed_label", ws_label, dim3((unsigned)n), dim3(RTPB), ra);
        }, done[pass]);
        if (rc) return rc;
    }
    c->ws_rounds = done[0].rounds + done[1].rounds, c->ws_visits = done[0].visits + done[1].visits;
    u64 st[5] = {0, 0, 0, 0, 0}, cnt[2] = {0, 0};
    call.fill(d_st, 0);
    call.timed("watershed_finish", ws_finish, dim3(pnr::grid_blocks(vblocks)), dim3(WS_TPB), c->d_img, (const unsigned *)d_key.get(),
               level_out ? d_rel.get() : (uint8_t *)nullptr, (long long)N, d, t, o.connectivity, d_st.get());
    call.down(st, d_st);
    call.down(cnt, d_cnt);
    if ((rc = call.finish())) return rc;
    PNR_REQUIRE(st[4] == 0, PNR_E_ARG, "%s: a plateau deeper than %u steps at level %d: the step count D of the key saturated", who, DMASK - 1, (int)std::min<u64>(st[4] - 1, 255));
    PNR_REQUIRE((int64_t)cnt[1] <= cap, PNR_E_HIP, "%s: %lld marker voxels kept, %lld counted", who, (long long)cnt[1], (long long)cap);
    std::vector<int32_t> labels((size_t)cnt[1]);
    if (!labels.empty()) call.down(labels.data(), (const int *)d_mlist.get(), labels.size());
    if (label_out) call.down(label_out, d_lab);
    if (level_out) call.down(level_out, d_rel);
    if ((rc = call.finish())) return rc;
    if (info) {
        std::sort(labels.begin(), labels.end()); // every region holds its marker: the labels of the result are those of the kept markers
        const int64_t regions = (int64_t)(std::unique(labels.begin(), labels.end()) - labels.begin());
        auto i32 = [](int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); };
        *info = pnr_watershed_info{N,      (int64_t)st[0], (int64_t)cnt[1], (int64_t)cnt[0], (int64_t)st[1], (int64_t)(st[0] - st[1]), regions,
                                   tiles,  done[0].visits, done[1].visits,  (int32_t)st[2],  (int32_t)st[3], t,                        o.connectivity,
                                   i32(done[0].rounds), i32(done[1].rounds)};
    }
    return PNR_OK;
}
