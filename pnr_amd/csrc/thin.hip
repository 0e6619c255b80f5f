// thin.hip -- topological thinning of the traced u8 volume to a one-voxel-wide curve skeleton (pnr_skeletonize).  The rule
// (include/pnr_hip.h): the object is V >= t under (26, 6) connectivity; a round marks the border voxels, then eight subfield passes
// delete the marked voxels that are simple and no end point, all voxels of a pass at once.  Two voxels of a subfield are never
// 26-adjacent, so a pass equals a sequential deletion and runs in place; every bit is fixed whatever the tiling or launch cut.
//
// One state byte per voxel: 0 background, 1 object, 2 object and candidate of the round.
//   thin_init    V and t become the state; counts the foreground.
//   thin_plan    between two passes, from completed passes only: the tiles to visit, those whose own stamp or one of their 26 neighbour
//                tiles' stamps (the last pass in which the tile deleted something) is not older than the previous round's first pass.
//                A voxel whose N26 has not changed since it was last tested gets the same answer, and N26 lies in these 27 tiles.
//   thin_mark    (round start) over the tiles of pass 0: object voxels with a background voxel in N6 become 2, the others 1.  In place: a
//                neighbour only ever switches between two non-zero states.  A tile that is not listed keeps the flags of its last mark,
//                which a mark now would give again.
//   thin_pass    one subfield over the listed tiles: the tile and a one-voxel halo go to LDS, a thread owns one voxel of the subfield,
//                gathers the 26 neighbour bits into one word (bit x + 3 y + 9 z of the 3 x 3 x 3 cube, the centre clear) and runs the
//                two connectivity tests on it by growing a reached-set: a box (26) or cross (6) dilation of the word by masked shifts,
//                clipped to the object (or to the background of N18), until it is stable.  A thread reads voxels of other subfields
//                and writes only its own.  The deletions are counted per work-group, the tile is stamped.
//   thin_count / thin_list   the skeleton voxels of every THIN_CHUNK voxels are counted, the host scans the counts, and the voxels are
//                written in raster order with their degree (object voxels in N26).
//   thin_finish  the state becomes 0 / 255.
// The host reads one word of deletions and the eight list lengths per round.
// Below the kernels: skeleton_forest, the host's Kruskal over the skeleton's voxels.
#include "thin.h"
#include "call.h"
#include "grid.h"
#include "volume.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

using pnr::THIN_CHUNK;
using pnr::THIN_TX;
using pnr::THIN_TY;
using pnr::THIN_TZ;

constexpr int TPB = 256;
constexpr int NWAVES = TPB / 64;
constexpr int HX = THIN_TX + 2, HY = THIN_TY + 2, HZ = THIN_TZ + 2; // the tile with its halo
constexpr int HALO = HX * HY * HZ;
constexpr int MAX_BLOCKS = 8192;
static_assert(THIN_TX % 2 == 0 && THIN_TY % 2 == 0 && THIN_TZ % 2 == 0, "a subfield is the parity of the place in the tile");
static_assert((THIN_TX / 2) * (THIN_TY / 2) * (THIN_TZ / 2) == TPB, "thin_pass: one voxel of the subfield per thread");
static_assert(THIN_TX * THIN_TY == TPB, "thin_mark: one slice of the tile per step");
static_assert(THIN_CHUNK == TPB * 16, "a lane of thin_count / thin_list owns 16 voxels of a chunk");

// ---- the 27-bit words of the 3 x 3 x 3 cube: bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1) ----
constexpr unsigned cube_mask(int axis, int at) // the cells whose coordinate `axis` is `at`
{
    unsigned m = 0;
    for (int i = 0; i < 27; i++) {
        const int c[3] = {i % 3, i / 3 % 3, i / 9};
        if (c[axis] == at) m |= 1u << i;
    }
    return m;
}
constexpr unsigned near_mask(int most) // the cells with 1..most coordinates off the centre: N6 for 1, N18 for 2, N26 for 3
{
    unsigned m = 0;
    for (int i = 0; i < 27; i++) {
        const int k = (i % 3 != 1) + (i / 3 % 3 != 1) + (i / 9 != 1);
        if (k >= 1 && k <= most) m |= 1u << i;
    }
    return m;
}
constexpr unsigned X0 = cube_mask(0, 0), X2 = cube_mask(0, 2), Y0 = cube_mask(1, 0), Y2 = cube_mask(1, 2), Z0 = cube_mask(2, 0), Z2 = cube_mask(2, 2);
constexpr unsigned N6 = near_mask(1), N18 = near_mask(2), N26 = near_mask(3);
static_assert(N26 == 0x7ffffffu - (1u << 13) && __builtin_popcount(N6) == 6 && __builtin_popcount(N18) == 18, "the neighbourhoods of the cube");

__device__ __forceinline__ unsigned along(unsigned r, unsigned lo, unsigned hi, int sh) { return ((r & ~hi) << sh) | ((r & ~lo) >> sh); }
// every cell within one step of r: 26-steps (the box, axis after axis) and 6-steps (the cross)
__device__ __forceinline__ unsigned grow26(unsigned r)
{
    r |= along(r, X0, X2, 1);
    r |= along(r, Y0, Y2, 3);
    return r | along(r, Z0, Z2, 9);
}
__device__ __forceinline__ unsigned grow6(unsigned r) { return r | along(r, X0, X2, 1) | along(r, Y0, Y2, 3) | along(r, Z0, Z2, 9); }

// m: the object voxels of N26(p).  Simple (Malandain-Bertrand) and not an end point?
__device__ __forceinline__ bool deletable(unsigned m)
{
    if (__popc(m) <= 1) return false; // isolated (not simple), or an end point
    unsigned r = m & (0u - m), was;
    do { // (a) the object of N26 is one 26-connected set
        was = r;
        r = grow26(r) & m;
    } while (r != was);
    if (r != m) return false;
    const unsigned b = ~m & N18, f = b & N6;
    if (!f) return false;
    r = f & (0u - f);
    do { // (b) the background of N6 lies in one 6-connected set of the background of N18
        was = r;
        r = grow6(r) & b;
    } while (r != was);
    return (f & ~r) == 0;
}

struct Grid {
    uint8_t *S; // the state
    int w, h, l;
    int tiles_x, tiles_y, tiles_z;
};

using Origin = pnr::TileAt;
__device__ __forceinline__ Origin tile_origin(const Grid &a, unsigned b) { return pnr::tile_origin(b, a.tiles_x, a.tiles_y, THIN_TX, THIN_TY, THIN_TZ); }
__device__ __forceinline__ long long vox(const Grid &a, int x, int y, int z) { return pnr::voxel_index(a.w, a.h, x, y, z); }

// the tile at o with its halo into sh; outside the volume is background
__device__ __forceinline__ void load_halo(const Grid &a, const Origin &o, uint8_t *sh)
{
    for (int e = threadIdx.x; e < HALO; e += TPB) {
        const int hx = e % HX, r = e / HX, hy = r % HY, hz = r / HY;
        const int x = o.x0 + hx - 1, y = o.y0 + hy - 1, z = o.z0 + hz - 1;
        uint8_t v = 0;
        if (x >= 0 && x < a.w && y >= 0 && y < a.h && z >= 0 && z < a.l) v = a.S[vox(a, x, y, z)];
        sh[e] = v;
    }
}

__global__ __launch_bounds__(TPB) void thin_init(const uint8_t *V, uint8_t *S, long long N, int t, unsigned long long *n_fg)
{
    __shared__ unsigned part;
    if (threadIdx.x == 0) part = 0;
    __syncthreads();
    unsigned cnt = 0;
    const long long stride = (long long)gridDim.x * TPB;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
        const bool f = (int)V[i] >= t;
        S[i] = f ? 1 : 0;
        cnt += f;
    }
    if (cnt) atomicAdd(&part, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && part) atomicAdd(n_fg, (unsigned long long)part);
}

// the tiles of the next pass: stamps are pass numbers from 1, lo the first pass of the previous round
__global__ __launch_bounds__(TPB) void thin_plan(const unsigned *stamp, int tiles_x, int tiles_y, int tiles_z, unsigned lo, unsigned *list, unsigned *count)
{
    const long long tiles = (long long)tiles_x * tiles_y * tiles_z, t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t >= tiles) return;
    const pnr::TileAt at = pnr::tile_origin((unsigned)t, tiles_x, tiles_y, 1, 1, 1);
    unsigned last = 0;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int x = at.tx + dx, y = at.ty + dy, z = at.tz + dz;
                if (x < 0 || x >= tiles_x || y < 0 || y >= tiles_y || z < 0 || z >= tiles_z) continue;
                last = max(last, stamp[pnr::voxel_index(tiles_x, tiles_y, x, y, z)]);
            }
    if (last >= lo) list[atomicAdd(count, 1u)] = (unsigned)t;
}

// list == NULL: every tile (n_all of them)
__global__ __launch_bounds__(TPB) void thin_mark(Grid a, const unsigned *list, const unsigned *count, unsigned n_all)
{
    __shared__ uint8_t sh[HALO];
    const unsigned n = list ? *count : n_all;
    const int lx = threadIdx.x % THIN_TX, ly = threadIdx.x / THIN_TX;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const Origin o = tile_origin(a, list ? list[i] : i);
        load_halo(a, o, sh);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < THIN_TZ; k++) {
            const int e = ((k + 1) * HY + ly + 1) * HX + lx + 1;
            const uint8_t c = sh[e];
            if (!c) continue; // (background, or outside the volume)
            const bool inner = sh[e - 1] && sh[e + 1] && sh[e - HX] && sh[e + HX] && sh[e - HX * HY] && sh[e + HX * HY];
            const uint8_t v = inner ? 1 : 2;
            if (v != c) a.S[vox(a, o.x0 + lx, o.y0 + ly, o.z0 + k)] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(TPB) void thin_pass(Grid a, const unsigned *list, const unsigned *count, unsigned n_all, int s, unsigned pass_no, unsigned *stamp,
                                                 unsigned *deleted)
{
    __shared__ uint8_t sh[HALO];
    __shared__ unsigned ndel;
    const unsigned n = list ? *count : n_all;
    const int t = threadIdx.x;
    const int lx = 2 * (t % (THIN_TX / 2)) + (s & 1), ly = 2 * (t / (THIN_TX / 2) % (THIN_TY / 2)) + ((s >> 1) & 1), lz = 2 * (t / (THIN_TX / 2 * (THIN_TY / 2))) + ((s >> 2) & 1);
    const int e = ((lz + 1) * HY + ly + 1) * HX + lx + 1;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const unsigned tile = list ? list[i] : i;
        const Origin o = tile_origin(a, tile);
        if (t == 0) ndel = 0;
        load_halo(a, o, sh);
        __syncthreads();
        bool del = false;
        if (sh[e] == 2) { // a candidate that is still object (and so inside the volume)
            unsigned m = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        if (!dx && !dy && !dz) continue;
                        m |= (unsigned)(sh[e + (dz * HY + dy) * HX + dx] != 0) << ((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1));
                    }
            del = deletable(m);
            if (del) a.S[vox(a, o.x0 + lx, o.y0 + ly, o.z0 + lz)] = 0;
        }
        const unsigned long long b = __ballot(del);
        if ((t & 63) == 0 && b) atomicAdd(&ndel, (unsigned)__popcll(b));
        __syncthreads();
        if (t == 0 && ndel) {
            atomicAdd(deleted, ndel);
            stamp[tile] = pass_no;
        }
        __syncthreads();
    }
}

// a work-group owns the chunk [b * THIN_CHUNK, ...), a wave a contiguous quarter of it, a lane the voxels base + 64 k + lane
__global__ __launch_bounds__(TPB) void thin_count(const uint8_t *S, long long N, unsigned *counts)
{
    __shared__ unsigned part[NWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * THIN_CHUNK + (long long)wave * (THIN_CHUNK / NWAVES);
    unsigned cnt = 0;
    for (int k = 0; k < THIN_CHUNK / TPB; k++) {
        const long long v = base + 64 * k + lane;
        cnt += (unsigned)__popcll(__ballot(v < N && S[v] != 0));
    }
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int i = 0; i < NWAVES; i++) s += part[i];
        counts[blockIdx.x] = s;
    }
}

// offsets: the exclusive scan of thin_count's counts.  The skeleton voxels in raster order: their index and their degree.
__global__ __launch_bounds__(TPB) void thin_list(Grid a, long long N, const unsigned *offsets, unsigned *out_vox, uint8_t *out_deg)
{
    __shared__ unsigned part[NWAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * THIN_CHUNK + (long long)wave * (THIN_CHUNK / NWAVES);
    unsigned bits = 0, cnt = 0;
    for (int k = 0; k < THIN_CHUNK / TPB; k++) {
        const long long v = base + 64 * k + lane;
        const bool on = v < N && a.S[v] != 0;
        bits |= (unsigned)on << k;
        cnt += (unsigned)__popcll(__ballot(on));
    }
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    unsigned run = offsets[blockIdx.x];
    for (int i = 0; i < wave; i++) run += part[i];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < THIN_CHUNK / TPB; k++) {
        const bool on = (bits >> k) & 1u;
        const unsigned long long m = __ballot(on);
        if (on) {
            const long long v = base + 64 * k + lane;
            const int x = (int)(v % a.w), y = (int)(v / a.w % a.h), z = (int)(v / ((long long)a.w * a.h));
            int deg = 0;
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int nx = x + dx, ny = y + dy, nz = z + dz;
                        if ((!dx && !dy && !dz) || nx < 0 || nx >= a.w || ny < 0 || ny >= a.h || nz < 0 || nz >= a.l) continue;
                        deg += a.S[vox(a, nx, ny, nz)] != 0;
                    }
            const unsigned r = run + (unsigned)__popcll(m & below);
            out_vox[r] = (unsigned)v;
            out_deg[r] = (uint8_t)deg;
        }
        run += (unsigned)__popcll(m);
    }
}

// four state bytes per lane (the state is an allocation of its own, padded to 16 bytes): 0 stays 0, 1 and 2 become 255
__global__ __launch_bounds__(TPB) void thin_finish(unsigned *S4, long long words)
{
    const long long stride = (long long)gridDim.x * TPB;
    for (long long g = (long long)blockIdx.x * TPB + threadIdx.x; g < words; g += stride) {
        const unsigned v = S4[g];
        S4[g] = ((v | (v >> 1)) & 0x01010101u) * 255u;
    }
}

unsigned blocks_for(long long items) { return pnr::grid_blocks(items, MAX_BLOCKS); }

} // namespace

int pnr_thin_run(pnr_ctx *c, const char *who, const pnr_thin_opts &o, pnr_thin_info *info, uint8_t *skel_out, int64_t *vox_out, uint8_t *deg_out, int64_t cap)
{
    const int64_t N = c->N;
    const int w = (int)c->w, h = (int)c->h, l = (int)c->l;
    const int tiles_x = (w + THIN_TX - 1) / THIN_TX, tiles_y = (h + THIN_TY - 1) / THIN_TY, tiles_z = (l + THIN_TZ - 1) / THIN_TZ;
    const int64_t tiles = (int64_t)tiles_x * tiles_y * tiles_z, chunks = (N + THIN_CHUNK - 1) / THIN_CHUNK;
    PNR_REQUIRE(tiles < (1LL << 31), PNR_E_ARG, "%s: volume extent too large", who);
    // device buffers of the call: the state | the tile stamps | the tile list | the chunk counts | list lengths and deletions | sums
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_S = buf.add<uint8_t>((size_t)N + 16);
    const auto d_stamp = buf.add<unsigned>((size_t)tiles), d_list = buf.add<unsigned>((size_t)tiles);
    const auto d_cnt = buf.add<unsigned>((size_t)chunks), d_ctl = buf.add<unsigned>(12);
    const auto d_sum = buf.add<unsigned long long>(2); // the byte sum of thr = -1 | n_fg
    int rc = buf.alloc(who);
    if (rc) return rc;
    int t = o.thr;
    if (o.thr < 0 && (rc = pnr_mean_threshold(c, who, "thin_threshold", c->d_img, N, d_sum, &t))) return rc; // the global mean
    pnr::Call call(c, who);
    const Grid ga{d_S, w, h, l, tiles_x, tiles_y, tiles_z};
    unsigned long long *d_nfg = d_sum.get() + 1;
    call.fill(d_nfg, 0, 1);
    call.fill(d_stamp, 0);
    call.fill(d_S.get() + N, 0, 16); // (the padding thin_finish reads)
    call.timed("thin_init", thin_init, dim3(blocks_for((N + TPB - 1) / TPB)), dim3(TPB), c->d_img, d_S.get(), (long long)N, t, d_nfg);
    unsigned long long n_fg = 0;
    call.down(&n_fg, d_nfg, 1);
    int32_t rounds = 0;
    int64_t visits = 0;
    unsigned ctl[9]; // the list lengths of the eight passes | the deletions of the round
    const unsigned nt = (unsigned)tiles, grid = blocks_for(tiles), plan_grid = (unsigned)((tiles + TPB - 1) / TPB);
    for (;;) {
        rounds++;
        const bool all = rounds == 1; // every tile, no list
        const unsigned lo = all ? 0u : 8u * (unsigned)(rounds - 2) + 1u;
        call.fill(d_ctl, 0);
        for (int s = 0; s < 8; s++) {
            unsigned *cnt = d_ctl.get() + s;
            const unsigned *list = all ? nullptr : d_list.get();
            if (!all) {
                c->tic();
                call.launch(thin_plan, dim3(plan_grid), dim3(TPB), d_stamp.get(), tiles_x, tiles_y, tiles_z, lo, d_list.get(), cnt);
                c->toc("thin_pass", 1);
            }
            if (s == 0) {
                call.timed("thin_mark", thin_mark, dim3(grid), dim3(TPB), ga, list, (const unsigned *)cnt, nt);
            }
            call.timed("thin_pass", thin_pass, dim3(grid), dim3(TPB), ga, list, (const unsigned *)cnt, nt, s, 8u * (unsigned)(rounds - 1) + (unsigned)s + 1u, d_stamp.get(),
                       d_ctl.get() + 8);
        }
        call.down(ctl, d_ctl.get(), 9);
        if ((rc = call.finish())) return rc;
        for (int s = 0; s < 8; s++) visits += all ? tiles : (int64_t)ctl[s];
        if (ctl[8] == 0 || rounds == o.max_rounds) break;
        PNR_REQUIRE(rounds < (1 << 28), PNR_E_ARG, "%s: too many rounds", who);
    }
    // the skeleton in raster order: the chunk counts become their exclusive scan
    call.timed("thin_list", thin_count, dim3((unsigned)chunks), dim3(TPB), (const uint8_t *)d_S.get(), (long long)N, d_cnt.get());
    std::vector<unsigned> cnt((size_t)chunks);
    call.down(cnt.data(), d_cnt);
    if ((rc = call.finish())) return rc;
    const int64_t K = pnr::exclusive_scan_counts(cnt);
    const size_t k = (size_t)K;
    std::vector<unsigned> vox(k);
    std::vector<uint8_t> deg(k);
    pnr::CallBuf lbuf;
    const auto l_vox = lbuf.add<unsigned>(k);
    const auto l_deg = lbuf.add<uint8_t>(k);
    if (K > 0) {
        if ((rc = lbuf.alloc(who))) return rc;
        call.up(d_cnt, cnt.data());
        call.timed("thin_list", thin_list, dim3((unsigned)chunks), dim3(TPB), ga, (long long)N, (const unsigned *)d_cnt.get(), l_vox.get(), l_deg.get());
        call.down(vox.data(), l_vox);
        call.down(deg.data(), l_deg);
    }
    if (skel_out) {
        const long long words = (N + 3) >> 2;
        call.timed("thin_finish", thin_finish, dim3(blocks_for((words + TPB - 1) / TPB)), dim3(TPB), (unsigned *)d_S.get(), words);
        call.down(skel_out, (const uint8_t *)d_S.get(), (size_t)N);
    }
    if ((rc = call.finish())) return rc;
    int64_t n_end = 0, n_branch = 0, n_isolated = 0;
    for (uint8_t d : deg) n_end += d == 1, n_branch += d >= 3, n_isolated += d == 0;
    if (info) *info = pnr_thin_info{N, (int64_t)n_fg, K, n_end, n_branch, n_isolated, tiles, visits, rounds, t};
    const size_t fill = (size_t)std::min<int64_t>(cap, K);
    if (vox_out)
        for (size_t i = 0; i < fill; i++) vox_out[i] = (int64_t)vox[i];
    if (deg_out && fill) std::memcpy(deg_out, deg.data(), fill);
    return PNR_OK;
}

namespace pnr {

int skeleton_forest(const char *who, const int64_t *vox, int64_t k, int64_t w, int64_t h, int64_t l, std::vector<pnr_bridge> &out)
{
    const int64_t N = w * h * l;
    std::vector<std::pair<int64_t, int32_t>> at((size_t)k); // (voxel, node), sorted by voxel
    for (int64_t i = 0; i < k; i++) {
        PNR_REQUIRE(vox[i] >= 0 && vox[i] < N, PNR_E_ARG, "%s: voxel %lld of node %lld is outside the grid", who, (long long)vox[i], (long long)i);
        at[(size_t)i] = {vox[i], (int32_t)i};
    }
    std::sort(at.begin(), at.end());
    for (int64_t i = 1; i < k; i++) PNR_REQUIRE(at[(size_t)i].first != at[(size_t)i - 1].first, PNR_E_ARG, "%s: voxel %lld is listed twice", who, (long long)at[(size_t)i].first);
    struct Edge {
        int32_t len2, lo, hi;
    };
    std::vector<Edge> edges;
    for (int64_t i = 0; i < k; i++) {
        const int64_t v = at[(size_t)i].first, x = v % w, y = v / w % h, z = v / (w * h);
        for (int dz = 0; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if (!(dz > 0 || dy > 0 || (dy == 0 && dx > 0))) continue; // the 13 forward neighbours
                    const int64_t nx = x + dx, ny = y + dy, nz = z + dz;
                    if (nx < 0 || nx >= w || ny < 0 || ny >= h || nz >= l) continue;
                    const int64_t u = (nz * h + ny) * w + nx;
                    const auto it = std::lower_bound(at.begin() + i + 1, at.end(), std::make_pair(u, (int32_t)0));
                    if (it == at.end() || it->first != u) continue;
                    const int32_t a = at[(size_t)i].second, b = it->second;
                    edges.push_back(Edge{dx * dx + dy * dy + dz * dz, std::min(a, b), std::max(a, b)});
                }
    }
    std::sort(edges.begin(), edges.end(), [](const Edge &p, const Edge &q) { return p.len2 != q.len2 ? p.len2 < q.len2 : p.lo != q.lo ? p.lo < q.lo : p.hi < q.hi; });
    std::vector<int32_t> up((size_t)k);
    for (int64_t i = 0; i < k; i++) up[(size_t)i] = (int32_t)i;
    auto find = [&](int32_t a) {
        while (up[(size_t)a] != a) a = up[(size_t)a] = up[(size_t)up[(size_t)a]];
        return a;
    };
    std::vector<Edge> kept;
    for (const Edge &e : edges) {
        const int32_t a = find(e.lo), b = find(e.hi);
        if (a == b) continue;
        up[(size_t)std::max(a, b)] = std::min(a, b);
        kept.push_back(e);
    }
    std::sort(kept.begin(), kept.end(), [](const Edge &p, const Edge &q) { return p.lo != q.lo ? p.lo < q.lo : p.hi < q.hi; });
    out.clear();
    for (const Edge &e : kept) out.push_back(pnr_bridge{e.lo, e.hi, sqrtf((float)e.len2)});
    return PNR_OK;
}

} // namespace pnr
