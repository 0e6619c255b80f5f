// geodesic.hip -- the gray-weighted geodesic distance through the traced u8 volume (pnr_geodesic_distance).  The rule
// (include/pnr_hip.h): passable V >= t; an edge between 26-neighbours p, q = p + o costs len[o] (c(V(p)) + c(V(q))); every voxel's u64 key
// (D << 32) | label is the minimum over its passable neighbours q with D(q) + wt <= dmax of key(q) + (wt << 32), a source voxel's is
// (0, its smallest label).  The keys are the unique solution of that recursion; they are found from above: all NONE but the sources, then
// every visit of a voxel replaces its key by the minimum of itself and its neighbours' candidates.  A key held at any time is the
// (cost, label) of a real path, so keys only decrease, a stale neighbour key is still an upper bound, and when no voxel can be lowered
// the recursion holds everywhere.  Order, tiling and launch cuts decide the number of visits, never a bit.
//
//   geo_sources  a thread per source: the centre voxel; a passable one takes the label with a 64-bit atomic minimum (D = 0) and marks its
//                tile and the tiles of its 26 neighbours; the others are counted as dropped.  The keys were filled with ones before.
//   geo_relax    a work-group per listed tile.  It loads the keys and costs of the tile and its halo of 1 into LDS (impassable and
//                non-existent cells: NONE, cost 0; keys with relaxed agent-scope atomic loads, another tile may be writing them), then
//                iterates in LDS: a thread owns the GEO_TZ voxels of a z column and gathers, for each of the 9 neighbouring columns, the 6
//                keys once for the 3 dz of all its voxels.  Reads and writes of an iteration are separated by barriers.  It stops when an
//                iteration changed nothing, or after `iters` iterations.  Changed keys are stored (atomic, so that a reader never sees
//                half a key).  The rounds, the flags and who marks whom: tilework.h; round 1 lists the tiles geo_sources marked.  Rounds ~
//                tiles along the longest path, not voxels along it.
//   geo_stats    n_pass, n_reached and the maximum of (D << 32) | ~index over the reached voxels (one 64-bit atomic maximum per
//                work-group): the largest D and the smallest index that attains it.
//   geo_split    D and L from the keys where the caller asks for the volumes.
//   geo_sample / geo_paths   a thread per target: the key at its centre voxel; the walk along pred() of at most path_cap voxels
//                (pnr_geo_targets: the stage with its own buffers, after the statistics and the split).
//   hook         a caller's function that runs once the keys have settled (geodesic.h): it sees the device keys, may run the target
//                stage itself and may replace the targets of the call (geojoin.hip: the bridges between the sources' trees).
#include "geodesic.h"
#include "call.h"
#include "grid.h"
#include "tilework.h"
#include "volume.h"
#include <cmath>
#include <vector>

namespace {

using pnr::GEO_TPB;
using pnr::GEO_TX;
using pnr::GEO_TY;
using pnr::GEO_TZ;
typedef unsigned long long u64;

constexpr u64 NONE = ~0ull;
constexpr int HX = GEO_TX + 2, HY = GEO_TY + 2, HZ = GEO_TZ + 2, CELLS = HX * HY * HZ;
constexpr int RTPB = GEO_TX * GEO_TY; // threads of a relaxation work-group
constexpr int AUTO_ITERS = 128;       // LDS iterations per tile visit (option geo_iters = 0)
static_assert(pnr::tile_shape_ok<GEO_TX, GEO_TY, GEO_TZ, GEO_TPB>());

using Dims = pnr::GeoDims;
using Lens = pnr::GeoLens;

using pnr::finite3;
// the centre voxel of the radius rule
__device__ inline long long centre(const Dims &d, float px, float py, float pz) { return pnr::centre_voxel(d.w, d.h, d.l, px, py, pz); }
__device__ inline u64 load_key(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(GEO_TPB) void geo_sources(const uint8_t *V, u64 *key, const float *xyz, const int *label, long long n, Dims d, int t, int *flag,
                                                        u64 *dropped)
{
    const long long i = (long long)blockIdx.x * GEO_TPB + threadIdx.x;
    if (i >= n) return;
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    long long g = -1;
    if (finite3(px, py, pz)) {
        g = centre(d, px, py, pz);
        if ((int)V[g] < t) g = -1;
    }
    if (g < 0) {
        atomicAdd(dropped, 1ull);
        return;
    }
    atomicMin(&key[g], (u64)(unsigned)(label ? label[i] : (int)i)); // D = 0
    // its tile, and every tile that holds one of its 26 neighbours: a source on a tile's face is in their halo, and its own tile never
    // sees it change
    const int x = (int)(g % d.w), y = (int)(g / d.w % d.h), z = (int)(g / ((long long)d.w * d.h));
    for (int qz = max(z - 1, 0); qz <= min(z + 1, d.l - 1); qz++)
        for (int qy = max(y - 1, 0); qy <= min(y + 1, d.h - 1); qy++)
            for (int qx = max(x - 1, 0); qx <= min(x + 1, d.w - 1); qx++) flag[((long long)(qz / GEO_TZ) * d.nty + qy / GEO_TY) * d.ntx + qx / GEO_TX] = 1;
}

struct RelaxArgs {
    const uint8_t *V;
    u64 *key;
    const uint16_t *ctab;
    const int *list; // the tiles of this launch
    int *flag_next;
    Dims d;
    int t, iters;
    unsigned dmax;
    Lens len;
};

__global__ __launch_bounds__(RTPB) void geo_relax(RelaxArgs a)
{
    __shared__ u64 sk[CELLS];
    __shared__ unsigned short sc[CELLS]; // 0: impassable or outside the volume
    __shared__ unsigned touched;         // the halo_bits of the voxels that changed
    const Dims d = a.d;
    const int tile = a.list[blockIdx.x];
    const pnr::TileAt o = pnr::tile_origin((unsigned)tile, d.ntx, d.nty, GEO_TX, GEO_TY, GEO_TZ);
    if (threadIdx.x == 0) touched = 0;
    pnr::stage_cells<GEO_TX, GEO_TY, GEO_TZ>(d, o, [&](int cx, int cy, int cz, bool inside, long long g, bool) {
        u64 k = NONE;
        unsigned short cc = 0;
        if (inside) {
            const int v = a.V[g];
            if (v >= a.t) cc = a.ctab[v], k = load_key(&a.key[g]);
        }
        const int cell = (cz * HY + cy) * HX + cx;
        sk[cell] = k, sc[cell] = cc;
    });
    __syncthreads();
    const int lx = threadIdx.x % GEO_TX, ly = threadIdx.x / GEO_TX;
    const int own = (HY + ly + 1) * HX + lx + 1; // the cell of the thread's voxel z = 0; z + 1 is HX * HY further
    u64 cur[GEO_TZ], first[GEO_TZ];
    unsigned cp[GEO_TZ];
#pragma unroll
    for (int z = 0; z < GEO_TZ; z++) cur[z] = first[z] = sk[own + z * HX * HY], cp[z] = sc[own + z * HX * HY];
    int again = 0;
    for (int it = 0; it < a.iters; it++) {
        u64 best[GEO_TZ];
#pragma unroll
        for (int z = 0; z < GEO_TZ; z++) best[z] = cur[z];
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int col = own - HX * HY + dy * HX + dx; // the neighbouring column's cell at z = -1
                u64 kq[HZ];
                unsigned cq[HZ];
#pragma unroll
                for (int q = 0; q < HZ; q++) kq[q] = sk[col + q * HX * HY], cq[q] = sc[col + q * HX * HY];
#pragma unroll
                for (int z = 0; z < GEO_TZ; z++)
#pragma unroll
                    for (int dz = -1; dz <= 1; dz++) {
                        if (dx == 0 && dy == 0 && dz == 0) continue;
                        const int q = z + 1 + dz;
                        const unsigned wt = a.len.v[(dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)] * (cp[z] + cq[q]); // (at most 2^31 - 1: checked by the host)
                        // an impassable or unreached q has D = 2^32 - 1; an impassable own voxel (cp = 0) stays NONE
                        if (cp[z] && wt <= a.dmax && (unsigned)(kq[q] >> 32) <= a.dmax - wt) best[z] = min(best[z], kq[q] + ((u64)wt << 32));
                    }
            }
        int changed = 0;
#pragma unroll
        for (int z = 0; z < GEO_TZ; z++) changed |= best[z] < cur[z];
        __syncthreads(); // every read of this iteration is done
#pragma unroll
        for (int z = 0; z < GEO_TZ; z++)
            if (best[z] < cur[z]) cur[z] = best[z], sk[own + z * HX * HY] = best[z];
        again = __syncthreads_or(changed); // ... and every write
        if (!again) break;
    }
    unsigned mine = 0;
#pragma unroll
    for (int z = 0; z < GEO_TZ; z++)
        if (cur[z] < first[z]) { // (a passable voxel inside the volume: the others stay NONE)
            const long long g = pnr::voxel_index(d.w, d.h, o.x0 + lx, o.y0 + ly, o.z0 + z);
            __hip_atomic_store(&a.key[g], cur[z], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mine |= pnr::halo_bits<GEO_TX, GEO_TY, GEO_TZ>(lx, ly, z);
        }
    pnr::mark_tiles(a.flag_next, d, o, tile, touched, mine, again);
}

// out: n_pass | n_reached | the maximum of (D << 32) | ~index over the reached voxels (zeroed by the host)
__global__ __launch_bounds__(GEO_TPB) void geo_stats(const uint8_t *V, const u64 *key, long long N, int t, u64 *out)
{
    __shared__ u64 part[3 * (GEO_TPB / 64)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 n_pass = 0, n_reached = 0, top = 0;
    const long long stride = (long long)gridDim.x * GEO_TPB;
    for (long long base = (long long)blockIdx.x * GEO_TPB; base < N; base += stride) { // (wave-uniform: the ballots see whole waves)
        const long long i = base + threadIdx.x;
        const bool in = i < N;
        const u64 k = in ? key[i] : NONE;
        n_pass += (u64)__popcll(__ballot(in && (int)V[i] >= t));
        n_reached += (u64)__popcll(__ballot(k != NONE));
        if (k != NONE) top = max(top, (k & 0xffffffff00000000ull) | (unsigned)~(unsigned)i);
    }
    for (int s = 32; s >= 1; s >>= 1) top = max(top, (u64)__shfl_xor((long long)top, s, 64));
    if (lane == 0) part[3 * wave] = n_pass, part[3 * wave + 1] = n_reached, part[3 * wave + 2] = top;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < GEO_TPB / 64; i++) n_pass += part[3 * i], n_reached += part[3 * i + 1], top = max(top, part[3 * i + 2]);
        if (n_pass) atomicAdd(&out[0], n_pass);
        if (n_reached) atomicAdd(&out[1], n_reached);
        if (top) atomicMax(&out[2], top); // (a reached voxel has ~index > 0: N <= 2^32 - 2)
    }
}

__global__ __launch_bounds__(GEO_TPB) void geo_split(const u64 *key, long long N, unsigned *dv, int *lv)
{
    const long long i = (long long)blockIdx.x * GEO_TPB + threadIdx.x;
    if (i >= N) return;
    const u64 k = key[i];
    if (dv) dv[i] = (unsigned)(k >> 32);
    if (lv) lv[i] = (int)(unsigned)k; // (NONE: -1)
}

__global__ __launch_bounds__(GEO_TPB) void geo_sample(const u64 *key, const float *xyz, long long m, Dims d, unsigned *d_at, int *l_at)
{
    const long long i = (long long)blockIdx.x * GEO_TPB + threadIdx.x;
    if (i >= m) return;
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const u64 k = finite3(px, py, pz) ? key[centre(d, px, py, pz)] : NONE;
    d_at[i] = (unsigned)(k >> 32), l_at[i] = (int)(unsigned)k;
}

struct PathArgs {
    const uint8_t *V;
    const u64 *key;
    const uint16_t *ctab;
    const float *xyz;
    long long m;
    Dims d;
    int cap;
    int *len;
    long long *vox; // m x cap
    Lens step;
};

__global__ __launch_bounds__(GEO_TPB) void geo_paths(PathArgs a)
{
    const long long i = (long long)blockIdx.x * GEO_TPB + threadIdx.x;
    if (i >= a.m) return;
    const Dims d = a.d;
    const float px = a.xyz[3 * i], py = a.xyz[3 * i + 1], pz = a.xyz[3 * i + 2];
    int n = 0;
    if (finite3(px, py, pz)) {
        long long p = centre(d, px, py, pz);
        u64 kp = a.key[p];
        long long *out = a.vox + i * a.cap;
        while (kp != NONE) { // (at most cap + 1 turns)
            if (n == a.cap) {
                n = -a.cap; // cut: cap voxels are written and the source voxel is not among them
                break;
            }
            out[n++] = p;
            if ((kp >> 32) == 0) break; // the source voxel
            const int x = (int)(p % d.w), y = (int)(p / d.w % d.h), z = (int)(p / ((long long)d.w * d.h));
            const unsigned cp = a.ctab[a.V[p]];
            long long q = -1;
            u64 kq = NONE;
            for (int o = 0; o < 27 && q < 0; o++) { // the offset order
                const int qx = x + o % 3 - 1, qy = y + o / 3 % 3 - 1, qz = z + o / 9 - 1;
                if (o == 13 || qx < 0 || qx >= d.w || qy < 0 || qy >= d.h || qz < 0 || qz >= d.l) continue;
                const long long g = pnr::voxel_index(d.w, d.h, qx, qy, qz);
                const u64 k = a.key[g];
                if (k == NONE) continue; // (impassable or unreached)
                const unsigned wt = a.step.v[o] * (cp + a.ctab[a.V[g]]);
                if (k + ((u64)wt << 32) == kp) q = g, kq = k;
            }
            if (q < 0) { // (the rule has a predecessor at every reached voxel with D > 0)
                n = 0;
                break;
            }
            p = q, kp = kq;
        }
    }
    a.len[i] = n;
}

} // namespace

int pnr_geo_targets(pnr_ctx *c, const char *who, const pnr_geo_keys &k, const pnr_geo_call &g)
{
    if (g.m <= 0) return PNR_OK;
    const int64_t m_path = g.path_cap > 0 ? g.m - g.m_no_path : 0;
    const bool paths = m_path > 0;
    pnr::CallBuf buf; // (freed when the stage returns)
    const auto d_axyz = buf.add<float>((size_t)g.m * 3);
    const auto d_dat = buf.add<unsigned>((size_t)g.m);
    const auto d_lat = buf.add<int>((size_t)g.m);
    const auto d_plen = buf.add<int>(paths ? (size_t)m_path : 0);
    const auto d_pvox = buf.add<long long>(paths ? (size_t)m_path * (size_t)g.path_cap : 0);
    const int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::Call call(c, who);
    call.up(d_axyz, g.at_xyz);
    if (g.d_at || g.label_at) {
        call.timed("geodesic_sample", geo_sample, dim3((unsigned)((g.m + GEO_TPB - 1) / GEO_TPB)), dim3(GEO_TPB), k.key, (const float *)d_axyz.get(), (long long)g.m, k.d, d_dat.get(), d_lat.get());
        if (g.d_at) call.down(g.d_at, d_dat);
        if (g.label_at) call.down(g.label_at, d_lat);
    }
    if (paths) {
        call.timed("geodesic_paths", geo_paths, dim3((unsigned)((m_path + GEO_TPB - 1) / GEO_TPB)), dim3(GEO_TPB),
                   PathArgs{k.V, k.key, k.ctab, (const float *)d_axyz.get(), (long long)m_path, k.d, g.path_cap, d_plen.get(), d_pvox.get(), k.len});
        call.down(g.path_len, d_plen);
        call.down(g.path_vox, d_pvox);
    }
    return call.finish();
}

int pnr_geodesic_run(pnr_ctx *c, const char *who, const pnr_geo_opts &o, const pnr_geo_call &g_in)
{
    pnr_geo_call g = g_in; // (the hook may replace the targets)
    const int64_t N = c->N;
    Dims d;
    int rc = pnr::tile_dims<GEO_TX, GEO_TY, GEO_TZ>(c, who, d);
    if (rc) return rc;
    const int64_t tiles = d.tiles(), vblocks = (N + GEO_TPB - 1) / GEO_TPB;
    // the cost table and the step lengths (f32, single operations: this file is built with -ffp-contract=off)
    uint16_t ctab[256];
    unsigned cmax = 0, lmax = 0;
    for (int v = 0; v < 256; v++) ctab[v] = o.cost ? o.cost[v] : (uint16_t)(256 - v), cmax = std::max<unsigned>(cmax, ctab[v]);
    const float zd = c->prm.zdist;
    Lens len{};
    for (int k = 0; k < 27; k++) {
        const int dx = k % 3 - 1, dy = k / 3 % 3 - 1, dz = k / 9 - 1;
        const float f = k == 13 ? 0.f : rintf(32.0f * sqrtf((float)(dx * dx + dy * dy) + (zd * (float)dz) * (zd * (float)dz)));
        // (checked before the cast: a length of 2^30 or more, or one that is not finite, is above the edge bound with any cost)
        PNR_REQUIRE(f >= 0.f && f < 1073741824.f, PNR_E_ARG, "%s: the step length %g is above 2^31 - 1 with any cost (zdist = %g)", who, (double)f, (double)zd);
        len.v[k] = (uint32_t)f;
        lmax = std::max(lmax, len.v[k]);
    }
    PNR_REQUIRE((uint64_t)lmax * 2 * cmax <= 0x7fffffffull, PNR_E_ARG, "%s: the largest edge %u * 2 * %u is above 2^31 - 1 (zdist = %g)", who, lmax, cmax, (double)zd);
    const bool split_d = g.d_out != nullptr, split_l = g.label_out != nullptr;
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_key = buf.add<u64>((size_t)N);
    pnr::TileRounds rounds(c, who, buf, d);
    const auto d_ctab = buf.add<uint16_t>(256);
    const auto d_word = buf.add<u64>(1), d_drop = buf.add<u64>(1), d_st = buf.add<u64>(3);
    const auto d_sxyz = buf.add<float>((size_t)g.n_src * 3);
    const auto d_slab = buf.add<int>(g.src_label ? (size_t)g.n_src : 0);
    const auto d_dv = buf.add<unsigned>(split_d ? (size_t)N : 0);
    const auto d_lv = buf.add<int>(split_l ? (size_t)N : 0);
    if ((rc = buf.alloc(who)) || (rc = rounds.pin())) return rc;
    int t = o.thr;
    if (o.thr < 0 && (rc = pnr_mean_threshold(c, who, "geodesic_threshold", c->d_img, N, d_word, &t))) return rc; // the global mean
    pnr::Call call(c, who);
    call.up(d_ctab, ctab);
    c->tic();
    call.fill(d_key, 0xff);
    rounds.seed_none(call);
    call.fill(d_drop, 0);
    if (g.n_src > 0) {
        call.up(d_sxyz, g.src_xyz);
        if (g.src_label) call.up(d_slab, g.src_label);
        call.launch(geo_sources, dim3((unsigned)((g.n_src + GEO_TPB - 1) / GEO_TPB)), dim3(GEO_TPB), c->d_img, d_key.get(), (const float *)d_sxyz.get(),
                    g.src_label ? (const int *)d_slab.get() : (const int *)nullptr, (long long)g.n_src, d, t, rounds.flag0(), d_drop.get());
    }
    c->toc("geodesic_init", 1);
    const int iters = c->opt.geo_iters > 0 ? c->opt.geo_iters : AUTO_ITERS;
    pnr::TileRounds::Tally done;
    c->geo_rounds = c->geo_visits = 0;
    rc = rounds.run(call, "geodesic_compact", pnr::tiles_per_launch(c->opt.geo_tiles_per_launch), N + tiles + 16, 0, [&](const int *list, int64_t n, int *flag_next) {
        call.timed("geodesic_relax", geo_relax, dim3((unsigned)n), dim3(RTPB),
                   RelaxArgs{c->d_img, d_key.get(), (const uint16_t *)d_ctab.get(), list, flag_next, d, t, iters, o.dmax, len});
    }, done);
    if (rc) return rc;
    c->geo_rounds = done.rounds, c->geo_visits = done.visits;
    const pnr_geo_keys keys{c->d_img, d_key.get(), d_ctab.get(), t, d, len};
    if (g.hook && (rc = g.hook(g.hook_user, c, who, keys, g))) return rc;
    u64 st[3] = {0, 0, 0}, dropped = 0;
    call.down(&dropped, d_drop);
    if (g.info) {
        call.fill(d_st, 0);
        call.timed("geodesic_stats", geo_stats, dim3(pnr::grid_blocks(vblocks)), dim3(GEO_TPB), c->d_img, (const u64 *)d_key.get(), (long long)N, t, d_st.get());
        call.down(st, d_st);
    }
    if (split_d || split_l) {
        call.timed("geodesic_split", geo_split, dim3((unsigned)vblocks), dim3(GEO_TPB), (const u64 *)d_key.get(), (long long)N, split_d ? d_dv.get() : (unsigned *)nullptr,
                   split_l ? d_lv.get() : (int *)nullptr);
        if (split_d) call.down(g.d_out, d_dv);
        if (split_l) call.down(g.label_out, d_lv);
    }
    if ((rc = pnr_geo_targets(c, who, keys, g))) { // (the same stream: behind the statistics and the split)
        (void)hipStreamSynchronize(c->stream); // (the downloads above write into this frame)
        return rc;
    }
    if ((rc = call.finish())) return rc;
    if (g.info) {
        const int64_t reached = (int64_t)st[1];
        *g.info = pnr_geo_info{N, (int64_t)st[0], reached, g.n_src - (int64_t)dropped, (int64_t)dropped, reached ? (int64_t)(uint32_t)~(uint32_t)st[2] : -1,
                               reached ? (uint32_t)(st[2] >> 32) : 0u, t, (int32_t)std::min<int64_t>(done.rounds, INT32_MAX), 0};
    }
    return PNR_OK;
}
