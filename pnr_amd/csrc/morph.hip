// morph.hip -- grey-level morphological reconstruction of the traced u8 volume (pnr_morph_reconstruct, pnr_morph_volume).  The rule
// (include/pnr_hip.h): R = rho_C(M, V) is the least volume with R >= min(M, V) and R(p) = min(V(p), max(R(p), max over the C-neighbours
// q of R(q))).  It is found from below: the state starts as min(M, V), every update replaces R(p) by min(V(p), max of itself and its
// neighbours).  A value held at any time is a lower bound of the fixed point, so values only rise, a stale neighbour value is still a
// lower bound, and when no voxel can rise the recursion holds everywhere.  Order, tiling and launch cuts decide the number of visits,
// never a bit.  The erosion forms (ERODE, FILL) run as the dilation of the complements: the state holds 255 - R, V is complemented
// when a tile is staged, and morph_finish turns the state back.
//
//   morph_init     a thread per voxel: the state from the op -- min(M, V) of the uploaded marker (DILATE), min(255 - M, 255 - V) (ERODE),
//                  255 - V on the border set and 0 elsewhere (FILL), max(V - h, 0) (HMAX, HDOME).
//   morph_relax    a work-group per listed tile.  It loads the state of the tile and its halo of 1 and the mask bytes of the tile into LDS
//                  (non-existent cells: 0), then iterates in LDS: a thread owns a line and runs a forward and a backward running
//                  min(V, max(R, previous)) along it -- the x rows, then the y columns, then (C = 6, 26) the z columns, the halo cell in
//                  front of a line as its first `previous` --, which carries a value any distance along an axis in one pass; with C = 8 or
//                  26 one step over the full 3 x 3 (x 3) neighbourhood follows, reads and writes separated by a barrier.  It stops when an
//                  iteration changed nothing -- every voxel was then compared with each of its neighbours while nothing was written --
//                  or after `iters` iterations.  Changed bytes are stored; a stale halo byte is a lower bound.  No atomic touches a
//                  voxel.  The rounds, the flags and who marks whom: tilework.h; in round 1 every tile is listed.
//   morph_finish   the state becomes the result in place (255 - R for the erosion forms, V - R for HDOME), four bytes at a time where
//                  the alignment of V allows, with the statistics as block partials and one set of atomics per work-group.
#include "morph.h"
#include "call.h"
#include "grid.h"
#include "tilework.h"
#include <vector>

namespace {

using pnr::MORPH_TPB;
using pnr::MORPH_TX;
using pnr::MORPH_TY;
using pnr::MORPH_TZ;
typedef unsigned long long u64;

constexpr int HX = MORPH_TX + 2, HY = MORPH_TY + 2, HZ = MORPH_TZ + 2, SXY = HX * HY, CELLS = SXY * HZ;
constexpr int RTPB = MORPH_TX * MORPH_TY; // threads of a relaxation work-group
constexpr int AUTO_ITERS = 64;            // LDS iterations per tile visit (option morph_iters = 0)
static_assert(pnr::tile_shape_ok<MORPH_TX, MORPH_TY, MORPH_TZ, MORPH_TPB>());
using Dims = pnr::TileDims;

struct InitArgs {
    const uint8_t *V;
    uint8_t *R; // ops 1, 2: holds the marker
    long long N;
    int w, h, l, op, hh;
    int border_z; // FILL: the first and the last slice belong to the border set
};

__global__ __launch_bounds__(MORPH_TPB) void morph_init(InitArgs a)
{
    const long long i = (long long)blockIdx.x * MORPH_TPB + threadIdx.x;
    if (i >= a.N) return;
    const unsigned v = a.V[i];
    unsigned r;
    if (a.op == PNR_MORPH_DILATE) r = min((unsigned)a.R[i], v);
    else if (a.op == PNR_MORPH_ERODE) r = 255u - max((unsigned)a.R[i], v);
    else if (a.op == PNR_MORPH_FILL) {
        const int x = (int)(i % a.w), y = (int)(i / a.w % a.h), z = (int)(i / ((long long)a.w * a.h));
        const bool border = x == 0 || x == a.w - 1 || y == 0 || y == a.h - 1 || (a.border_z && (z == 0 || z == a.l - 1));
        r = border ? 255u - v : 0u;
    } else r = v > (unsigned)a.hh ? v - (unsigned)a.hh : 0u;
    a.R[i] = (uint8_t)r;
}

struct RelaxArgs {
    const uint8_t *V;
    uint8_t *R;
    const int *list; // the tiles of this launch
    int *flag_next;
    Dims d;
    int iters, conn;
    unsigned cmpl; // 255: the mask is 255 - V (the erosion forms), 0: V
};

// forward and backward along the N cells base, base + stride, ...; the cells in front of both ends are the halo.  Returns whether a cell rose.
template <int N>
__device__ inline int scan_line(uint8_t *sr, const uint8_t *sv, int base, int stride)
{
    int ch = 0;
    unsigned p = sr[base - stride];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int cell = base + k * stride;
        const unsigned r0 = sr[cell], r = min((unsigned)sv[cell], max(r0, p));
        if (r != r0) sr[cell] = (uint8_t)r, ch = 1;
        p = r;
    }
    p = sr[base + N * stride];
#pragma unroll
    for (int k = N - 1; k >= 0; k--) {
        const int cell = base + k * stride;
        const unsigned r0 = sr[cell], r = min((unsigned)sv[cell], max(r0, p));
        if (r != r0) sr[cell] = (uint8_t)r, ch = 1;
        p = r;
    }
    return ch;
}

__global__ __launch_bounds__(RTPB) void morph_relax(RelaxArgs a)
{
    __shared__ uint8_t sr[CELLS]; // the state; 0: outside the volume
    __shared__ uint8_t sv[CELLS]; // the mask of the tile's own cells; 0: outside the volume (such a cell stays 0) and in the halo (never read)
    __shared__ unsigned touched;  // the halo_bits of the voxels that changed
    const Dims d = a.d;
    const int tile = a.list[blockIdx.x];
    const pnr::TileAt o = pnr::tile_origin((unsigned)tile, d.ntx, d.nty, MORPH_TX, MORPH_TY, MORPH_TZ);
    if (threadIdx.x == 0) touched = 0;
    pnr::stage_cells<MORPH_TX, MORPH_TY, MORPH_TZ>(d, o, [&](int cx, int cy, int cz, bool inside, long long g, bool own_cell) {
        unsigned r = 0, v = 0;
        if (inside) {
            r = __hip_atomic_load(&a.R[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (another tile may be writing its bytes)
            if (own_cell) v = a.V[g] ^ a.cmpl;
        }
        const int cell = (cz * HY + cy) * HX + cx;
        sr[cell] = (uint8_t)r, sv[cell] = (uint8_t)v;
    });
    __syncthreads();
    const int lx = threadIdx.x % MORPH_TX, ly = threadIdx.x / MORPH_TX;
    const int own = (HY + ly + 1) * HX + lx + 1; // the cell of the thread's voxel z = 0; z + 1 is SXY further
    unsigned first[MORPH_TZ];
#pragma unroll
    for (int z = 0; z < MORPH_TZ; z++) first[z] = sr[own + z * SXY];
    const bool with_z = a.conn == 6 || a.conn == 26, with_diag = a.conn == 8 || a.conn == 26, diag_z = a.conn == 26;
    int again = 0;
    for (int it = 0; it < a.iters; it++) {
        int changed = 0;
        for (int line = threadIdx.x; line < MORPH_TY * MORPH_TZ; line += RTPB) // the x rows
            changed |= scan_line<MORPH_TX>(sr, sv, ((line / MORPH_TY + 1) * HY + line % MORPH_TY + 1) * HX + 1, 1);
        __syncthreads();
        for (int line = threadIdx.x; line < MORPH_TX * MORPH_TZ; line += RTPB) // the y columns
            changed |= scan_line<MORPH_TY>(sr, sv, ((line / MORPH_TX + 1) * HY + 1) * HX + line % MORPH_TX + 1, HX);
        __syncthreads();
        if (with_z) {
            changed |= scan_line<MORPH_TZ>(sr, sv, own, SXY); // the thread's own z column
            __syncthreads();
        }
        if (with_diag) {
            unsigned m[HZ]; // the maximum over the 9 columns around the thread's, per plane of the tile and its halo
#pragma unroll
            for (int q = 0; q < HZ; q++) m[q] = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int col = own - SXY + dy * HX + dx; // the neighbouring column's cell at z = -1
#pragma unroll
                    for (int q = 0; q < HZ; q++) m[q] = max(m[q], (unsigned)sr[col + q * SXY]);
                }
            unsigned nw[MORPH_TZ];
#pragma unroll
            for (int z = 0; z < MORPH_TZ; z++) {
                const unsigned best = diag_z ? max(m[z], max(m[z + 1], m[z + 2])) : m[z + 1]; // (holds the voxel's own value)
                nw[z] = min((unsigned)sv[own + z * SXY], best);
            }
            __syncthreads(); // every read of this step is done
#pragma unroll
            for (int z = 0; z < MORPH_TZ; z++)
                if (nw[z] > sr[own + z * SXY]) sr[own + z * SXY] = (uint8_t)nw[z], changed = 1;
        }
        again = __syncthreads_or(changed); // ... and every write
        if (!again) break;
    }
    unsigned mine = 0;
#pragma unroll
    for (int z = 0; z < MORPH_TZ; z++) {
        const unsigned cur = sr[own + z * SXY];
        if (cur != first[z]) { // (a voxel inside the volume: the others stay 0)
            const long long g = pnr::voxel_index(d.w, d.h, o.x0 + lx, o.y0 + ly, o.z0 + z);
            __hip_atomic_store(&a.R[g], (uint8_t)cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mine |= pnr::halo_bits<MORPH_TX, MORPH_TY, MORPH_TZ>(lx, ly, z);
        }
    }
    pnr::mark_tiles(a.flag_next, d, o, tile, touched, mine, again);
}

// st (zeroed by the host): n_changed | n_nonzero | sum_in | sum_out | max_delta
struct Stats {
    u64 n_changed = 0, n_nonzero = 0, sum_in = 0, sum_out = 0;
    unsigned max_delta = 0;
    __device__ inline unsigned add(unsigned v, unsigned r, unsigned cmpl, bool dome)
    {
        const unsigned s = r ^ cmpl, out = dome ? v - s : s, delta = out > v ? out - v : v - out;
        n_changed += out != v, n_nonzero += out != 0, sum_in += v, sum_out += out;
        max_delta = max(max_delta, delta);
        return out;
    }
};

// R becomes the result in place.  head: the bytes in front of the first 4-byte boundary of V and R alike, nvec: the words behind them
// (0 where the two are not aligned alike: then every byte goes the scalar way, head = N)
__global__ __launch_bounds__(MORPH_TPB) void morph_finish(const uint8_t *V, uint8_t *R, long long N, long long head, long long nvec, unsigned cmpl, int dome, u64 *st)
{
    __shared__ u64 part[5 * (MORPH_TPB / 64)];
    const long long gid = (long long)blockIdx.x * MORPH_TPB + threadIdx.x, stride = (long long)gridDim.x * MORPH_TPB;
    Stats s;
    const unsigned *v4 = (const unsigned *)(V + head);
    unsigned *r4 = (unsigned *)(R + head);
    for (long long g = gid; g < nvec; g += stride) {
        const unsigned v = v4[g], r = r4[g];
        unsigned out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) out |= s.add(v >> (8 * k) & 255u, r >> (8 * k) & 255u, cmpl, dome != 0) << (8 * k);
        r4[g] = out;
    }
    const long long t0 = head + 4 * nvec; // the scalar bytes: [0, head) and [t0, N)
    for (long long i = gid; i < head + (N - t0); i += stride) {
        const long long at = i < head ? i : t0 + (i - head);
        R[at] = (uint8_t)s.add(V[at], R[at], cmpl, dome != 0);
    }
    u64 w[5] = {s.n_changed, s.n_nonzero, s.sum_in, s.sum_out, s.max_delta};
#pragma unroll
    for (int k = 0; k < 5; k++)
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const u64 other = (u64)__shfl_xor((long long)w[k], sh, 64);
            w[k] = k == 4 ? max(w[k], other) : w[k] + other;
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 5; k++) part[5 * wave + k] = w[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < MORPH_TPB / 64; i++)
            for (int k = 0; k < 5; k++) w[k] = k == 4 ? max(w[k], part[5 * i + k]) : w[k] + part[5 * i + k];
        for (int k = 0; k < 4; k++)
            if (w[k]) atomicAdd(&st[k], w[k]);
        if (w[4]) atomicMax(&st[4], w[4]);
    }
}

} // namespace

int pnr_morph_run(pnr_ctx *c, const char *who, const pnr_morph_opts &o, const uint8_t *marker, pnr_morph_info *info, uint8_t *out, pnr::DevBuf<uint8_t> *keep)
{
    const int64_t N = c->N;
    Dims d;
    int rc = pnr::tile_dims<MORPH_TX, MORPH_TY, MORPH_TZ>(c, who, d);
    if (rc) return rc;
    const int64_t tiles = d.tiles(), vblocks = (N + MORPH_TPB - 1) / MORPH_TPB;
    const bool erosion = o.op == PNR_MORPH_ERODE || o.op == PNR_MORPH_FILL;
    const unsigned cmpl = erosion ? 255u : 0u;
    pnr::DevBuf<uint8_t> state; // (freed when the call returns, or handed to the caller)
    if ((rc = pnr::dev_alloc(state, (size_t)N, who, "for the state volume"))) return rc;
    pnr::CallBuf buf; // (freed when the call returns)
    pnr::TileRounds rounds(c, who, buf, d);
    const auto d_st = buf.add<u64>(5);
    if ((rc = buf.alloc(who)) || (rc = rounds.pin())) return rc;
    pnr::Call call(c, who);
    uint8_t *const R = state.get();
    if (marker) call.up(R, marker, (size_t)N);
    call.timed("morph_init", morph_init, dim3((unsigned)vblocks), dim3(MORPH_TPB),
               InitArgs{c->d_img, R, (long long)N, d.w, d.h, d.l, o.op, o.h, (o.connectivity == 6 || o.connectivity == 26) && d.l > 1 ? 1 : 0});
    rounds.seed_all(call);
    const int iters = c->opt.morph_iters > 0 ? c->opt.morph_iters : AUTO_ITERS;
    pnr::TileRounds::Tally done;
    c->morph_rounds = c->morph_visits = 0;
    // (a voxel rises at most 255 times, and a round without a rise is the last but one)
    rc = rounds.run(call, "morph_compact", pnr::tiles_per_launch(c->opt.morph_tiles_per_launch), 256 * N + tiles + 16, 0, [&](const int *list, int64_t n, int *flag_next) {
        call.timed("morph_relax", morph_relax, dim3((unsigned)n), dim3(RTPB), RelaxArgs{c->d_img, R, list, flag_next, d, iters, o.connectivity, cmpl});
    }, done);
    if (rc) return rc;
    c->morph_rounds = done.rounds, c->morph_visits = done.visits;
    const uintptr_t av = (uintptr_t)c->d_img, ar = (uintptr_t)R;
    const bool alike = (av & 3) == (ar & 3);
    const long long head = alike ? std::min<long long>(N, (long long)((4 - (av & 3)) & 3)) : (long long)N, nvec = (N - head) >> 2;
    u64 st[5] = {0, 0, 0, 0, 0};
    call.fill(d_st, 0);
    call.timed("morph_finish", morph_finish, dim3(pnr::grid_blocks((std::max<long long>(nvec, head + 4) + MORPH_TPB - 1) / MORPH_TPB)), dim3(MORPH_TPB), c->d_img, R, (long long)N,
               head, nvec, cmpl, o.op == PNR_MORPH_HDOME ? 1 : 0, d_st.get());
    call.down(st, d_st);
    if (out) call.down(out, (const uint8_t *)R, (size_t)N);
    if ((rc = call.finish())) return rc;
    if (info)
        *info = pnr_morph_info{N, (int64_t)st[0], (int64_t)st[1], st[2], st[3], tiles, done.visits, (int32_t)st[4], o.connectivity, (int32_t)std::min<int64_t>(done.rounds, INT32_MAX), 0};
    if (keep) *keep = std::move(state);
    return PNR_OK;
}
