// prune.hip -- the pruning rule of include/pnr_hip.h on the device, behind pnr_prune_tree: heights, paths, branch orders, segments
// and the removal by pointer jumping.  The trees this is for are skeletons and traces: 10^5 to 10^6 nodes in degree-2 chains 10^4 to
// 10^5 long, so nothing here walks a chain; the launches grow with log2(depth).
//
//   prune_edges      q (rule 1), the children per node (one 32-bit atomic add on the parent), the first (anc, dist) = (parent, q)
//   prune_up    x ru round k: every node does ONE atomic max of dist + H_k[self] into H_{k+1}[anc] (H_{k+1} starts as a copy of H_k),
//                    then (anc, dist) <- (anc[anc], dist + dist[anc]).  After round k, H holds the longest downward path among the
//                    descendants fewer than 2^(k+1) edges away, and dist ends as the path from the root.  A root carries (self, 0).
//   prune_child      the continuing child (rule 3): ONE 64-bit atomic max on the parent of (q + H) << 32 | (0xffffffff - index)
//   prune_down_init  heads (rule 4), their own removal (rule 5), the first (anc, order << 1 | removed) = (parent, own) and the first
//                    segment pointer (self for a head, else the parent)
//   prune_down  x rd the same jumping downward: sums for the order, OR for the removal; the segment pointer stops at a head
//   prune_finish     rule 5 for the roots, the outputs and the sums of pnr_prune_info (wave shuffles, one atomic per wave and value)
//
// A round raises a word of `flags` while a pointer it read was not yet final; the host reads those 4 bytes back after the launch
// (as morph.hip reads its count) and stops after the first round that raised nothing.  Every sum that could reach 2^32 is taken in
// 64 bits, raises flags[FLAG_RANGE] and is clamped, so nothing wraps before the host refuses the call (rule 7).
#include "prune.h"
#include "call.h"
#include "grid.h"

namespace {

typedef unsigned long long u64;
constexpr int PTPB = 256;
constexpr int MAX_ROUNDS = 40; // n < 2^31: 32 rounds at the most
constexpr int FLAG_RANGE = MAX_ROUNDS, N_FLAGS = MAX_ROUNDS + 1;

__device__ inline u64 pack(unsigned lo, unsigned hi) { return (u64)hi << 32 | lo; }
__device__ inline unsigned sum_u32(unsigned a, unsigned b, unsigned *flags)
{
    const u64 s = (u64)a + b;
    if (s >> 32) flags[FLAG_RANGE] = 1;
    return s >> 32 ? 0xffffffffu : (unsigned)s;
}

// A (out) = anc | dist << 32
__global__ __launch_bounds__(PTPB) void prune_edges(const float *__restrict__ xyz, const int *__restrict__ parent, int n, pnr::PruneRule rule, unsigned *__restrict__ q,
                                                    unsigned *__restrict__ kids, u64 *__restrict__ A, unsigned *__restrict__ flags)
{
    const int i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= n) return;
    const int p = parent[i];
    unsigned e = 0;
    if (p >= 0) {
        const float a[3] = {xyz[3 * (long long)i], xyz[3 * (long long)i + 1], xyz[3 * (long long)i + 2]};
        const float b[3] = {xyz[3 * (long long)p], xyz[3 * (long long)p + 1], xyz[3 * (long long)p + 2]};
        const double d = rule.edge(a, b);
        if (!(d < pnr::PRUNE_LIMIT)) flags[FLAG_RANGE] = 1;
        e = d < pnr::PRUNE_LIMIT ? (unsigned)d : 0xffffffffu;
        atomicAdd(&kids[p], 1u);
    }
    q[i] = e;
    A[i] = pack(p >= 0 ? (unsigned)p : (unsigned)i, e);
}

__global__ __launch_bounds__(PTPB) void prune_up(const u64 *__restrict__ A, u64 *__restrict__ An, const unsigned *__restrict__ H, unsigned *__restrict__ Hn, int n, int round,
                                                 unsigned *__restrict__ flags)
{
    const int i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= n) return;
    const u64 mine = A[i];
    const unsigned anc = (unsigned)mine, dist = (unsigned)(mine >> 32);
    const u64 up = A[anc];
    if ((unsigned)up != anc) flags[round] = 1; // anc is no root yet: another round
    An[i] = pack((unsigned)up, sum_u32(dist, (unsigned)(up >> 32), flags));
    if (anc != (unsigned)i) atomicMax(&Hn[anc], sum_u32(dist, H[i], flags));
}

__global__ __launch_bounds__(PTPB) void prune_child(const int *__restrict__ parent, const unsigned *__restrict__ q, const unsigned *__restrict__ H, int n, u64 *__restrict__ best)
{
    const int i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= n) return;
    const int p = parent[i];
    if (p >= 0) atomicMax(&best[p], pack(0xffffffffu - (unsigned)i, q[i] + H[i])); // (q + H < 2^32: the heights raised no range flag)
}

// D (out) = anc | (order << 1 | removed) << 32 over the path (anc, i]; a root carries (self, 0).  T (out): the segment pointer
__global__ __launch_bounds__(PTPB) void prune_down_init(const int *__restrict__ parent, const float *__restrict__ radius, const unsigned *__restrict__ q,
                                                        const unsigned *__restrict__ H, const u64 *__restrict__ best, int n, pnr::PruneRule rule, u64 *__restrict__ D,
                                                        int *__restrict__ T)
{
    const int i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= n) return;
    const int p = parent[i];
    if (p < 0) {
        D[i] = pack((unsigned)i, 0u);
        T[i] = i;
        return;
    }
    const bool head = (unsigned)best[p] != 0xffffffffu - (unsigned)i;
    const bool gone = head && rule.cut(q[i] + H[i], radius ? radius[p] : 0.f);
    D[i] = pack((unsigned)p, (head ? 2u : 0u) | (gone ? 1u : 0u));
    T[i] = head ? i : p;
}

__global__ __launch_bounds__(PTPB) void prune_down(const u64 *__restrict__ D, u64 *__restrict__ Dn, const int *__restrict__ T, int *__restrict__ Tn, int n, int round,
                                                   unsigned *__restrict__ flags)
{
    const int i = blockIdx.x * PTPB + threadIdx.x;
    if (i >= n) return;
    const u64 mine = D[i];
    const unsigned anc = (unsigned)mine, val = (unsigned)(mine >> 32);
    const u64 up = D[anc];
    const unsigned uval = (unsigned)(up >> 32);
    const int t = T[i], tt = T[t];
    if ((unsigned)up != anc || tt != t) flags[round] = 1;
    Dn[i] = pack((unsigned)up, ((val & ~1u) + (uval & ~1u)) | ((val | uval) & 1u)); // (order < n < 2^31)
    Tn[i] = tt;
}

enum { ST_ROOTS, ST_LEAVES, ST_BRANCH, ST_SEGMENTS, ST_REMOVED, ST_REMOVED_SEGMENTS, ST_REMOVED_TREES, ST_LENGTH_IN, ST_LENGTH_OUT, ST_H_MAX, ST_ORDER_MAX, N_ST };

// D, T final: anc = the root, T = the segment's head.  order_out receives the order, keep the answer of rule 5; st (zeroed): the sums
__global__ __launch_bounds__(PTPB) void prune_finish(const int *__restrict__ parent, const unsigned *__restrict__ q, const unsigned *__restrict__ kids,
                                                     const unsigned *__restrict__ H, const u64 *__restrict__ A, const u64 *__restrict__ D, const int *__restrict__ T, int n,
                                                     pnr::PruneRule rule, uint8_t *__restrict__ keep, unsigned *__restrict__ path, int *__restrict__ order, u64 *__restrict__ st)
{
    u64 w[N_ST] = {0};
    for (long long g = (long long)blockIdx.x * PTPB + threadIdx.x; g < n; g += (long long)gridDim.x * PTPB) {
        const int i = (int)g;
        const u64 d = D[i];
        const unsigned root = (unsigned)d, val = (unsigned)(d >> 32), h = H[i], k = kids[i], e = q[i];
        const bool gone = (val & 1u) || rule.cut_tree(H[root]), is_root = parent[i] < 0, head = T[i] == i;
        keep[i] = gone ? 0 : 1;
        path[i] = (unsigned)(A[i] >> 32);
        order[i] = (int)(val >> 1);
        w[ST_ROOTS] += is_root, w[ST_LEAVES] += k == 0, w[ST_BRANCH] += k >= 2, w[ST_SEGMENTS] += head;
        w[ST_REMOVED] += gone, w[ST_REMOVED_SEGMENTS] += head && gone, w[ST_REMOVED_TREES] += is_root && gone;
        w[ST_LENGTH_IN] += e, w[ST_LENGTH_OUT] += gone ? 0 : e;
        w[ST_H_MAX] = max(w[ST_H_MAX], (u64)h), w[ST_ORDER_MAX] = max(w[ST_ORDER_MAX], (u64)(val >> 1));
    }
#pragma unroll
    for (int k = 0; k < N_ST; k++) {
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const u64 other = (u64)__shfl_xor((long long)w[k], sh, 64);
            w[k] = k >= ST_H_MAX ? max(w[k], other) : w[k] + other;
        }
        if ((threadIdx.x & 63) == 0 && w[k]) {
            if (k >= ST_H_MAX) atomicMax(&st[k], w[k]);
            else atomicAdd(&st[k], w[k]);
        }
    }
}

} // namespace

int pnr_prune_run(pnr_ctx *c, const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts &o, pnr_prune_info *info,
                  uint8_t *keep, uint32_t *height, uint32_t *path, int32_t *order, int32_t *seg)
{
    const pnr::PruneRule rule(o);
    const size_t k = (size_t)n;
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_xyz = buf.add<float>(3 * k), d_rad = buf.add<float>(radius ? k : 0);
    const auto d_par = buf.add<int>(k), d_T = buf.add<int>(2 * k), d_order = buf.add<int>(k);
    const auto d_q = buf.add<unsigned>(k), d_kids = buf.add<unsigned>(k), d_H = buf.add<unsigned>(2 * k), d_path = buf.add<unsigned>(k), d_flags = buf.add<unsigned>(N_FLAGS);
    const auto d_A = buf.add<u64>(2 * k), d_D = buf.add<u64>(2 * k), d_best = buf.add<u64>(k), d_st = buf.add<u64>(N_ST);
    const auto d_keep = buf.add<uint8_t>(k);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::PinBuf<unsigned> h_flags;
    if (h_flags.alloc(2) != hipSuccess) {
        (void)hipGetLastError();
        pnr::set_error("%s: pinned allocation of 8 B failed", who);
        return PNR_E_NOMEM;
    }
    pnr::Call call(c, who);
    const dim3 grid((unsigned)((n + PTPB - 1) / PTPB)), block(PTPB);
    const float *const rad = radius ? d_rad.get() : nullptr;
    call.up(d_xyz, xyz);
    if (radius) call.up(d_rad, radius);
    call.up(d_par, parent);
    call.fill(d_kids, 0), call.fill(d_H, 0), call.fill(d_flags, 0), call.fill(d_best, 0), call.fill(d_st, 0);
    call.timed("prune", prune_edges, grid, block, d_xyz.get(), d_par.get(), (int)n, rule, d_q.get(), d_kids.get(), d_A.get(), d_flags.get());
    // one loop for both directions: launch round r on buffer `cur`, read its flag and the range flag back, stop after a quiet round
    int cur = 0, rounds_up = 0, rounds_down = 0;
    auto jump = [&](int &rounds, auto &&launch) -> int {
        for (rounds = 0;; cur ^= 1) {
            PNR_REQUIRE(rounds < MAX_ROUNDS, PNR_E_HIP, "%s: the pointer jumping did not settle in %d rounds", who, MAX_ROUNDS);
            launch(rounds);
            call.down(h_flags.get(), d_flags.get() + rounds, 1);
            call.down(h_flags.get() + 1, d_flags.get() + FLAG_RANGE, 1);
            if (const int e = call.finish()) return e;
            rounds++;
            PNR_REQUIRE(!h_flags.get()[1], PNR_E_ARG, PNR_PRUNE_RANGE_TEXT, who);
            if (!h_flags.get()[0]) return PNR_OK;
        }
    };
    unsigned *H[2] = {d_H.get(), d_H.get() + k};
    u64 *A[2] = {d_A.get(), d_A.get() + k}, *D[2] = {d_D.get(), d_D.get() + k};
    int *T[2] = {d_T.get(), d_T.get() + k};
    rc = jump(rounds_up, [&](int r) {
        if (call.ok()) call.note(hipMemcpyAsync(H[cur ^ 1], H[cur], k * sizeof(unsigned), hipMemcpyDeviceToDevice, call.stream()));
        call.timed("prune", prune_up, grid, block, (const u64 *)A[cur], A[cur ^ 1], (const unsigned *)H[cur], H[cur ^ 1], (int)n, r, d_flags.get());
    });
    if (rc) return rc;
    const unsigned *const Hf = H[cur ^ 1]; // (the last round wrote the other buffer)
    const u64 *const Af = A[cur ^ 1];
    call.fill(d_flags, 0);
    c->tic();
    call.launch(prune_child, grid, block, d_par.get(), d_q.get(), Hf, (int)n, d_best.get());
    call.launch(prune_down_init, grid, block, d_par.get(), rad, d_q.get(), Hf, (const u64 *)d_best.get(), (int)n, rule, D[0], T[0]);
    c->toc("prune", 2);
    cur = 0;
    rc = jump(rounds_down, [&](int r) {
        call.timed("prune", prune_down, grid, block, (const u64 *)D[cur], D[cur ^ 1], (const int *)T[cur], T[cur ^ 1], (int)n, r, d_flags.get());
    });
    if (rc) return rc;
    u64 st[N_ST];
    call.timed("prune", prune_finish, dim3(pnr::grid_blocks((n + PTPB - 1) / PTPB)), block, d_par.get(), d_q.get(), d_kids.get(), Hf, Af, (const u64 *)D[cur ^ 1],
               (const int *)T[cur ^ 1], (int)n, rule, d_keep.get(), d_path.get(), d_order.get(), d_st.get());
    call.down(st, d_st);
    if (keep) call.down(keep, d_keep);
    if (height) call.down(height, Hf, k);
    if (path) call.down(path, d_path);
    if (order) call.down(order, d_order);
    if (seg) call.down(seg, (const int *)T[cur ^ 1], k);
    if ((rc = call.finish())) return rc;
    if (info)
        *info = pnr_prune_info{n, (int64_t)st[ST_ROOTS], (int64_t)st[ST_LEAVES], (int64_t)st[ST_BRANCH], (int64_t)st[ST_SEGMENTS], (int64_t)st[ST_REMOVED],
                               (int64_t)st[ST_REMOVED_SEGMENTS], (int64_t)st[ST_REMOVED_TREES], st[ST_LENGTH_IN], st[ST_LENGTH_OUT], (uint32_t)st[ST_H_MAX],
                               (int32_t)st[ST_ORDER_MAX], rounds_up, rounds_down};
    return PNR_OK;
}
