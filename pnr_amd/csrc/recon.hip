// recon.hip -- the neighbour stages of reconstruct() on the device (pnr_reconstruct_ctx): the non-blurring mean-shift
// (reconstruct.cpp mean_shift, reference :968-1052) and the ball lists of the sphere grouping (group_spheres, :1566-1642).
// Both give the host stage's bits: the same IEEE operations in the same order (-ffp-contract=off, correctly rounded f32
// division and square root), members taken in ascending node index.
//
// Grid: the nodes >= 1 are binned into a dense uniform grid over the box of their finite coordinates; a bin outside the box is
// clamped to its edge, nodes and queries alike.  Clamping and binning are monotone in the coordinate, so a query that visits the
// cells of [q - R, q + R] sees every node within R of q, and no query visits more than every cell once, whatever the radius.
// Cells are numbered with z fastest: the cells of one (x, y) row of a query are one contiguous run of the packed node array.
//
// Queries: one wave per node.  Members are ballot-compacted into an LDS list, sorted (bitonic) and used in ascending index.  A
// ball with more than CAP members is left to a second kernel, where a work-group marks the members in a bitmap over the node
// indices and walks it in ascending order: same members, same order, no bound on the ball.
#include "recon.h"
#include "call.h"
#include <climits>
#include <cmath>

namespace {

constexpr int CAP = 512;          // members of a wave's LDS list
constexpr int BIG = 256;          // threads of a work-group of the bitmap kernels
constexpr int WALK = 64;          // bitmap words turned into indices at a time (<= WALK * 32 members in LDS)
constexpr size_t BITMAP_BUDGET = size_t(256) << 20; // bytes of bitmaps of all work-groups of a bitmap kernel together
constexpr unsigned NEG_NAN = 0xFFC00000u; // 0.f / 0 on the host's SSE divide (an empty ball): the default NaN, sign set

struct Geom {
    float ox, oy, oz, cell;
    int nx, ny, nz;
};

__device__ __forceinline__ int bin1(float v, float o, float cell, int dim)
{
    float f = floorf((v - o) / cell);
    if (!(f >= 0.f)) f = 0.f; // (NaN as well)
    if (f > (float)(dim - 1)) f = (float)(dim - 1);
    return (int)f;
}

__device__ __forceinline__ bool any_nan(float a, float b, float c, float d) { return a != a || b != b || c != c || d != d; }

// every (x, y) row of cells of the cube [q - R, q + R]: calls row(p0, p1), the positions of its nodes in the packed array
template <class F>
__device__ __forceinline__ void for_rows(const Geom &g, const int *start, float x, float y, float z, float R, F &&row)
{
    const int a0 = bin1(x - R, g.ox, g.cell, g.nx), a1 = bin1(x + R, g.ox, g.cell, g.nx);
    const int b0 = bin1(y - R, g.oy, g.cell, g.ny), b1 = bin1(y + R, g.oy, g.cell, g.ny);
    const int c0 = bin1(z - R, g.oz, g.cell, g.nz), c1 = bin1(z + R, g.oz, g.cell, g.nz);
    for (int a = a0; a <= a1; a++)
        for (int b = b0; b <= b1; b++) {
            const int r = (a * g.ny + b) * g.nz;
            row(start[r + c0], start[r + c1 + 1]);
        }
}

// ---- grid build: bin, count, scan, scatter ----
__global__ void k_bin(const float4 *pos, int n, Geom g, int *cell, int *count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (i >= n) return;
    const float4 p = pos[i];
    const int c = (bin1(p.x, g.ox, g.cell, g.nx) * g.ny + bin1(p.y, g.oy, g.cell, g.ny)) * g.nz + bin1(p.z, g.oz, g.cell, g.nz);
    cell[i] = c;
    atomicAdd(&count[c], 1);
}

// one work-group: start[k] = sum of count[0 .. k), k <= ncell; cursor[k] = start[k]
__global__ __launch_bounds__(1024) void k_scan(const int *count, int ncell, int *start, int *cursor)
{
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;
    for (int base = 0; base < ncell; base += 1024) {
        const int i = base + t;
        const int v = i < ncell ? count[i] : 0;
        int x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < 16; k++) {
            const int s = wsum[k];
            before += k < w ? s : 0;
            total += s;
        }
        if (i < ncell) start[i] = cursor[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (t == 0) start[ncell] = carry;
}

// packed array: (x, y, z, node index as bits), cell by cell (the order inside a cell is free: members are sorted by index)
__global__ void k_scatter(const float4 *pos, int n, const int *cell, int *cursor, float4 *gp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (i >= n) return;
    const int slot = atomicAdd(&cursor[cell[i]], 1);
    const float4 p = pos[i];
    gp[slot] = make_float4(p.x, p.y, p.z, __int_as_float(i));
}

// ---- membership tests of the host stages ----
// mean-shift: f32 squares of f32 differences, f32 sums, tested one term at a time
__device__ __forceinline__ bool shift_member(float4 q, float x, float y, float z, float r2)
{
    const float dx = q.x - x, x2 = dx * dx;
    if (!(x2 <= r2)) return false;
    const float dy = q.y - y, y2 = dy * dy;
    if (!(x2 + y2 <= r2)) return false;
    const float dz = q.z - z, z2 = dz * dz;
    return x2 + y2 + z2 <= r2;
}

// grouping: each square and each running sum in f64, rounded to f32 after every term
__device__ __forceinline__ bool ball_member(float4 q, float x, float y, float z, float r2)
{
    const float dx = q.x - x;
    float d2 = (float)((double)dx * (double)dx);
    if (!(d2 <= r2)) return false;
    const float dy = q.y - y;
    d2 = (float)((double)d2 + (double)dy * (double)dy);
    if (!(d2 <= r2)) return false;
    const float dz = q.z - z;
    d2 = (float)((double)d2 + (double)dz * (double)dz);
    return d2 <= r2;
}

// ---- wave kernels: one 64-lane work-group per node ----
// every member of the ball into list[] (first CAP of them), returns how many there are (uniform)
template <class Test>
__device__ __forceinline__ int wave_collect(const Geom &g, const int *start, const float4 *gp, float x, float y, float z, float R,
                                            int *list, Test &&test)
{
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1;
    int cnt = 0;
    for_rows(g, start, x, y, z, R, [&](int p0, int p1) {
        for (int base = p0; base < p1; base += 64) {
            const int p = base + lane;
            int j = 0;
            bool m = false;
            if (p < p1) {
                const float4 q = gp[p];
                j = __float_as_int(q.w);
                m = test(q, j);
            }
            const unsigned long long mask = __ballot(m);
            if (m) {
                const int at = cnt + __popcll(mask & below);
                if (at < CAP) list[at] = j;
            }
            cnt += __popcll(mask);
        }
    });
    return cnt;
}

// list[0 .. cnt) ascending (cnt <= CAP)
__device__ void wave_sort(int *list, int cnt)
{
    const int lane = threadIdx.x;
    int m = 1;
    while (m < cnt) m <<= 1;
    for (int k = cnt + lane; k < m; k += 64) list[k] = INT_MAX;
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < m / 2; t += 64) {
                const int lo = 2 * stride * (t / stride) + t % stride, hi = lo + stride;
                const bool up = (lo & size) == 0;
                const int a = list[lo], b = list[hi];
                if ((a > b) == up) { list[lo] = b; list[hi] = a; }
            }
            __syncthreads();
        }
}

// lane q < 4: acc + component q of src[list[0]], src[list[1]], ... one f32 add at a time
__device__ __forceinline__ float chain_sum(const float4 *src, const int *list, int cnt, float acc)
{
    const int q = threadIdx.x & 3;
    const float *sf = (const float *)src;
    int k = 0;
    for (; k + 8 <= cnt; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = sf[4 * (size_t)list[k + u] + q];
#pragma unroll
        for (int u = 0; u < 8; u++) acc += v[u];
    }
    for (; k < cnt; k++) acc += sf[4 * (size_t)list[k] + q];
    return acc;
}

// the end of a mean-shift iteration (uniform): the mean of the members, its squared move (f64 terms), the next position
__device__ __forceinline__ float shift_step(float s[4], int cnt, float c[4])
{
    if (cnt == 0) {
        s[0] = s[1] = s[2] = s[3] = __uint_as_float(NEG_NAN);
    } else {
        const float fc = (float)cnt;
        for (int k = 0; k < 4; k++) s[k] /= fc;
    }
    const double ex = (double)(s[0] - c[0]), ey = (double)(s[1] - c[1]), ez = (double)(s[2] - c[2]);
    const float d2 = (float)(ex * ex + ey * ey + ez * ez);
    for (int k = 0; k < 4; k++) c[k] = s[k];
    return d2;
}

__global__ __launch_bounds__(64) void k_shift(const float4 *src, int n, Geom g, const int *start, const float4 *gp, float s2r, int maxiter,
                                              float eps2, float4 *res, int *ovf, int *n_ovf)
{
    __shared__ int list[CAP];
    const int i = blockIdx.x + 1, lane = threadIdx.x;
    const float4 s0 = src[i];
    float c[4] = {s0.x, s0.y, s0.z, s0.w};
    int iter = 0;
    float d2;
    do {
        const float rad = s2r * c[3], r2 = rad * rad;
        int cnt = 0;
        if (!any_nan(c[0], c[1], c[2], r2)) // (no member otherwise)
            cnt = wave_collect(g, start, gp, c[0], c[1], c[2], sqrtf(r2) * 1.0001f + 1e-3f, list,
                               [&](float4 q, int) { return shift_member(q, c[0], c[1], c[2], r2); });
        if (cnt > CAP) { // the bitmap kernel takes this node, from the start
            if (lane == 0) ovf[atomicAdd(n_ovf, 1)] = i;
            return;
        }
        wave_sort(list, cnt);
        const float acc = lane < 4 ? chain_sum(src, list, cnt, 0.f) : 0.f;
        float s[4] = {__shfl(acc, 0, 64), __shfl(acc, 1, 64), __shfl(acc, 2, 64), __shfl(acc, 3, 64)};
        __syncthreads(); // list[] is refilled
        d2 = shift_step(s, cnt, c);
        iter++;
    } while (iter < maxiter && d2 > eps2);
    if (lane == 0) res[i] = make_float4(c[0], c[1], c[2], c[3]);
}

__global__ __launch_bounds__(64) void k_balls(const float4 *pos, int n, Geom g, const int *start, const float4 *gp, float rad, long long *off,
                                              int *cnt_out, int *list_out, long long cap, unsigned long long *cursor, int *ovf, int *n_ovf)
{
    __shared__ int list[CAP];
    const int ci = blockIdx.x + 1, lane = threadIdx.x;
    const float4 p = pos[ci];
    const float r2 = rad * rad;
    int cnt = 0;
    if (!any_nan(p.x, p.y, p.z, r2))
        cnt = wave_collect(g, start, gp, p.x, p.y, p.z, rad * 1.0001f + 1e-3f, list,
                           [&](float4 q, int j) { return j != ci && ball_member(q, p.x, p.y, p.z, r2); });
    if (cnt > CAP) {
        if (lane == 0) ovf[atomicAdd(n_ovf, 1)] = ci;
        return;
    }
    wave_sort(list, cnt);
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor, (unsigned long long)cnt);
    base = __shfl(base, 0, 64);
    if (lane == 0) { off[ci] = (long long)base; cnt_out[ci] = cnt; }
    if ((long long)base + cnt <= cap) // else the host sizes the list up and runs again
        for (int k = lane; k < cnt; k += 64) list_out[base + k] = list[k];
}

// ---- bitmap kernels: one work-group per ball larger than CAP ----
// mark the members (bits of the work-group's bitmap, all clear on entry); returns how many there are (uniform)
template <class Test>
__device__ int big_mark(const Geom &g, const int *start, const float4 *gp, float x, float y, float z, float R, unsigned *bm, int *tot,
                        Test &&test)
{
    if (threadIdx.x == 0) *tot = 0;
    __syncthreads();
    int mine = 0;
    for_rows(g, start, x, y, z, R, [&](int p0, int p1) {
        for (int p = p0 + (int)threadIdx.x; p < p1; p += BIG) {
            const float4 q = gp[p];
            const int j = __float_as_int(q.w);
            if (test(q, j)) {
                atomicOr(&bm[j >> 5], 1u << (j & 31));
                mine++;
            }
        }
    });
    if (mine) atomicAdd(tot, mine);
    __syncthreads();
    const int cnt = *tot;
    __syncthreads();
    return cnt;
}

// the marked indices in ascending order, WALK * 32 at most at a time: chunk(list, k) with the k of them in list[] (uniform
// calls); the bitmap is left clear
template <class F>
__device__ void big_walk(unsigned *bm, int nw, int *list, int *woff, F &&chunk)
{
    const int t = threadIdx.x;
    for (int w0 = 0; w0 < nw; w0 += WALK) {
        unsigned word = 0;
        if (t < WALK && w0 + t < nw) word = atomicExch(&bm[w0 + t], 0u); // (the marks are L2 atomics: read and cleared there too)
        if (t < 64) { // wave 0: exclusive scan of the words' bit counts
            const int pc = __popc(word);
            int x = pc;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d, 64);
                if (t >= d) x += y;
            }
            woff[t] = x - pc;
            if (t == 63) woff[64] = x;
        }
        __syncthreads();
        const int k = woff[64];
        if (word) {
            int at = woff[t];
            while (word) {
                const int b = __ffs(word) - 1;
                word &= word - 1;
                list[at++] = ((w0 + t) << 5) + b;
            }
        }
        __syncthreads();
        if (k) chunk(list, k);
        __syncthreads();
    }
}

__global__ __launch_bounds__(BIG) void k_shift_big(const float4 *src, Geom g, const int *start, const float4 *gp, float s2r, int maxiter,
                                                   float eps2, float4 *res, const int *ovf, const int *n_ovf, unsigned *bitmaps, int nw)
{
    __shared__ int list[WALK * 32];
    __shared__ int woff[65];
    __shared__ int tot;
    __shared__ float part[4];
    unsigned *bm = bitmaps + (size_t)blockIdx.x * nw;
    const int t = threadIdx.x;
    for (int o = blockIdx.x; o < *n_ovf; o += gridDim.x) {
        const int i = ovf[o];
        const float4 s0 = src[i];
        float c[4] = {s0.x, s0.y, s0.z, s0.w};
        int iter = 0;
        float d2;
        do {
            const float rad = s2r * c[3], r2 = rad * rad;
            int cnt = 0;
            if (!any_nan(c[0], c[1], c[2], r2))
                cnt = big_mark(g, start, gp, c[0], c[1], c[2], sqrtf(r2) * 1.0001f + 1e-3f, bm, &tot,
                               [&](float4 q, int) { return shift_member(q, c[0], c[1], c[2], r2); });
            float acc = 0.f;
            if (cnt)
                big_walk(bm, nw, list, woff, [&](const int *l, int k) {
                    if (t < 4) acc = chain_sum(src, l, k, acc);
                });
            if (t < 4) part[t] = acc;
            __syncthreads();
            float s[4] = {part[0], part[1], part[2], part[3]};
            __syncthreads();
            d2 = shift_step(s, cnt, c);
            iter++;
        } while (iter < maxiter && d2 > eps2);
        if (t == 0) res[i] = make_float4(c[0], c[1], c[2], c[3]);
    }
}

__global__ __launch_bounds__(BIG) void k_balls_big(const float4 *pos, Geom g, const int *start, const float4 *gp, float rad, long long *off,
                                                   int *cnt_out, int *list_out, long long cap, unsigned long long *cursor, const int *ovf,
                                                   const int *n_ovf, unsigned *bitmaps, int nw)
{
    __shared__ int list[WALK * 32];
    __shared__ int woff[65];
    __shared__ int tot;
    __shared__ unsigned long long base_s;
    unsigned *bm = bitmaps + (size_t)blockIdx.x * nw;
    const int t = threadIdx.x;
    const float r2 = rad * rad;
    for (int o = blockIdx.x; o < *n_ovf; o += gridDim.x) {
        const int ci = ovf[o];
        const float4 p = pos[ci];
        // (a ball of a NaN centre is empty and never comes here)
        const int cnt = big_mark(g, start, gp, p.x, p.y, p.z, rad * 1.0001f + 1e-3f, bm, &tot,
                                 [&](float4 q, int j) { return j != ci && ball_member(q, p.x, p.y, p.z, r2); });
        if (t == 0) {
            base_s = atomicAdd(cursor, (unsigned long long)cnt);
            off[ci] = (long long)base_s;
            cnt_out[ci] = cnt;
        }
        __syncthreads();
        const long long base = (long long)base_s;
        const bool fits = base + cnt <= cap;
        long long at = base;
        big_walk(bm, nw, list, woff, [&](const int *l, int k) {
            if (fits)
                for (int e = t; e < k; e += BIG) list_out[at + e] = l[e];
            at += k;
        });
        __syncthreads();
    }
}

// ---- host side ----
using advantra::P4;
static_assert(sizeof(P4) == sizeof(float4), "P4 is uploaded as float4");
const char *const who = "reconstruct";

// the grid of a call: its geometry (host) and its arrays, parts of the call's buffer
struct DevGrid {
    Geom g;
    int ncell = 0;
    pnr::Part<int> cell, count, cursor; // [n] [ncell] [ncell]
    pnr::Part<int> start;               // [ncell + 1]
    pnr::Part<float4> gp;               // [n - 1]
};

// the grid over nodes 1 .. n-1 of pos, cells of at least `cell` (larger where the box would need more than max(4096, 4n) of them): the
// geometry, and the arrays as parts of buf
void plan_grid(pnr::CallBuf &buf, const std::vector<P4> &pos, float cell, DevGrid &G)
{
    const int n = (int)pos.size();
    double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int i = 1; i < n; i++) {
        const float v[3] = {pos[i].x, pos[i].y, pos[i].z};
        for (int k = 0; k < 3; k++)
            if (std::isfinite(v[k])) { mn[k] = std::min(mn[k], (double)v[k]); mx[k] = std::max(mx[k], (double)v[k]); }
    }
    for (int k = 0; k < 3; k++)
        if (mn[k] > mx[k]) mn[k] = mx[k] = 0;
    double dim[3] = {1, 1, 1}, cs = cell;
    if (std::isfinite(cs) && cs > 0) {
        const double cap = std::max(4096.0, 4.0 * n);
        for (;;) {
            for (int k = 0; k < 3; k++) dim[k] = std::floor((mx[k] - mn[k]) / cs) + 1;
            if (dim[0] * dim[1] * dim[2] <= cap) break;
            cs *= 1.25;
        }
    } else cs = 1; // one cell: every query visits it
    Geom &g = G.g;
    g = Geom{(float)mn[0], (float)mn[1], (float)mn[2], (float)cs, (int)dim[0], (int)dim[1], (int)dim[2]};
    G.ncell = g.nx * g.ny * g.nz;
    G.cell = buf.add<int>((size_t)n);
    G.count = buf.add<int>((size_t)G.ncell);
    G.cursor = buf.add<int>((size_t)G.ncell);
    G.start = buf.add<int>((size_t)G.ncell + 1);
    G.gp = buf.add<float4>((size_t)n - 1);
}

// fills the grid from the n positions d_pos (the ones plan_grid saw): three launches
void build_grid(pnr::Call &call, const float4 *d_pos, int n, const DevGrid &G)
{
    call.fill(G.count, 0);
    const unsigned nb = (unsigned)((n - 1 + 255) / 256);
    call.launch(k_bin, dim3(nb), dim3(256), d_pos, n, G.g, G.cell.get(), G.count.get());
    call.launch(k_scan, dim3(1), dim3(1024), (const int *)G.count, G.ncell, G.start.get(), G.cursor.get());
    call.launch(k_scatter, dim3(nb), dim3(256), d_pos, n, (const int *)G.cell, G.cursor.get(), G.gp.get());
}

// work-groups of a bitmap kernel for `balls` large balls over n nodes, and its bitmap words per work-group
void bitmap_shape(int balls, int n, int &groups, int &nw)
{
    nw = (n + 31) / 32;
    const size_t fit = std::max<size_t>(1, BITMAP_BUDGET / ((size_t)nw * 4));
    groups = (int)std::min<size_t>({(size_t)balls, fit, (size_t)1024});
}

} // namespace

int pnr_recon_shift(pnr_ctx *c, const std::vector<P4> &src, float s2r, int maxiter, float eps2, std::vector<P4> &res)
{
    res = src;
    const int64_t n64 = (int64_t)src.size();
    if (n64 < 2) return PNR_OK;
    PNR_REQUIRE(n64 < (1 << 28), PNR_E_ARG, "reconstruct: %lld nodes, at most 2^28 on the device", (long long)n64);
    const int n = (int)n64;
    PNR_HIP(hipSetDevice(c->device));
    // cells of about the mean ball radius (the candidate boxes stay a few cells wide)
    double ssum = 0;
    int64_t sn = 0;
    for (int i = 1; i < n; i++)
        if (std::isfinite(src[i].s) && src[i].s > 0) { ssum += src[i].s; sn++; }
    const float cell = std::max(1.0f, s2r * (float)(sn ? ssum / (double)sn : 1.0));
    // device buffers of the call: input | result | the large balls and their number | the grid
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_src = buf.add<float4>((size_t)n), d_res = buf.add<float4>((size_t)n);
    const auto d_ovf = buf.add<int>((size_t)n), d_novf = buf.add<int>(1);
    DevGrid G;
    plan_grid(buf, src, cell, G);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::Call call(c, who);
    call.up(d_src, src.data());
    call.fill(d_novf, 0);
    c->tic();
    build_grid(call, d_src, n, G);
    call.launch(k_shift, dim3(n - 1), dim3(64), (const float4 *)d_src, n, G.g, (const int *)G.start, (const float4 *)G.gp, s2r, maxiter, eps2,
                d_res.get(), d_ovf.get(), d_novf.get());
    c->toc("recon", 4);
    int novf = 0;
    call.down(&novf, d_novf);
    if ((rc = call.finish())) return rc;
    pnr::CallBuf bm; // the bitmaps, sized by the read-back
    if (novf > 0) {
        int groups = 0, nw = 0;
        bitmap_shape(novf, n, groups, nw);
        const auto d_bm = bm.add<unsigned>((size_t)groups * nw);
        if ((rc = bm.alloc(who))) return rc;
        call.fill(d_bm, 0);
        call.timed("recon", k_shift_big, dim3(groups), dim3(BIG), (const float4 *)d_src, G.g, (const int *)G.start, (const float4 *)G.gp, s2r, maxiter, eps2,
                   d_res.get(), (const int *)d_ovf, (const int *)d_novf, d_bm.get(), nw);
    }
    call.down(res.data() + 1, d_res.get() + 1, (size_t)n - 1);
    return call.finish();
}

int pnr_recon_balls(pnr_ctx *c, const std::vector<P4> &pos, float rad, advantra::BallLists &out)
{
    const int64_t n64 = (int64_t)pos.size();
    out.off.assign((size_t)n64, 0);
    out.cnt.assign((size_t)n64, 0);
    out.list.clear();
    if (n64 < 2) return PNR_OK;
    PNR_REQUIRE(n64 < (1 << 28), PNR_E_ARG, "reconstruct: %lld nodes, at most 2^28 on the device", (long long)n64);
    const int n = (int)n64;
    PNR_HIP(hipSetDevice(c->device));
    // device buffers of the call: positions | offset and size of every ball | the large balls and their number | the list cursor | the grid
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_pos = buf.add<float4>((size_t)n);
    const auto d_off = buf.add<long long>((size_t)n);
    const auto d_cnt = buf.add<int>((size_t)n), d_ovf = buf.add<int>((size_t)n), d_novf = buf.add<int>(1);
    const auto d_cursor = buf.add<unsigned long long>(1);
    DevGrid G;
    plan_grid(buf, pos, std::max(2.0f, rad), G);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::Call call(c, who);
    call.up(d_pos, pos.data());
    c->tic();
    build_grid(call, d_pos, n, G);
    c->toc("recon", 3);
    long long cap = std::max<long long>(1 << 20, 16LL * n);
    for (int pass = 0;; pass++) {
        pnr::CallBuf lists, bm; // of this pass: a list that was too small and the bitmaps are gone before the next one
        const auto d_list = lists.add<int>((size_t)cap);
        if ((rc = lists.alloc(who))) return rc;
        call.fill(d_novf, 0);
        call.fill(d_cursor, 0);
        call.timed("recon", k_balls, dim3(n - 1), dim3(64), (const float4 *)d_pos, n, G.g, (const int *)G.start, (const float4 *)G.gp, rad, d_off.get(),
                   d_cnt.get(), d_list.get(), cap, d_cursor.get(), d_ovf.get(), d_novf.get());
        int novf = 0;
        call.down(&novf, d_novf);
        if ((rc = call.finish())) return rc;
        if (novf > 0) {
            int groups = 0, nw = 0;
            bitmap_shape(novf, n, groups, nw);
            const auto d_bm = bm.add<unsigned>((size_t)groups * nw);
            if ((rc = bm.alloc(who))) return rc;
            call.fill(d_bm, 0);
            call.timed("recon", k_balls_big, dim3(groups), dim3(BIG), (const float4 *)d_pos, G.g, (const int *)G.start, (const float4 *)G.gp, rad, d_off.get(),
                       d_cnt.get(), d_list.get(), cap, d_cursor.get(), (const int *)d_ovf, (const int *)d_novf, d_bm.get(), nw);
        }
        unsigned long long used = 0;
        call.down(&used, d_cursor);
        if ((rc = call.finish())) return rc;
        if ((long long)used <= cap) {
            out.list.resize((size_t)used);
            call.down(out.off.data() + 1, d_off.get() + 1, (size_t)n - 1);
            call.down(out.cnt.data() + 1, d_cnt.get() + 1, (size_t)n - 1);
            if (used) call.down(out.list.data(), d_list.get(), (size_t)used);
            return call.finish();
        }
        PNR_REQUIRE(pass == 0, PNR_E_STATE, "reconstruct: ball lists need %llu entries after resizing to %lld", used, cap);
        cap = (long long)used; // too small: sized to what this pass needed, and run again
    }
}
