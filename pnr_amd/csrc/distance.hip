// distance.hip -- all-pairs point-to-segment minimum behind pnr_point_segment_distance / pnr_tree_distance.  The rule
// (include/pnr_hip.h): per segment ab = b - a, den = (ab.x^2 + ab.y^2) + ab.z^2, r = den > 0 ? 1 / den : 0; per pair
// t = min(max(((p - a) . ab) * r, 0), 1), e = p - (a + t ab), d2 = e . e; per point d = sqrt(min_j d2), j* = the smallest j at the minimum.
// Every operation is one IEEE f32 operation in the order of the header (the build has -ffp-contract=off).
//
// dist_prep turns the segments into two float4 each: (a, r) and (ab, 0).  dist_min has one thread per point with the point in
// registers; the segment index of its loop is the same in every lane, so a segment arrives through scalar loads (two dwordx4 per
// segment and wave, none per lane) and the vector unit only does the ~25 operations of the pair.  blockIdx.y cuts the segments into
// slices, so that a few thousand points still fill the chip; every thread ends with ONE 64-bit atomicMin on
// (bits(d2) << 32) | j -- d2 >= +0, so its bit pattern orders like its value, and the low word makes the smallest j win a tie.
// The result therefore does not depend on the slices or on how the (points x segments) rectangle is cut into launches: a launch
// is bounded by a pair budget, so that no single kernel occupies the GPU for seconds.  dist_finish unpacks and takes the root.
#include "distance.h"
#include <cmath>

namespace pnr {

int tree_sample(const float *xyz, const int32_t *parent, int64_t n, float zscale, float step, float *pts_out, int32_t *owner_out, int64_t cap,
                int64_t *n_out)
{
    int64_t k = 0;
    auto put = [&](float x, float y, float z, int64_t node) {
        if (k < cap) {
            if (pts_out) pts_out[3 * k] = x, pts_out[3 * k + 1] = y, pts_out[3 * k + 2] = z;
            if (owner_out) owner_out[k] = (int32_t)node;
        }
        k++;
    };
    for (int64_t i = 0; i < n; i++) {
        const float *p = xyz + 3 * i;
        PNR_REQUIRE(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]), PNR_E_ARG, "tree: node %lld has a coordinate that is not finite", (long long)i);
        PNR_REQUIRE(parent[i] < n, PNR_E_ARG, "tree: parent[%lld] = %d outside [-1, %lld)", (long long)i, parent[i], (long long)n);
        const float az = p[2] * zscale;
        PNR_REQUIRE(std::isfinite(az), PNR_E_ARG, "tree: z * zscale of node %lld is not finite", (long long)i);
        put(p[0], p[1], az, i);
        if (parent[i] < 0 || !(step > 0.f)) continue;
        const float *b = xyz + 3 * (int64_t)parent[i];
        const double ax = p[0], ay = p[1], azd = az;
        const double dx = (double)b[0] - ax, dy = (double)b[1] - ay, dz = (double)(b[2] * zscale) - azd;
        const double L = std::sqrt((dx * dx + dy * dy) + dz * dz);
        const double qd = std::ceil(L / (double)step);
        PNR_REQUIRE(qd <= 2147483648.0, PNR_E_ARG, "tree: the segment of node %lld has %g steps (coordinates not finite, or more than 2^31)", (long long)i, qd);
        const int64_t q = (int64_t)qd;
        for (int64_t s = 1; s < q; s++) {
            const double f = (double)s / (double)q;
            put((float)(ax + dx * f), (float)(ay + dy * f), (float)(azd + dz * f), i);
        }
    }
    *n_out = k;
    return PNR_OK;
}

} // namespace pnr

namespace {

constexpr int DTPB = 256;              // threads of a work-group = points of a block row
constexpr int MIN_SPLIT = 64;          // automatic slices hold at least this many segments: one atomic per 64 pairs at the most
constexpr int TARGET_BLOCKS = 2048;    // automatic slices: work-groups of a launch that fill 256 CUs eight deep
constexpr long long AUTO_PAIRS = 1ll << 34; // pairs per launch: some 10 ms

__global__ __launch_bounds__(DTPB) void dist_prep(const float *__restrict__ a, const float *__restrict__ b, int m, float4 *__restrict__ seg)
{
    const int j = blockIdx.x * DTPB + threadIdx.x;
    if (j >= m) return;
    const float ax = a[3 * j], ay = a[3 * j + 1], az = a[3 * j + 2];
    const float abx = b[3 * j] - ax, aby = b[3 * j + 1] - ay, abz = b[3 * j + 2] - az;
    const float den = (abx * abx + aby * aby) + abz * abz;
    const float r = den > 0.f ? 1.0f / den : 0.f;
    seg[2 * j] = make_float4(ax, ay, az, r);
    seg[2 * j + 1] = make_float4(abx, aby, abz, 0.f);
}

// points [p0, p1) x segments [s0, s1); blockIdx.y = the slice of `split` segments
__global__ __launch_bounds__(DTPB) void dist_min(const float *__restrict__ pts, int p0, int p1, const float4 *__restrict__ seg, int s0, int s1, int split,
                                                 unsigned long long *__restrict__ key)
{
    const int i = p0 + blockIdx.x * DTPB + threadIdx.x;
    const int j0 = s0 + blockIdx.y * split, j1 = min(j0 + split, s1);
    const int ip = min(i, p1 - 1); // (the lanes past the last point run along on it and write nothing)
    const float px = pts[3 * ip], py = pts[3 * ip + 1], pz = pts[3 * ip + 2];
    float best = INFINITY;
    int bj = j0;
#pragma unroll 4
    for (int j = j0; j < j1; j++) { // j is wave-uniform: scalar loads
        const float4 A = seg[2 * j], B = seg[2 * j + 1];
        const float apx = px - A.x, apy = py - A.y, apz = pz - A.z;
        const float num = (apx * B.x + apy * B.y) + apz * B.z;
        const float t = fminf(fmaxf(num * A.w, 0.f), 1.f);
        const float ex = px - (A.x + t * B.x), ey = py - (A.y + t * B.y), ez = pz - (A.z + t * B.z);
        const float d2 = (ex * ex + ey * ey) + ez * ez;
        if (d2 < best) best = d2, bj = j; // (ascending j: the first of equals stays)
    }
    if (i < p1) atomicMin(&key[i], (unsigned long long)__float_as_uint(best) << 32 | (unsigned)bj);
}

__global__ __launch_bounds__(DTPB) void dist_finish(const unsigned long long *__restrict__ key, int n, float *__restrict__ d, int *__restrict__ j)
{
    const int i = blockIdx.x * DTPB + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    d[i] = sqrtf(__uint_as_float((unsigned)(k >> 32)));
    j[i] = (int)(unsigned)k;
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

} // namespace

int pnr_distance_run(pnr_ctx *c, const float *pts, int64_t n, const float *seg_a, const float *seg_b, int64_t m, float *d_out, int32_t *j_out)
{
    hipStream_t st = c->stream;
    // device buffers of the call: the prepared segments | the packed minima | the points | a | b | d | j
    const size_t o_key = pad16((size_t)m * 32), o_pts = o_key + pad16((size_t)n * 8), o_a = o_pts + pad16((size_t)n * 12), o_b = o_a + pad16((size_t)m * 12),
                 o_d = o_b + pad16((size_t)m * 12), o_j = o_d + pad16((size_t)n * 4), bytes = o_j + pad16((size_t)n * 4);
    pnr::DevBuf<char> buf; // (freed when the call returns)
    if (buf.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        pnr::set_error("pnr_point_segment_distance: device allocation of %zu B failed", bytes);
        return PNR_E_NOMEM;
    }
    char *const d_buf = buf.get();
    auto fail = [&](hipError_t e) {
        (void)hipStreamSynchronize(st);
        pnr::set_error("pnr_point_segment_distance: %s", hipGetErrorString(e));
        return PNR_E_HIP;
    };
    float4 *const d_seg = (float4 *)d_buf;
    unsigned long long *const d_key = (unsigned long long *)(d_buf + o_key);
    float *const d_pts = (float *)(d_buf + o_pts);
    hipError_t e;
    if ((e = hipMemcpyAsync(d_pts, pts, (size_t)n * 12, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_buf + o_a, seg_a, (size_t)m * 12, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_buf + o_b, seg_b, (size_t)m * 12, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_key, 0xff, (size_t)n * 8, st)) != hipSuccess) return fail(e);
    // the (points x segments) rectangle in launches of at most `budget` pairs (whole block rows; at least one row by one segment)
    const long long budget = c->opt.dist_pairs_per_launch > 0 ? c->opt.dist_pairs_per_launch : AUTO_PAIRS;
    const long long rows_fit = budget / m / DTPB * DTPB;
    const long long rows = std::min<long long>(std::max<long long>(rows_fit, DTPB), (n + DTPB - 1) / DTPB * DTPB);
    const long long segs = rows_fit >= DTPB ? m : std::max<long long>(1, budget / DTPB);
    int launches = 2;
    c->tic();
    hipLaunchKernelGGL(dist_prep, dim3((unsigned)((m + DTPB - 1) / DTPB)), dim3(DTPB), 0, st, (const float *)(d_buf + o_a), (const float *)(d_buf + o_b), (int)m, d_seg);
    e = hipGetLastError();
    for (long long p0 = 0; p0 < n && e == hipSuccess; p0 += rows)
        for (long long s0 = 0; s0 < m && e == hipSuccess; s0 += segs) {
            const long long p1 = std::min<long long>(p0 + rows, n), s1 = std::min<long long>(s0 + segs, m), ms = s1 - s0;
            const long long bx = (p1 - p0 + DTPB - 1) / DTPB;
            long long split = c->opt.dist_split;
            if (split <= 0) { // enough slices to fill the chip, of at least MIN_SPLIT segments
                const long long slices = std::max<long long>(1, std::min<long long>((TARGET_BLOCKS + bx - 1) / bx, ms / MIN_SPLIT));
                split = (ms + slices - 1) / slices;
            }
            split = std::max<long long>(split, (ms + 65534) / 65535); // (gridDim.y)
            const long long by = (ms + split - 1) / split;
            hipLaunchKernelGGL(dist_min, dim3((unsigned)bx, (unsigned)by), dim3(DTPB), 0, st, (const float *)d_pts, (int)p0, (int)p1, (const float4 *)d_seg, (int)s0,
                               (int)s1, (int)split, d_key);
            e = hipGetLastError();
            launches++;
        }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dist_finish, dim3((unsigned)((n + DTPB - 1) / DTPB)), dim3(DTPB), 0, st, (const unsigned long long *)d_key, (int)n, (float *)(d_buf + o_d),
                           (int *)(d_buf + o_j));
        e = hipGetLastError();
    }
    c->toc("distance", launches);
    if (e == hipSuccess) e = hipMemcpyAsync(d_out, d_buf + o_d, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && j_out) e = hipMemcpyAsync(j_out, d_buf + o_j, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    return PNR_OK;
}
