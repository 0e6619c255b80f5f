// distance.hip -- the point-to-segment rule behind pnr_point_segment_distance / pnr_tree_distance, under the pair minimum of pairmin.h.  The rule
// (include/pnr_hip.h): per segment ab = b - a, den = (ab.x^2 + ab.y^2) + ab.z^2, r = den > 0 ? 1 / den : 0; per pair
// t = min(max(((p - a) . ab) * r, 0), 1), e = p - (a + t ab), d2 = e . e; per point d = sqrt(min_j d2), j* = the smallest j at the minimum.
// Every operation is one IEEE f32 operation in the order of the header (the build has -ffp-contract=off).
//
// dist_prep turns the segments into two float4 each: (a, r) and (ab, 0), so a segment is two scalar dwordx4 loads per wave and the
// vector unit only does the ~25 operations of the pair.  Every pair counts, so a point whose minimum stays +inf reports the first
// segment of the smallest slice.  Above it, the host's side of a tree distance: tree_sample, the
// sampling of a tree; tree_side and direction_metrics, the points and segments of one tree and the metrics of one direction.
#include "distance.h"
#include "call.h"
#include "pairmin.h"
#include <algorithm>
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

int tree_side(const char *which, const float *xyz, const int32_t *parent, int64_t n, const pnr_distance_opts &o, TreeSide &s)
{
    PNR_REQUIRE(n >= 1 && n <= PNR_DISTANCE_MAX_N && xyz && parent, PNR_E_ARG, "pnr_tree_distance: tree %s has %lld nodes (1 to 2^22)", which, (long long)n);
    int rc = tree_sample(xyz, parent, n, o.zscale, o.step, nullptr, nullptr, 0, &s.np);
    if (rc) return rc;
    PNR_REQUIRE(s.np <= PNR_DISTANCE_MAX_N, PNR_E_ARG, "pnr_tree_distance: tree %s has %lld sample points (at most 2^22): raise the step", which, (long long)s.np);
    s.n = n;
    s.pts.resize((size_t)s.np * 3);
    s.owner.resize((size_t)s.np);
    s.d.resize((size_t)s.np);
    if ((rc = tree_sample(xyz, parent, n, o.zscale, o.step, s.pts.data(), s.owner.data(), s.np, &s.np))) return rc;
    s.a.resize((size_t)n * 3);
    s.b.resize((size_t)n * 3);
    for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) s.a[(size_t)(3 * i + k)] = k == 2 ? xyz[3 * i + 2] * o.zscale : xyz[3 * i + k];
    for (int64_t i = 0; i < n; i++) {
        const int64_t q = parent[i] < 0 ? i : parent[i];
        for (int k = 0; k < 3; k++) s.b[(size_t)(3 * i + k)] = s.a[(size_t)(3 * q + k)];
    }
    return PNR_OK;
}
// the metrics of one direction: sequential f64 sums in point order
void direction_metrics(const std::vector<float> &d, float thr, pnr_distance_dir &r)
{
    double sum = 0, sum_big = 0;
    float mx = 0.f;
    int64_t big = 0;
    for (float v : d) {
        sum += (double)v;
        if (v >= thr) sum_big += (double)v, big++;
        mx = std::max(mx, v);
    }
    r.n = (int64_t)d.size();
    r.n_big = big;
    r.mean = sum / (double)r.n;
    r.ssd = big ? sum_big / (double)big : 0.0;
    r.pct = (double)big / (double)r.n;
    r.max = (double)mx;
}

} // namespace pnr

namespace {

constexpr int DTPB = pnr::PAIR_TPB;

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

struct DistRule {
    const float *__restrict__ pts;
    const float4 *__restrict__ seg; // (dist_prep)
    struct Point {
        float x, y, z;
    };
    __device__ Point point(int i) const { return {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}; }
    __device__ bool live(const Point &) const { return true; }
    __device__ int first(int j0) const { return j0; }
    __device__ bool pair(const Point &p, int j, float &d2) const
    {
        const float4 A = seg[2 * j], B = seg[2 * j + 1];
        const float apx = p.x - A.x, apy = p.y - A.y, apz = p.z - A.z;
        const float num = (apx * B.x + apy * B.y) + apz * B.z;
        const float t = fminf(fmaxf(num * A.w, 0.f), 1.f);
        const float ex = p.x - (A.x + t * B.x), ey = p.y - (A.y + t * B.y), ez = p.z - (A.z + t * B.z);
        d2 = (ex * ex + ey * ey) + ez * ez;
        return true;
    }
};

} // namespace

int pnr_distance_run(pnr_ctx *c, const float *pts, int64_t n, const float *seg_a, const float *seg_b, int64_t m, float *d_out, int32_t *j_out)
{
    static const char *who = "pnr_point_segment_distance";
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_seg = buf.add<float4>((size_t)m * 2);
    const auto d_key = buf.add<unsigned long long>((size_t)n);
    const auto d_pts = buf.add<float>((size_t)n * 3), d_a = buf.add<float>((size_t)m * 3), d_b = buf.add<float>((size_t)m * 3), d_d = buf.add<float>((size_t)n);
    const auto d_j = buf.add<int>((size_t)n);
    const int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::Call call(c, who);
    call.up(d_pts, pts);
    call.up(d_a, seg_a);
    call.up(d_b, seg_b);
    call.fill(d_key, 0xff);
    int launches = 0;
    c->tic();
    call.launch(dist_prep, dim3((unsigned)((m + DTPB - 1) / DTPB)), dim3(DTPB), d_a, d_b, (int)m, d_seg);
    if (call.ok()) call.note(pnr::pair_sweep(call.stream(), DistRule{d_pts, d_seg}, n, m, c->opt.dist_split, c->opt.dist_pairs_per_launch, d_key, &launches));
    call.launch(pnr::pair_finish, dim3((unsigned)((n + DTPB - 1) / DTPB)), dim3(DTPB), d_key, (int)n, 1, d_d, d_j);
    c->toc("distance", 2 + launches);
    call.down(d_out, d_d);
    if (j_out) call.down(j_out, d_j);
    return call.finish();
}
