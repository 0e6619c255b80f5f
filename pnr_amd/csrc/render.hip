// render.hip -- a tree rendered into the stack: label volume, mask, coverage counts and residual (pnr_render_tree / pnr_tree_coverage).
// The rule (include/pnr_hip.h): voxel p = (x, y, z * zscale) is inside segment i iff d2(p, segment) <= rt * rt with the point-to-segment
// arithmetic of the tree distance and rt = ra + t * dr; L(p) = 1 + the smallest such i, 0 if none.  Every operation is one IEEE f32
// operation in the order of the header (the build has -ffp-contract=off).
//
// The host cuts every segment along its axis into pieces and gives each piece the box of voxels it can reach (render_items); an item is
// (segment, box), the test always uses the whole segment's constants, so no cut changes a bit.  rn_scatter runs one work-group per item:
// the item and the three float4 of its segment are wave-uniform (scalar loads), the lanes stride over the box with x fastest and a lane
// issues a 32-bit atomicMin of i only where the test passes and the label it just read is larger -- a minimum is order-free.  rn_finish is
// one grid-stride pass of 16-byte label loads that turns the raw minimum into L, writes mask and residual and reduces the coverage
// counts to one 64-bit atomic per work-group and count; the per-segment triples are integer atomics keyed by label, run-length
// combined inside a lane.  The exact byte sum behind thr = -1 is volume.hip's (pnr_mean_threshold).
#include "render.h"
#include "call.h"
#include "grid.h"
#include "volume.h"
#include <cmath>
#include <cstring>

namespace pnr {

int render_prepare(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_render_opts &o, RenderTree &t)
{
    PNR_REQUIRE(std::isfinite(o.zscale) && o.zscale > 0.f, PNR_E_ARG, "%s: zscale = %g must be positive", who, (double)o.zscale);
    PNR_REQUIRE(std::isfinite(o.rscale) && o.rscale >= 0.f, PNR_E_ARG, "%s: rscale = %g must not be negative", who, (double)o.rscale);
    PNR_REQUIRE(std::isfinite(o.radd), PNR_E_ARG, "%s: radd is not finite", who);
    t.n = n;
    t.zscale = o.zscale;
    t.seg.assign((size_t)n * 12, 0.f);
    std::vector<float> p((size_t)n * 3), rr((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const float *v = xyz + 3 * i;
        const float z = v[2] * o.zscale;
        PNR_REQUIRE(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(z), PNR_E_ARG, "%s: node %lld has a coordinate that is not finite", who, (long long)i);
        PNR_REQUIRE(std::isfinite(radius[i]) && radius[i] >= 0.f, PNR_E_ARG, "%s: radius[%lld] = %g must be finite and not negative", who, (long long)i, (double)radius[i]);
        PNR_REQUIRE(parent[i] < n, PNR_E_ARG, "%s: parent[%lld] = %d outside [-1, %lld)", who, (long long)i, parent[i], (long long)n);
        const float r = fmaxf(radius[i] * o.rscale + o.radd, 0.f);
        PNR_REQUIRE(r <= (float)PNR_RENDER_MAX_R, PNR_E_ARG, "%s: the scaled radius %g of node %lld is above %d", who, (double)r, (long long)i, PNR_RENDER_MAX_R);
        p[(size_t)(3 * i)] = v[0], p[(size_t)(3 * i + 1)] = v[1], p[(size_t)(3 * i + 2)] = z;
        rr[(size_t)i] = r;
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t q = parent[i] < 0 ? i : parent[i];
        const float *a = &p[(size_t)(3 * i)], *b = &p[(size_t)(3 * q)];
        const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
        const float den = (abx * abx + aby * aby) + abz * abz;
        const float r = den > 0.f ? 1.0f / den : 0.f;
        const float ra = rr[(size_t)i], rb = rr[(size_t)q];
        float *s = &t.seg[(size_t)(12 * i)];
        s[0] = a[0], s[1] = a[1], s[2] = a[2], s[3] = r;
        s[4] = abx, s[5] = aby, s[6] = abz, s[7] = ra;
        s[8] = rb - ra, s[9] = rb;
    }
    return PNR_OK;
}

void render_items(const RenderTree &t, int64_t w, int64_t h, int64_t l, int64_t piece_opt, int64_t box_opt, const std::function<bool(const RenderItem &)> &f)
{
    const double piece = (double)(piece_opt > 0 ? piece_opt : RENDER_AUTO_PIECE);
    const int64_t box = box_opt > 0 ? box_opt : RENDER_AUTO_BOX;
    const double zs = (double)t.zscale;
    const double scale[3] = {1.0, 1.0, zs};                  // point = voxel index * scale
    const double ext[3] = {(double)(w - 1), (double)(h - 1), (double)(l - 1)};
    for (int64_t i = 0; i < t.n; i++) {
        const float *s = &t.seg[(size_t)(12 * i)];
        const double a[3] = {s[0], s[1], s[2]}, ab[3] = {s[4], s[5], s[6]};
        const double R = (double)std::max(s[7], s[9]) + 1.0; // (the + 1: the f32 rounding of the point on the axis)
        // the part [t0, t1] of the axis from which the grid can be reached at all
        double t0 = 0.0, t1 = 1.0;
        for (int d = 0; d < 3 && t0 <= t1; d++) {
            const double lo = -R, hi = ext[d] * scale[d] + R;
            if (ab[d] == 0.0) {
                if (a[d] < lo || a[d] > hi) t1 = -1.0;
                continue;
            }
            const double u = (lo - a[d]) / ab[d], v = (hi - a[d]) / ab[d];
            t0 = std::max(t0, std::min(u, v));
            t1 = std::min(t1, std::max(u, v));
        }
        if (!(t0 <= t1)) continue;
        const double L = std::sqrt((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]);
        const double q = std::max(1.0, std::ceil(L / piece));
        const double k0 = std::max(0.0, std::floor(t0 * q) - 1.0), k1 = std::min(q - 1.0, std::ceil(t1 * q));
        for (double k = k0; k <= k1; k += 1.0) {
            const double ta = k / q, tb = (k + 1.0) / q;
            int64_t lo[3], hi[3];
            bool empty = false;
            for (int d = 0; d < 3; d++) {
                const double pa = a[d] + ta * ab[d], pb = a[d] + tb * ab[d];
                const double vlo = std::max(0.0, std::floor((std::min(pa, pb) - R) / scale[d]));
                const double vhi = std::min(ext[d], std::ceil((std::max(pa, pb) + R) / scale[d]));
                if (!(vlo <= vhi)) empty = true;
                else lo[d] = (int64_t)vlo, hi[d] = (int64_t)vhi;
            }
            if (empty) continue;
            // sub-boxes of at most `box` voxels: the longest side is halved until the tile fits
            int64_t tile[3] = {hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1};
            while (tile[0] * tile[1] * tile[2] > box) {
                const int d = tile[0] >= tile[1] && tile[0] >= tile[2] ? 0 : tile[1] >= tile[2] ? 1 : 2;
                tile[d] = (tile[d] + 1) / 2;
            }
            for (int64_t z = lo[2]; z <= hi[2]; z += tile[2])
                for (int64_t y = lo[1]; y <= hi[1]; y += tile[1])
                    for (int64_t x = lo[0]; x <= hi[0]; x += tile[0])
                        if (!f(RenderItem{i, x, y, z, std::min(x + tile[0] - 1, hi[0]), std::min(y + tile[1] - 1, hi[1]), std::min(z + tile[2] - 1, hi[2])})) return;
        }
    }
}

} // namespace pnr

namespace {

constexpr int NTPB = 256;          // threads of a work-group
constexpr int NWAVES = NTPB / 64;
constexpr unsigned NONE = 0xffffffffu; // the label of a voxel no segment has reached (one hipMemsetAsync of 0xff)

struct ScatArgs {
    const int4 *items;   // two per item: (seg, x0, y0, z0), (nx, ny, nz, 0)
    const float4 *seg;   // three per segment (render.h)
    unsigned *lab;
    int w, h;
    float zscale;
};

// one work-group per item; the label holds the smallest segment index whose test has passed so far
__global__ __launch_bounds__(NTPB) void rn_scatter(ScatArgs a)
{
    const int4 I0 = a.items[2 * (long long)blockIdx.x], I1 = a.items[2 * (long long)blockIdx.x + 1]; // wave-uniform: scalar loads
    const unsigned seg = (unsigned)I0.x, nx = (unsigned)I1.x, ny = (unsigned)I1.y, nxy = nx * ny, total = nxy * (unsigned)I1.z;
    const float4 A = a.seg[3 * (long long)seg], B = a.seg[3 * (long long)seg + 1], C = a.seg[3 * (long long)seg + 2];
    unsigned v = threadIdx.x;
    if (v >= total) return;
    // the lane's voxel of the box, and the step of NTPB voxels in (x, y, z) with its carries
    unsigned z = v / nxy, y = (v - z * nxy) / nx, x = v - z * nxy - y * nx;
    const unsigned sx = NTPB % nx, sy = (NTPB / nx) % ny, sz = NTPB / nxy;
    for (; v < total; v += NTPB) {
        const int xi = I0.y + (int)x, yi = I0.z + (int)y, zi = I0.w + (int)z;
        const float px = (float)xi, py = (float)yi, pz = (float)zi * a.zscale;
        const float apx = px - A.x, apy = py - A.y, apz = pz - A.z;
        const float num = (apx * B.x + apy * B.y) + apz * B.z;
        const float t = fminf(fmaxf(num * A.w, 0.f), 1.f);
        const float ex = px - (A.x + t * B.x), ey = py - (A.y + t * B.y), ez = pz - (A.z + t * B.z);
        const float d2 = (ex * ex + ey * ey) + ez * ez;
        const float rt = B.w + t * C.x;
        if (d2 <= rt * rt) {
            unsigned *p = a.lab + (((long long)zi * a.h + yi) * a.w + xi);
            if (seg < *p) atomicMin(p, seg);
        }
        x += sx;
        if (x >= nx) x -= nx, y++;
        y += sy;
        if (y >= ny) y -= ny, z++;
        z += sz;
    }
}

struct FinArgs {
    unsigned *lab;           // in: the raw minimum; out (write_label): L
    const uint8_t *V;        // nullable: no coverage
    long long N;
    int t;                   // foreground: V >= t
    int write_label;
    uint8_t *mask, *res;     // nullable; padded to whole 4-byte words
    unsigned long long *cnt; // [1] n_tree, [2] n_fg, [3] n_both, [4] sum_fg, [5] sum_both  ([0]: the byte sum)
    unsigned long long *seg; // nullable: seg_vox[n] | seg_fg[n] | seg_sum[n]
    long long n;
};

// four voxels per lane and step: one 16-byte label load, one 4-byte load of V (bytes where V is not 4-byte aligned, and at the end)
__global__ __launch_bounds__(NTPB) void rn_finish(FinArgs a)
{
    __shared__ unsigned long long part[5][NWAVES];
    const long long groups = (a.N + 3) >> 2, stride = (long long)gridDim.x * NTPB;
    const bool vword = a.V && ((uintptr_t)a.V & 3) == 0;
    unsigned long long c_tree = 0, c_fg = 0, c_both = 0, s_fg = 0, s_both = 0;
    unsigned run = NONE, r_vox = 0, r_fg = 0, r_sum = 0; // the lane's current run of one label (per-segment triples)
    auto flush = [&]() {
        if (run == NONE) return;
        atomicAdd(&a.seg[run], (unsigned long long)r_vox);
        if (r_fg) atomicAdd(&a.seg[a.n + run], (unsigned long long)r_fg);
        if (r_sum) atomicAdd(&a.seg[2 * a.n + run], (unsigned long long)r_sum);
    };
    for (long long g = (long long)blockIdx.x * NTPB + threadIdx.x; g < groups; g += stride) {
        const long long i0 = 4 * g;
        const int k = (int)min(4ll, a.N - i0); // voxels of the group that exist
        unsigned lb[4], vv[4] = {0, 0, 0, 0};
        const uint4 q = ((const uint4 *)a.lab)[g]; // (the buffer is padded to 16 bytes)
        lb[0] = q.x, lb[1] = k > 1 ? q.y : NONE, lb[2] = k > 2 ? q.z : NONE, lb[3] = k > 3 ? q.w : NONE;
        if (a.V) {
            if (vword && k == 4) {
                const unsigned wd = ((const unsigned *)a.V)[g];
                vv[0] = wd & 255u, vv[1] = (wd >> 8) & 255u, vv[2] = (wd >> 16) & 255u, vv[3] = wd >> 24;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (e < k) vv[e] = a.V[i0 + e];
            }
        }
        unsigned mk = 0, rs = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool in = lb[e] != NONE, fg = a.V && e < k && (int)vv[e] >= a.t;
            c_tree += in, c_fg += fg, c_both += in && fg;
            s_fg += fg ? vv[e] : 0u, s_both += in && fg ? vv[e] : 0u;
            mk |= in ? 255u << (8 * e) : 0u;
            rs |= in ? 0u : vv[e] << (8 * e);
            if (a.seg && in) {
                if (lb[e] != run) {
                    flush();
                    run = lb[e], r_vox = r_fg = r_sum = 0;
                }
                r_vox++, r_fg += fg, r_sum += vv[e];
            }
            lb[e] = in ? lb[e] + 1u : 0u;
        }
        if (a.write_label) ((uint4 *)a.lab)[g] = make_uint4(lb[0], lb[1], lb[2], lb[3]);
        if (a.mask) ((unsigned *)a.mask)[g] = mk;
        if (a.res) ((unsigned *)a.res)[g] = rs;
    }
    if (a.seg) flush();
    unsigned long long val[5] = {c_tree, c_fg, c_both, s_fg, s_both};
#pragma unroll
    for (int j = 0; j < 5; j++) {
        for (int d = 32; d >= 1; d >>= 1) val[j] += (unsigned long long)__shfl_xor((long long)val[j], d, 64);
        if ((threadIdx.x & 63) == 0) part[j][threadIdx.x >> 6] = val[j];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned long long s = 0;
        for (int k = 0; k < NWAVES; k++) s += part[threadIdx.x][k];
        if (s) atomicAdd(&a.cnt[1 + threadIdx.x], s);
    }
}

} // namespace

int pnr_render_run(pnr_ctx *c, const char *who, const pnr::RenderTree &t, int64_t w, int64_t h, int64_t l, const uint8_t *V, int thr, int32_t *label_out,
                   uint8_t *mask_out, uint8_t *residual_out, pnr_coverage *cov, int64_t *seg_vox, int64_t *seg_fg, int64_t *seg_sum)
{
    const int64_t N = w * h * l, n = t.n;
    const bool per_seg = (seg_vox || seg_fg || seg_sum) && n > 0;
    // the items are walked twice: counted (the size of the staging buffer; options render_items / render_pairs), then dealt out
    int64_t items = 0, pairs = 0;
    pnr::render_items(t, w, h, l, c->opt.render_piece, c->opt.render_box, [&](const pnr::RenderItem &it) {
        items++;
        pairs += (it.x1 - it.x0 + 1) * (it.y1 - it.y0 + 1) * (it.z1 - it.z0 + 1);
        return true;
    });
    c->render_items = items, c->render_pairs = pairs;
    const int64_t per_launch = c->opt.render_items_per_launch > 0 ? c->opt.render_items_per_launch : pnr::RENDER_AUTO_ITEMS;
    const size_t cap = (size_t)std::max<int64_t>(1, std::min(items, per_launch));
    // device buffers of the call: the labels | the segments | a launch's items | the counts | mask | residual | the per-segment triples
    pnr::CallBuf buf; // (freed when the call returns)
    const auto d_lab = buf.add<unsigned>((size_t)N);
    const auto d_seg = buf.add<float4>((size_t)n * 3);
    const auto d_items = buf.add<int4>(cap * 2);
    const auto d_cnt = buf.add<unsigned long long>(6);
    const auto d_mask = buf.add<uint8_t>(mask_out ? (size_t)N + 4 : 0), d_res = buf.add<uint8_t>(residual_out ? (size_t)N + 4 : 0);
    const auto d_tri = buf.add<unsigned long long>(per_seg ? (size_t)n * 3 : 0);
    int rc = buf.alloc(who);
    if (rc) return rc;
    pnr::Call call(c, who);
    call.fill(d_lab, 0xff);
    call.fill(d_cnt, 0);
    if (per_seg) call.fill(d_tri, 0);
    if (n > 0) call.up(d_seg, t.seg.data());
    // scatter: launches of at most `cap` items; the staging vector is reused once its launch has ended
    std::vector<int32_t> stage;
    stage.reserve(cap * 8);
    const ScatArgs sa{d_items, d_seg, d_lab, (int)w, (int)h, t.zscale};
    auto launch = [&]() {
        const size_t k = stage.size() / 8;
        if (k == 0) return true;
        call.up(d_items.get(), stage.data(), 2 * k);
        call.timed("render_scatter", rn_scatter, dim3((unsigned)k), dim3(NTPB), sa);
        stage.clear();
        return call.finish() == PNR_OK;
    };
    if (items > 0)
        pnr::render_items(t, w, h, l, c->opt.render_piece, c->opt.render_box, [&](const pnr::RenderItem &it) {
            const int32_t row[8] = {(int32_t)it.seg, (int32_t)it.x0, (int32_t)it.y0, (int32_t)it.z0, (int32_t)(it.x1 - it.x0 + 1), (int32_t)(it.y1 - it.y0 + 1), (int32_t)(it.z1 - it.z0 + 1), 0};
            stage.insert(stage.end(), row, row + 8);
            return stage.size() / 8 < cap || launch();
        });
    if (!call.ok() || !launch()) return call.finish();
    // the threshold of the coverage
    int t_abs = thr;
    if (V && thr < 0 && (rc = pnr_mean_threshold(c, who, "render_finish", V, N, d_cnt, &t_abs))) return rc;
    const FinArgs fa{d_lab, V, (long long)N, t_abs, label_out ? 1 : 0, mask_out ? d_mask.get() : nullptr, residual_out ? d_res.get() : nullptr,
                     d_cnt, per_seg ? d_tri.get() : nullptr, (long long)n};
    const long long groups = (N + 3) >> 2;
    call.timed("render_finish", rn_finish, dim3(pnr::grid_blocks((groups + NTPB - 1) / NTPB)), dim3(NTPB), fa);
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    std::vector<int64_t> tri(per_seg ? (size_t)n * 3 : 0);
    call.down(cnt, d_cnt);
    if (label_out) call.down(label_out, d_lab);
    if (mask_out) call.down(mask_out, d_mask.get(), (size_t)N);
    if (residual_out) call.down(residual_out, d_res.get(), (size_t)N);
    if (per_seg) call.down(tri.data(), d_tri);
    if ((rc = call.finish())) return rc;
    if (per_seg) {
        if (seg_vox) std::memcpy(seg_vox, tri.data(), (size_t)n * 8);
        if (seg_fg) std::memcpy(seg_fg, tri.data() + n, (size_t)n * 8);
        if (seg_sum) std::memcpy(seg_sum, tri.data() + 2 * n, (size_t)n * 8);
    }
    if (cov) {
        cov->n_vox = N, cov->n_tree = (int64_t)cnt[1], cov->n_fg = (int64_t)cnt[2], cov->n_both = (int64_t)cnt[3];
        cov->sum_fg = (int64_t)cnt[4], cov->sum_both = (int64_t)cnt[5];
        cov->thr_used = V ? t_abs : 0, cov->pad = 0;
    }
    return PNR_OK;
}
