// api_tools.cpp -- the extern "C" boundary of libpnr_hip.so (include/pnr_hip.h), third part: the tools on the volume (filter, components,
// distance transform, skeleton, geodesic distance, morphological reconstruction, watershed, thresholds, radii) and on trees (distance, join, geodesic join, render, prune), with their pure-host test
// taps (include/pnr_hip_test.h).  An entry point checks its arguments first, then the state (args.h holds the shared rules), and hands
// over to the tool's own file; no tool needs or touches the pipeline state of the context (Frangi, seeds, graph).
#include "args.h"
#include "volume.h"
#include "radius.h"
#include "filter.h"
#include "distance.h"
#include "join.h"
#include "pairmin.h"
#include "render.h"
#include "components.h"
#include "edt.h"
#include "thin.h"
#include "geodesic.h"
#include "geojoin.h"
#include "morph.h"
#include "watershed.h"
#include "threshold.h"
#include "prune.h"
#include "../host/stack_io.h"

namespace args = pnr::args;

extern "C" {

// pnr_filter_volume: arguments first, then the state; the context changes only after the filtered volume is complete (filter.hip)
int pnr_filter_volume(pnr_ctx *c, const pnr_filter_opts *opts)
{
    PNR_REQUIRE(c && opts, PNR_E_ARG, "null argument");
    PNR_REQUIRE(opts->median == 0 || opts->median == 2 || opts->median == 3, PNR_E_ARG, "pnr_filter_volume: median = %d, not 0, 2 or 3", opts->median);
    PNR_REQUIRE(opts->tophat_r >= 0 && opts->tophat_r <= PNR_TOPHAT_MAX_R, PNR_E_ARG, "pnr_filter_volume: tophat_r = %d outside [0, %d]", opts->tophat_r, PNR_TOPHAT_MAX_R);
    PNR_TRY(args::volume_set(c, "pnr_filter_volume"));
    if (!opts->median && !opts->tophat_r) return PNR_OK;
    PNR_HIP(hipSetDevice(c->device));
    pnr::DevBuf<uint8_t> out;
    const int rc = pnr_filter_run(c, *opts, out);
    if (!rc) pnr::replace_volume(c, std::move(out));
    return rc;
}

// pnr_label_components / pnr_despeckle_volume (components.hip): arguments first, then the state and the device
static int components_args(pnr_ctx *c, const char *who, const pnr_components_opts *opts, pnr_components_opts &o)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    o = opts ? *opts : pnr_components_opts{-1, 26, 1};
    PNR_TRY(args::thr_range(who, o.thr));
    PNR_REQUIRE(o.connectivity == 6 || o.connectivity == 26, PNR_E_ARG, "%s: connectivity = %d, not 6 or 26", who, o.connectivity);
    PNR_REQUIRE(o.min_size >= 1, PNR_E_ARG, "%s: min_size = %lld must be at least 1", who, (long long)o.min_size);
    return args::volume_u32(c, who);
}

int pnr_label_components(pnr_ctx *c, const pnr_components_opts *opts, pnr_components_info *info, int32_t *label_out, pnr_component *comps, int64_t cap)
{
    static const char *who = "pnr_label_components";
    pnr_components_opts o;
    PNR_TRY(args::cap_not_negative(who, cap));
    PNR_TRY(components_args(c, who, opts, o));
    return pnr_components_run(c, who, o, info, label_out, comps, cap, nullptr);
}

int pnr_despeckle_volume(pnr_ctx *c, const pnr_components_opts *opts, pnr_components_info *info)
{
    static const char *who = "pnr_despeckle_volume";
    pnr_components_opts o;
    PNR_TRY(components_args(c, who, opts, o));
    if (o.min_size == 1) return info ? pnr_components_run(c, who, o, info, nullptr, nullptr, 0, nullptr) : PNR_OK; // nothing can be dropped
    pnr::DevBuf<uint8_t> out;
    const int rc = pnr_components_run(c, who, o, info, nullptr, nullptr, 0, &out);
    if (!rc) pnr::replace_volume(c, std::move(out));
    return rc;
}

// pnr_distance_transform (edt.hip): arguments first, then the state; the pipeline state of the context is neither needed nor touched
int pnr_distance_transform(pnr_ctx *c, const pnr_edt_opts *opts, pnr_edt_info *info, float *d2_out, const float *xyz, int64_t n, float *d2_at)
{
    static const char *who = "pnr_distance_transform";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_edt_opts o = opts ? *opts : pnr_edt_opts{-1, 64};
    PNR_TRY(args::thr_range(who, o.thr));
    PNR_REQUIRE(o.rmax >= 1 && o.rmax <= PNR_EDT_MAX_R, PNR_E_ARG, "%s: rmax = %d outside [1, %d]", who, o.rmax, PNR_EDT_MAX_R);
    PNR_REQUIRE(n >= 0 && n <= PNR_RADIUS_MAX_N && (n == 0 || (xyz && d2_at)), PNR_E_ARG, "%s: n = %lld positions (at most 2^28) need xyz and d2_at", who, (long long)n);
    PNR_TRY(args::volume_u32(c, who));
    return pnr_edt_run(c, who, o, info, d2_out, xyz, n, d2_at);
}

// pnr_skeletonize (thin.hip): arguments first, then the state; the pipeline state of the context is neither needed nor touched
int pnr_skeletonize(pnr_ctx *c, const pnr_thin_opts *opts, pnr_thin_info *info, uint8_t *skel_out, int64_t *vox_out, uint8_t *deg_out, int64_t cap)
{
    static const char *who = "pnr_skeletonize";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_thin_opts o = opts ? *opts : pnr_thin_opts{-1, 0};
    PNR_TRY(args::thr_range(who, o.thr));
    PNR_REQUIRE(o.max_rounds >= 0, PNR_E_ARG, "%s: max_rounds = %d is negative", who, o.max_rounds);
    PNR_TRY(args::cap_not_negative(who, cap));
    PNR_TRY(args::volume_u32(c, who));
    return pnr_thin_run(c, who, o, info, skel_out, vox_out, deg_out, cap);
}

// pnr_skeleton_forest: pure host; the forest itself is thin.h's
int pnr_skeleton_forest(const int64_t *vox, int64_t k, int64_t w, int64_t h, int64_t l, pnr_bridge *edges_out, int64_t cap, int64_t *n_edges)
{
    static const char *who = "pnr_skeleton_forest";
    PNR_REQUIRE(n_edges, PNR_E_ARG, "null argument");
    PNR_REQUIRE(k >= 0 && k <= 0x7fffffffLL && (k == 0 || vox), PNR_E_ARG, "%s: k = %lld voxels (0 to 2^31 - 1) need vox", who, (long long)k);
    PNR_REQUIRE(w >= 1 && h >= 1 && l >= 1 && w < (1LL << 31) && h < (1LL << 31) && l < (1LL << 31) && w * h <= (1LL << 40) / l, PNR_E_ARG, "%s: grid %lld x %lld x %lld", who,
                (long long)w, (long long)h, (long long)l);
    PNR_TRY(args::cap_not_negative(who, cap));
    std::vector<pnr_bridge> edges;
    PNR_TRY(pnr::skeleton_forest(who, vox, k, w, h, l, edges));
    *n_edges = (int64_t)edges.size();
    pnr::put(edges_out, cap, edges);
    return PNR_OK;
}

// pnr_geodesic_distance (geodesic.hip): arguments first, then the state; the pipeline state of the context is neither needed nor touched
int pnr_geodesic_distance(pnr_ctx *c, const float *src_xyz, const int32_t *src_label, int64_t n_src, const pnr_geo_opts *opts, pnr_geo_info *info, uint32_t *d_out,
                          int32_t *label_out, const float *at_xyz, int64_t m, uint32_t *d_at, int32_t *label_at, int32_t path_cap, int32_t *path_len, int64_t *path_vox)
{
    static const char *who = "pnr_geodesic_distance";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_geo_opts o = opts ? *opts : pnr_geo_opts{0, 0x7fffffffu, nullptr};
    PNR_TRY(args::thr_range(who, o.thr));
    PNR_REQUIRE(o.dmax >= 1 && o.dmax <= 0x7fffffffu, PNR_E_ARG, "%s: dmax = %u outside [1, 2^31 - 1]", who, o.dmax);
    PNR_TRY(args::cost_table(who, o.cost));
    PNR_REQUIRE(n_src >= 0 && n_src <= PNR_RADIUS_MAX_N && (n_src == 0 || src_xyz), PNR_E_ARG, "%s: n_src = %lld sources (at most 2^28) need src_xyz", who, (long long)n_src);
    for (int64_t i = 0; src_label && i < n_src; i++) PNR_REQUIRE(src_label[i] >= 0, PNR_E_ARG, "%s: label[%lld] = %d is negative", who, (long long)i, src_label[i]);
    PNR_REQUIRE(path_cap >= 0 && path_cap <= PNR_GEO_MAX_PATH, PNR_E_ARG, "%s: path_cap = %d outside [0, %d]", who, path_cap, PNR_GEO_MAX_PATH);
    PNR_REQUIRE(m >= 0 && m <= PNR_RADIUS_MAX_N && (m == 0 || (at_xyz && (d_at || label_at || path_cap > 0))), PNR_E_ARG,
                "%s: m = %lld targets (at most 2^28) need at_xyz and one of d_at, label_at and path_cap > 0", who, (long long)m);
    PNR_REQUIRE(m == 0 || path_cap == 0 || (path_len && path_vox), PNR_E_ARG, "%s: path_cap = %d needs path_len and path_vox", who, path_cap);
    PNR_TRY(args::volume_u32(c, who));
    return pnr_geodesic_run(c, who, o, pnr_geo_call{src_xyz, src_label, n_src, info, d_out, label_out, at_xyz, m, d_at, label_at, path_cap, path_len, path_vox});
}

// pnr_morph_reconstruct / pnr_morph_volume (morph.hip): arguments first, then the state and the device; o has the connectivity resolved
static int morph_args(pnr_ctx *c, const char *who, const pnr_morph_opts *opts, bool need_marker_rule, const uint8_t *marker, pnr_morph_opts &o)
{
    PNR_REQUIRE(c && opts, PNR_E_ARG, "null argument");
    o = *opts;
    PNR_REQUIRE(o.op >= (need_marker_rule ? PNR_MORPH_DILATE : PNR_MORPH_FILL) && o.op <= PNR_MORPH_HDOME, PNR_E_ARG, "%s: op = %d outside [%d, %d]", who, o.op,
                need_marker_rule ? PNR_MORPH_DILATE : PNR_MORPH_FILL, PNR_MORPH_HDOME);
    PNR_REQUIRE(o.connectivity == 0 || o.connectivity == 4 || o.connectivity == 8 || o.connectivity == 6 || o.connectivity == 26, PNR_E_ARG,
                "%s: connectivity = %d, not 0, 4, 8, 6 or 26", who, o.connectivity);
    const bool with_h = o.op == PNR_MORPH_HMAX || o.op == PNR_MORPH_HDOME, with_marker = o.op == PNR_MORPH_DILATE || o.op == PNR_MORPH_ERODE;
    PNR_REQUIRE(with_h ? o.h >= 1 && o.h <= 255 : o.h == 0, PNR_E_ARG, "%s: h = %d, %s", who, o.h, with_h ? "outside [1, 255]" : "not 0 (only ops 4 and 5 take an h)");
    if (need_marker_rule) PNR_REQUIRE(with_marker == (marker != nullptr), PNR_E_ARG, "%s: op = %d %s", who, o.op, with_marker ? "needs a marker" : "takes no marker");
    if (o.connectivity == 0) o.connectivity = o.op == PNR_MORPH_FILL ? 6 : 26;
    return args::volume_u32(c, who);
}

int pnr_morph_reconstruct(pnr_ctx *c, const pnr_morph_opts *opts, const uint8_t *marker, pnr_morph_info *info, uint8_t *out)
{
    static const char *who = "pnr_morph_reconstruct";
    pnr_morph_opts o;
    PNR_TRY(morph_args(c, who, opts, true, marker, o));
    return pnr_morph_run(c, who, o, marker, info, out, nullptr);
}

int pnr_morph_volume(pnr_ctx *c, const pnr_morph_opts *opts, pnr_morph_info *info)
{
    static const char *who = "pnr_morph_volume";
    pnr_morph_opts o;
    PNR_TRY(morph_args(c, who, opts, false, nullptr, o));
    pnr::DevBuf<uint8_t> out;
    const int rc = pnr_morph_run(c, who, o, nullptr, info, nullptr, &out);
    if (!rc) pnr::replace_volume(c, std::move(out));
    return rc;
}

// pnr_watershed (watershed.hip): arguments in the order of the header, then the state and the device, then the marker volume's entries
int pnr_watershed(pnr_ctx *c, const pnr_watershed_opts *opts, const uint8_t *relief, const int32_t *marker_vol, const float *src_xyz, const int32_t *src_label, int64_t n_src,
                  pnr_watershed_info *info, int32_t *label_out, uint8_t *level_out)
{
    static const char *who = "pnr_watershed";
    PNR_REQUIRE(c && opts, PNR_E_ARG, "null argument");
    pnr_watershed_opts o = *opts;
    PNR_TRY(args::thr_range(who, o.thr));
    PNR_REQUIRE(o.connectivity == 0 || o.connectivity == 4 || o.connectivity == 8 || o.connectivity == 6 || o.connectivity == 26, PNR_E_ARG,
                "%s: connectivity = %d, not 0, 4, 8, 6 or 26", who, o.connectivity);
    PNR_REQUIRE(n_src >= 0 && n_src <= 0x7ffffffeLL, PNR_E_ARG, "%s: n_src = %lld outside [0, 2^31 - 2]", who, (long long)n_src);
    PNR_REQUIRE(!(marker_vol && (n_src > 0 || src_xyz || src_label)), PNR_E_ARG, "%s: markers as a volume and as points, exactly one of the two forms", who);
    PNR_REQUIRE(marker_vol || n_src > 0, PNR_E_ARG, "%s: no markers, neither marker_vol nor n_src > 0", who);
    PNR_REQUIRE(marker_vol || src_xyz, PNR_E_ARG, "%s: n_src = %lld needs src_xyz", who, (long long)n_src);
    for (int64_t i = 0; src_label && i < n_src; i++)
        PNR_REQUIRE(src_label[i] >= 1, PNR_E_ARG, "%s: src_label[%lld] = %d, labels are at least 1", who, (long long)i, src_label[i]);
    if (o.connectivity == 0) o.connectivity = 26;
    PNR_TRY(args::volume_u32(c, who));
    int64_t n_pos = 0;
    for (int64_t i = 0; marker_vol && i < c->N; i++) {
        PNR_REQUIRE(marker_vol[i] >= 0, PNR_E_ARG, "%s: marker_vol[%lld] = %d is negative", who, (long long)i, marker_vol[i]);
        n_pos += marker_vol[i] > 0;
    }
    return pnr_watershed_run(c, who, o, relief, pnr_ws_markers{marker_vol, n_pos, src_xyz, src_label, n_src}, info, label_out, level_out);
}

// ---- thresholds (threshold_rule.cpp, threshold.hip): the rule checks its own arguments; then the state and the device ----
int pnr_threshold_from_hist(const uint64_t *hist, const pnr_threshold_opts *opts, pnr_threshold_info *info)
{
    return pnr::threshold_rule("pnr_threshold_from_hist", hist, opts, info);
}

int pnr_auto_threshold(pnr_ctx *c, const pnr_threshold_opts *opts, pnr_threshold_info *info, uint64_t *hist_out)
{
    static const char *who = "pnr_auto_threshold";
    PNR_REQUIRE(c && opts && info, PNR_E_ARG, "null argument");
    uint64_t hist[256] = {0};
    pnr_threshold_info dry;
    PNR_TRY(pnr::threshold_rule(who, hist, opts, &dry)); // (the arguments, before any work)
    PNR_TRY(args::volume_set(c, who));
    PNR_HIP(hipSetDevice(c->device));
    PNR_TRY(pnr_hist_run(c, who, "threshold", c->d_img, c->N, hist));
    PNR_TRY(pnr::threshold_rule(who, hist, opts, info));
    if (hist_out) std::copy(hist, hist + 256, hist_out);
    return PNR_OK;
}

static int local_args(pnr_ctx *c, const char *who, const pnr_local_opts *opts, bool need_volume = true)
{
    PNR_REQUIRE(c && opts, PNR_E_ARG, "null argument");
    PNR_REQUIRE(opts->r >= 1 && opts->r <= PNR_LOCAL_MAX_R, PNR_E_ARG, "%s: r = %d outside [1, %d]", who, opts->r, PNR_LOCAL_MAX_R);
    PNR_REQUIRE(opts->offset >= -255 && opts->offset <= 255, PNR_E_ARG, "%s: offset = %d outside [-255, 255]", who, opts->offset);
    PNR_REQUIRE(opts->scale_256 >= 0 && opts->scale_256 <= 4096, PNR_E_ARG, "%s: scale_256 = %d outside [0, 4096]", who, opts->scale_256);
    PNR_REQUIRE(opts->floor >= 1 && opts->floor <= 255, PNR_E_ARG, "%s: floor = %d outside [1, 255]", who, opts->floor);
    PNR_REQUIRE(opts->binary == 0 || opts->binary == 1, PNR_E_ARG, "%s: binary = %d, not 0 or 1", who, opts->binary);
    if (need_volume) PNR_TRY(args::volume_set(c, who));
    PNR_HIP(hipSetDevice(c->device));
    return PNR_OK;
}

int pnr_local_threshold(pnr_ctx *c, const pnr_local_opts *opts, pnr_local_info *info, uint8_t *out)
{
    static const char *who = "pnr_local_threshold";
    PNR_TRY(local_args(c, who, opts));
    return pnr_local_run(c, who, pnr_local_vol_of(c), *opts, info, out, nullptr);
}

int pnr_local_threshold_volume(pnr_ctx *c, const pnr_local_opts *opts, pnr_local_info *info)
{
    static const char *who = "pnr_local_threshold_volume";
    PNR_TRY(local_args(c, who, opts));
    pnr::DevBuf<uint8_t> out;
    const int rc = pnr_local_run(c, who, pnr_local_vol_of(c), *opts, info, nullptr, &out);
    if (!rc) pnr::replace_volume(c, std::move(out));
    return rc;
}

// test taps (pnr_hip_test.h): the two kernels' entry points on bytes of any size, also below the 2 x 2 x 1 a context takes as its volume
int pnr_test_histogram(pnr_ctx *c, const uint8_t *bytes, int64_t n, int32_t offset, uint64_t *hist)
{
    static const char *who = "pnr_test_histogram";
    PNR_REQUIRE(c && bytes && hist, PNR_E_ARG, "null argument");
    PNR_REQUIRE(n >= 1 && n <= (1LL << 32) && offset >= 0 && offset <= 15, PNR_E_ARG, "%s: n = %lld bytes (1 to 2^32) at offset %d (0 to 15)", who, (long long)n, offset);
    PNR_HIP(hipSetDevice(c->device));
    pnr::DevBuf<uint8_t> buf;
    PNR_TRY(pnr::dev_alloc(buf, (size_t)n + 16, who));
    uint8_t *V = buf.get() + ((16 - ((uintptr_t)buf.get() & 15)) & 15) + offset; // `offset` bytes past a 16-byte boundary
    PNR_HIP(hipMemcpy(V, bytes, (size_t)n, hipMemcpyHostToDevice));
    return pnr_hist_run(c, who, "threshold", V, n, hist);
}

int pnr_test_local_threshold(pnr_ctx *c, const uint8_t *vol, int64_t w, int64_t h, int64_t l, const pnr_local_opts *opts, pnr_local_info *info, uint8_t *out)
{
    static const char *who = "pnr_test_local_threshold";
    PNR_REQUIRE(vol && out, PNR_E_ARG, "null argument");
    PNR_REQUIRE(w >= 1 && h >= 1 && l >= 1 && w <= 1 << 20 && h <= 1 << 20 && l <= 1 << 20 && w * h * l <= (1LL << 32), PNR_E_ARG, "%s: volume %lld x %lld x %lld", who, (long long)w,
                (long long)h, (long long)l);
    PNR_TRY(local_args(c, who, opts, false));
    pnr::DevBuf<uint8_t> buf;
    PNR_TRY(pnr::dev_alloc(buf, (size_t)(w * h * l), who));
    PNR_HIP(hipMemcpy(buf.get(), vol, (size_t)(w * h * l), hipMemcpyHostToDevice));
    return pnr_local_run(c, who, pnr_local_vol{buf.get(), w, h, l}, *opts, info, out, nullptr);
}

// pnr_measure_radii: arguments first, then the state; the pipeline state of the context (Frangi, seeds, graph) is neither needed nor touched
int pnr_measure_radii(pnr_ctx *c, const float *xyz, int64_t n, const pnr_radius_opts *opts, int32_t *k_out, int32_t *thr_used)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_radius_opts o = opts ? *opts : pnr_radius_opts{-1, 50, 32, 1};
    PNR_REQUIRE(o.rmax >= 1 && o.rmax <= PNR_RADIUS_MAX, PNR_E_ARG, "pnr_measure_radii: rmax = %d outside [1, %d]", o.rmax, PNR_RADIUS_MAX);
    PNR_TRY(args::thr_range("pnr_measure_radii", o.thr));
    PNR_REQUIRE(o.rel_pct >= 0 && o.rel_pct <= 100, PNR_E_ARG, "pnr_measure_radii: rel_pct = %d outside [0, 100]", o.rel_pct);
    PNR_REQUIRE(o.bg_permille >= 0 && o.bg_permille <= 999, PNR_E_ARG, "pnr_measure_radii: bg_permille = %d outside [0, 999]", o.bg_permille);
    PNR_REQUIRE(n >= 0 && n <= PNR_RADIUS_MAX_N && (n == 0 || (xyz && k_out)), PNR_E_ARG, "pnr_measure_radii: n = %lld positions (at most 2^28) need xyz and k_out", (long long)n);
    PNR_TRY(args::volume_set(c, "pnr_measure_radii"));
    PNR_HIP(hipSetDevice(c->device));
    return pnr_radius_run(c, xyz, n, o, k_out, thr_used);
}

// ---- tree distance (distance.hip): arguments first; neither a volume nor any pipeline state is needed or touched ----
int pnr_point_segment_distance(pnr_ctx *c, const float *pts, int64_t n, const float *seg_a, const float *seg_b, int64_t m, float *d_out, int32_t *j_out)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(m >= 1 && m <= PNR_DISTANCE_MAX_N && seg_a && seg_b, PNR_E_ARG, "pnr_point_segment_distance: m = %lld segments (1 to 2^22) need seg_a and seg_b", (long long)m);
    PNR_REQUIRE(n >= 0 && n <= PNR_DISTANCE_MAX_N && (n == 0 || (pts && d_out)), PNR_E_ARG, "pnr_point_segment_distance: n = %lld points (at most 2^22) need pts and d_out", (long long)n);
    PNR_REQUIRE(args::all_finite(seg_a, 3 * m) && args::all_finite(seg_b, 3 * m) && args::all_finite(pts, 3 * n), PNR_E_ARG, "pnr_point_segment_distance: a coordinate is not finite");
    if (n == 0) return PNR_OK;
    PNR_HIP(hipSetDevice(c->device));
    return pnr_distance_run(c, pts, n, seg_a, seg_b, m, d_out, j_out);
}

int pnr_tree_sample(const float *xyz, const int32_t *parent, int64_t n, float zscale, float step, float *pts_out, int32_t *owner_out, int64_t cap, int64_t *n_out)
{
    PNR_REQUIRE(n >= 0 && n <= PNR_DISTANCE_MAX_N && (n == 0 || (xyz && parent)) && n_out && cap >= 0, PNR_E_ARG, "pnr_tree_sample: n = %lld nodes (at most 2^22) need xyz, parent and n_out", (long long)n);
    PNR_TRY(args::positive("pnr_tree_sample", "zscale", zscale));
    PNR_TRY(args::not_negative("pnr_tree_sample", "step", step));
    return pnr::tree_sample(xyz, parent, n, zscale, step, pts_out, owner_out, cap, n_out);
}

int pnr_tree_distance(pnr_ctx *c, const float *xyzA, const int32_t *parentA, int64_t nA, const float *xyzB, const int32_t *parentB, int64_t nB,
                      const pnr_distance_opts *opts, pnr_distance_result *result, float *dA_out, int32_t *ownerA_out, int64_t capA, float *dB_out,
                      int32_t *ownerB_out, int64_t capB)
{
    PNR_REQUIRE(c && result, PNR_E_ARG, "null argument");
    const pnr_distance_opts o = opts ? *opts : pnr_distance_opts{1.f, 1.f, 2.f};
    PNR_TRY(args::positive("pnr_tree_distance", "zscale", o.zscale));
    PNR_TRY(args::not_negative("pnr_tree_distance", "step", o.step));
    PNR_REQUIRE(std::isfinite(o.thr), PNR_E_ARG, "pnr_tree_distance: thr is not finite");
    PNR_REQUIRE(capA >= 0 && capB >= 0, PNR_E_ARG, "pnr_tree_distance: negative capacity");
    pnr::TreeSide A, B;
    PNR_TRY(pnr::tree_side("A", xyzA, parentA, nA, o, A));
    PNR_TRY(pnr::tree_side("B", xyzB, parentB, nB, o, B));
    PNR_HIP(hipSetDevice(c->device));
    PNR_TRY(pnr_distance_run(c, A.pts.data(), A.np, B.a.data(), B.b.data(), B.n, A.d.data(), nullptr));
    PNR_TRY(pnr_distance_run(c, B.pts.data(), B.np, A.a.data(), A.b.data(), A.n, B.d.data(), nullptr));
    pnr::direction_metrics(A.d, o.thr, result->ab);
    pnr::direction_metrics(B.d, o.thr, result->ba);
    result->sd = (result->ab.mean + result->ba.mean) / 2;
    result->ssd = (result->ab.ssd + result->ba.ssd) / 2;
    result->pct = (result->ab.pct + result->ba.pct) / 2;
    result->hausdorff = std::max(result->ab.max, result->ba.max);
    pnr::put(dA_out, capA, A.d), pnr::put(ownerA_out, capA, A.owner);
    pnr::put(dB_out, capB, B.d), pnr::put(ownerB_out, capB, B.owner);
    return PNR_OK;
}

// ---- joining the forest (join.hip): arguments first; neither a volume nor any pipeline state is needed or touched ----
int pnr_nearest_other(pnr_ctx *c, const float *xyz, const int32_t *label, int64_t n, float *d_out, int32_t *j_out)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(n >= 1 && n <= PNR_JOIN_MAX_N && xyz && label && d_out && j_out, PNR_E_ARG, "pnr_nearest_other: n = %lld points (1 to 2^22) need xyz, label, d_out and j_out", (long long)n);
    PNR_REQUIRE(args::all_finite(xyz, 3 * n), PNR_E_ARG, "pnr_nearest_other: a coordinate is not finite");
    PNR_HIP(hipSetDevice(c->device));
    pnr::JoinSearch search;
    const int rc = search.begin(c, xyz, n, "pnr_nearest_other");
    return rc ? rc : search.run(label, true, d_out, j_out, "pnr_nearest_other");
}

int pnr_join_reroot(const int32_t *parent, int64_t n, const pnr_bridge *bridges, int64_t nb, int64_t root, int32_t *parent_out, int32_t *order_out, int32_t *comp_out)
{
    PNR_REQUIRE(n >= 1 && n <= PNR_JOIN_MAX_N && parent, PNR_E_ARG, "pnr_join_reroot: n = %lld nodes (1 to 2^22) need parent", (long long)n);
    PNR_REQUIRE(nb >= 0 && nb < n && (nb == 0 || bridges), PNR_E_ARG, "pnr_join_reroot: %lld bridges (0 to n - 1) need bridges", (long long)nb);
    return pnr::join_reroot(parent, n, bridges, nb, root, parent_out, order_out, comp_out, nullptr);
}

int pnr_join_trees(pnr_ctx *c, const float *xyz, const int32_t *parent, int64_t n, const pnr_join_opts *opts, int32_t *parent_out, int32_t *order_out,
                   int32_t *comp_out, pnr_bridge *bridges_out, int64_t cap_bridges, int64_t *n_bridges, int64_t *n_trees_in, int64_t *n_trees_out)
{
    PNR_REQUIRE(c && n_bridges, PNR_E_ARG, "null argument");
    PNR_REQUIRE(n >= 1 && n <= PNR_JOIN_MAX_N && xyz && parent, PNR_E_ARG, "pnr_join_trees: n = %lld nodes (1 to 2^22) need xyz and parent", (long long)n);
    const pnr_join_opts o = opts ? *opts : pnr_join_opts{1.f, 0.f, -1};
    PNR_TRY(args::positive("pnr_join_trees", "zscale", o.zscale));
    PNR_TRY(args::not_negative("pnr_join_trees", "gap", o.gap));
    PNR_REQUIRE(o.root < n, PNR_E_ARG, "pnr_join_trees: root = %d outside [-1, %lld)", o.root, (long long)n);
    PNR_CAP_NEEDS("pnr_join_trees", cap_bridges, bridges_out);
    std::vector<float> scaled(xyz, xyz + 3 * n);
    for (int64_t i = 0; i < n; i++) {
        float *p = &scaled[(size_t)(3 * i)];
        p[2] = p[2] * o.zscale;
        PNR_REQUIRE(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(xyz[3 * i + 2]) && std::isfinite(p[2]), PNR_E_ARG,
                    "pnr_join_trees: node %lld has a coordinate that is not finite", (long long)i);
    }
    PNR_HIP(hipSetDevice(c->device));
    std::vector<pnr_bridge> bridges;
    int64_t trees_in = 0, trees_out = 0;
    PNR_TRY(pnr::join_bridges(c, scaled.data(), parent, n, o.gap, bridges, &trees_in, &c->join_rounds));
    PNR_TRY(pnr::join_reroot(parent, n, bridges.data(), (int64_t)bridges.size(), o.root, parent_out, order_out, comp_out, &trees_out));
    *n_bridges = (int64_t)bridges.size();
    pnr::put(bridges_out, cap_bridges, bridges);
    if (n_trees_in) *n_trees_in = trees_in;
    if (n_trees_out) *n_trees_out = trees_out;
    return PNR_OK;
}

// ---- joining the forest along the signal (geojoin.hip): arguments first, then the state; the pipeline state is neither needed nor touched ----
int pnr_geodesic_bridges(pnr_ctx *c, const float *xyz, const int32_t *parent, int64_t n, const pnr_geojoin_opts *opts, pnr_geojoin_info *info, pnr_geo_bridge *bridges_out,
                         int64_t cap_bridges, int64_t *n_bridges, int64_t *path_vox, int64_t cap_path, int64_t *n_path)
{
    static const char *who = "pnr_geodesic_bridges";
    PNR_REQUIRE(c && n_bridges && n_path, PNR_E_ARG, "null argument");
    PNR_REQUIRE(n >= 1 && n <= PNR_JOIN_MAX_N && xyz && parent, PNR_E_ARG, "%s: n = %lld nodes (1 to 2^22) need xyz and parent", who, (long long)n);
    const pnr_geojoin_opts o = opts ? *opts : pnr_geojoin_opts{0, 0, 1.f, nullptr};
    PNR_TRY(args::thr_range(who, o.thr));
    PNR_TRY(args::not_negative(who, "step", o.step));
    PNR_TRY(args::cost_table(who, o.cost));
    PNR_CAP_NEEDS(who, cap_bridges, bridges_out);
    PNR_CAP_NEEDS(who, cap_path, path_vox);
    PNR_TRY(args::volume_u32(c, who));
    std::vector<pnr_geo_bridge> bridges;
    std::vector<int64_t> chain;
    PNR_TRY(pnr_geojoin_run(c, xyz, parent, n, o, info, bridges, chain));
    *n_bridges = (int64_t)bridges.size();
    *n_path = (int64_t)chain.size();
    pnr::put(bridges_out, cap_bridges, bridges), pnr::put(path_vox, cap_path, chain);
    return PNR_OK;
}

int pnr_join_expand(const float *xyz, const int32_t *parent, int64_t n, const pnr_geo_bridge *bridges, int64_t nb, const int64_t *path_vox, int64_t n_path, int64_t w, int64_t h,
                    int64_t l, float *xyz_out, int32_t *parent_out, int32_t *bridge_of, int64_t cap_nodes, int64_t *n_nodes, pnr_bridge *join_out)
{
    static const char *who = "pnr_join_expand";
    PNR_REQUIRE(n >= 1 && n <= PNR_JOIN_MAX_N && xyz && parent && n_nodes, PNR_E_ARG, "%s: n = %lld nodes (1 to 2^22) need xyz, parent and n_nodes", who, (long long)n);
    PNR_REQUIRE(nb >= 0 && nb < n && (nb == 0 || bridges), PNR_E_ARG, "%s: %lld bridges (0 to n - 1) need bridges", who, (long long)nb);
    PNR_REQUIRE(n_path >= 0 && (nb == 0 || path_vox) && cap_nodes >= 0, PNR_E_ARG, "%s: %lld bridges need path_vox", who, (long long)nb);
    PNR_REQUIRE(w >= 1 && h >= 1 && l >= 1 && w < (1 << 24) && h < (1 << 24) && l < (1 << 24), PNR_E_ARG, "%s: the grid %lld x %lld x %lld needs sides from 1 and below 2^24", who,
                (long long)w, (long long)h, (long long)l);
    for (int64_t i = 0; i < n; i++) PNR_REQUIRE(parent[i] < n, PNR_E_ARG, "%s: parent[%lld] = %d outside [-1, %lld)", who, (long long)i, parent[i], (long long)n);
    return pnr_geojoin_expand(xyz, parent, n, bridges, nb, path_vox, n_path, w, h, l, xyz_out, parent_out, bridge_of, cap_nodes, n_nodes, join_out);
}

// ---- pruning the tree (prune_rule.cpp, prune.hip): the shared arguments first; neither a volume nor any pipeline state is needed or touched ----
int pnr_prune_tree(pnr_ctx *c, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts *opts, pnr_prune_info *info, uint8_t *keep,
                   uint32_t *height, uint32_t *path, int32_t *order, int32_t *seg)
{
    static const char *who = "pnr_prune_tree";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    pnr_prune_opts o;
    PNR_TRY(pnr::prune_args(who, xyz, radius, parent, n, opts, o));
    PNR_HIP(hipSetDevice(c->device));
    return pnr_prune_run(c, who, xyz, radius, parent, n, o, info, keep, height, path, order, seg);
}

int pnr_prune_tree_host(const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts *opts, pnr_prune_info *info, uint8_t *keep,
                        uint32_t *height, uint32_t *path, int32_t *order, int32_t *seg)
{
    static const char *who = "pnr_prune_tree_host";
    pnr_prune_opts o;
    PNR_TRY(pnr::prune_args(who, xyz, radius, parent, n, opts, o));
    return pnr::prune_rule(who, xyz, radius, parent, n, o, info, keep, height, path, order, seg);
}

int pnr_prune_apply(const int32_t *parent, const uint8_t *keep, int64_t n, int32_t *new_index_out, int32_t *parent_out, int64_t *m)
{
    return pnr::prune_apply(parent, keep, n, new_index_out, parent_out, m);
}

// ---- rendering the tree (render.hip): arguments first; pnr_render_tree needs no volume, neither call touches the pipeline state ----
static pnr_render_opts default_render_opts(const pnr_render_opts *opts) { return opts ? *opts : pnr_render_opts{1.f, 1.f, 0.f, -1}; }
static int render_grid_ok(const char *who, int64_t w, int64_t h, int64_t l)
{
    const int64_t lim = 0x7fffffffll;
    PNR_REQUIRE(w >= 1 && h >= 1 && l >= 1 && w <= lim && h <= lim && l <= lim && w <= (1ll << 40) / h && w * h <= (1ll << 40) / l, PNR_E_ARG,
                "%s: the grid %lld x %lld x %lld needs sides from 1 and at most 2^40 voxels", who, (long long)w, (long long)h, (long long)l);
    return PNR_OK;
}
// the checks the three entry points share, in their order: the tree's size and thr, the grid (where the call has one), the tree's values
static int render_args(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_render_opts &o, bool grid, int64_t w, int64_t h,
                       int64_t l, pnr::RenderTree &t)
{
    PNR_REQUIRE(n >= 0 && n <= PNR_RENDER_MAX_N && (n == 0 || (xyz && radius && parent)), PNR_E_ARG, "%s: n = %lld nodes (at most 2^22) need xyz, radius and parent", who, (long long)n);
    PNR_TRY(args::thr_range(who, o.thr));
    if (grid) PNR_TRY(render_grid_ok(who, w, h, l));
    return pnr::render_prepare(who, xyz, radius, parent, n, o, t);
}

int pnr_render_tree(pnr_ctx *c, const float *xyz, const float *radius, const int32_t *parent, int64_t n, int64_t w, int64_t h, int64_t l,
                    const pnr_render_opts *opts, int32_t *label_out, uint8_t *mask_out)
{
    static const char *who = "pnr_render_tree";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_render_opts o = default_render_opts(opts);
    pnr::RenderTree t;
    PNR_TRY(render_args(who, xyz, radius, parent, n, o, true, w, h, l, t));
    PNR_HIP(hipSetDevice(c->device));
    return pnr_render_run(c, who, t, w, h, l, nullptr, 0, label_out, mask_out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int pnr_tree_coverage(pnr_ctx *c, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_render_opts *opts, pnr_coverage *cov,
                      int64_t *seg_vox, int64_t *seg_fg, int64_t *seg_sum, uint8_t *mask_out, uint8_t *residual_out)
{
    static const char *who = "pnr_tree_coverage";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_render_opts o = default_render_opts(opts);
    pnr::RenderTree t;
    PNR_TRY(render_args(who, xyz, radius, parent, n, o, false, 0, 0, 0, t));
    PNR_TRY(args::volume_set(c, who));
    PNR_HIP(hipSetDevice(c->device));
    pnr_coverage r;
    std::memset(&r, 0, sizeof(r));
    PNR_TRY(pnr_render_run(c, who, t, c->w, c->h, c->l, c->d_img, o.thr, nullptr, mask_out, residual_out, &r, seg_vox, seg_fg, seg_sum));
    r.covered = r.n_fg ? (double)r.n_both / (double)r.n_fg : 0.0;
    r.on_signal = r.n_tree ? (double)r.n_both / (double)r.n_tree : 0.0;
    r.covered_intensity = r.sum_fg ? (double)r.sum_both / (double)r.sum_fg : 0.0;
    if (cov) *cov = r;
    return PNR_OK;
}

// the rows of pnr_render_items and pnr_pair_tiles: seven values each, written while the capacity lasts and counted on
namespace {
struct Rows7 {
    int64_t *out, cap, k = 0;
    bool add(const int64_t (&row)[7])
    {
        if (k < cap) std::copy(row, row + 7, out + 7 * k);
        k++;
        return true;
    }
};
} // namespace

// test tap (pnr_hip_test.h): the work items of a render, pure host
int pnr_render_items(const float *xyz, const float *radius, const int32_t *parent, int64_t n, int64_t w, int64_t h, int64_t l, const pnr_render_opts *opts,
                     int64_t piece, int64_t box, int64_t *items_out, int64_t cap, int64_t *count)
{
    static const char *who = "pnr_render_items";
    PNR_REQUIRE(count && piece >= 0 && box >= 0 && (cap <= 0 || items_out), PNR_E_ARG, "%s: piece and box (not negative) need a count, and items_out for cap = %lld", who, (long long)cap);
    const pnr_render_opts o = default_render_opts(opts);
    pnr::RenderTree t;
    PNR_TRY(render_args(who, xyz, radius, parent, n, o, true, w, h, l, t));
    Rows7 rows{items_out, cap};
    pnr::render_items(t, w, h, l, piece, box, [&](const pnr::RenderItem &it) { return rows.add({it.seg, it.x0, it.y0, it.z0, it.x1, it.y1, it.z1}); });
    *count = rows.k;
    return PNR_OK;
}

// test tap (pnr_hip_test.h): the host's volume writer
int pnr_test_write_tiff(const char *path, const uint8_t *img, int64_t w, int64_t h, int64_t l)
{
    PNR_REQUIRE(path && w >= 1 && h >= 1 && l >= 1, PNR_E_ARG, "pnr_test_write_tiff: a path and sides from 1");
    const std::string name = path;
    const bool raw = name.size() > 4 && name.substr(name.size() - 4) == ".raw";
    std::string err;
    if (!raw && advantra::tiff_u8_bytes(w, h, l) < 0) img = (const uint8_t *)""; // (refused from the dimensions: never read)
    PNR_REQUIRE(img, PNR_E_ARG, "pnr_test_write_tiff: null image");
    PNR_REQUIRE(advantra::save_stack_u8(name, img, w, h, l, err), PNR_E_ARG, "%s", err.c_str());
    return PNR_OK;
}

int pnr_live_bytes(int64_t *device, int64_t *pinned)
{
    if (device) *device = pnr::live_device_bytes.load();
    if (pinned) *pinned = pnr::live_pinned_bytes.load();
    return PNR_OK;
}

// test tap (pnr_hip_test.h): the shells of the rule, pure host
int pnr_radius_offsets(float zdist, int rmax, int is2d, int32_t *starts, int32_t *dx, int32_t *dy, int32_t *dz, int64_t cap, int64_t *n)
{
    PNR_REQUIRE(rmax >= 1 && rmax <= PNR_RADIUS_MAX && n, PNR_E_ARG, "pnr_radius_offsets: rmax = %d outside [1, %d], or null count", rmax, PNR_RADIUS_MAX);
    pnr::RadiusTable t;
    pnr::build_radius_table(zdist, rmax, is2d != 0, t);
    *n = (int64_t)t.off.size();
    if (starts) std::copy(t.start.begin(), t.start.end(), starts);
    for (int64_t i = 0; i < std::min(cap, *n); i++) {
        const uint32_t o = t.off[(size_t)i];
        if (dx) dx[i] = (int32_t)(o & 255u) - 64;
        if (dy) dy[i] = (int32_t)((o >> 8) & 255u) - 64;
        if (dz) dz[i] = (int32_t)((o >> 16) & 255u) - 64;
    }
    return PNR_OK;
}

// test tap (pnr_hip_test.h): the launch plan of the pair minimum, pure host
int pnr_pair_tiles(int64_t n, int64_t m, int64_t split, int64_t budget, int64_t *tiles, int64_t cap, int64_t *count)
{
    PNR_REQUIRE(n >= 1 && m >= 1 && split >= 0 && budget >= 0 && count && (cap <= 0 || tiles), PNR_E_ARG,
                "pnr_pair_tiles: %lld x %lld (at least 1 x 1), split = %lld and budget = %lld (not negative) need a count, and tiles for cap = %lld", (long long)n,
                (long long)m, (long long)split, (long long)budget, (long long)cap);
    Rows7 rows{tiles, cap};
    pnr::pair_tiles(n, m, split, budget, [&](const pnr::PairTile &t) { return rows.add({t.p0, t.p1, t.s0, t.s1, t.split, t.gx, t.gy}); });
    *count = rows.k;
    return PNR_OK;
}

} // extern "C"
