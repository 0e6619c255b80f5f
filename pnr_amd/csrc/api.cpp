// api.cpp -- the extern "C" boundary of libpnr_hip.so (include/pnr_hip.h): context life-cycle,
// parameter validation (Advantra::dofunc, Advantra_plugin.cpp:317-326), uploads/read-backs, the
// seed filter/sort (:2561-2586) and the host replay of the trace bookkeeping
// (tracker.cpp:825-933 + Advantra_plugin.cpp:2602-2710).
#include "call.h"
#include "replay.h"
#include "stream_sched.h"
#include "../host/reconstruct.h"
#include "recon.h"
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
#include "../host/stack_io.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <unordered_map>
#include <fstream>
#include <thread>
#include <sched.h>

namespace pnr {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// worker threads for the host-side stages (seed flood fill, reconstruct()): the CPUs this process may run on (affinity mask,
// cgroup quota), shared between the ranks of this host (one process per GPU)
int host_threads(const Options &o)
{
    if (o.host_threads > 0) return o.host_threads;
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    std::ifstream f("/sys/fs/cgroup/cpu.max"); // "<quota> <period>" or "max <period>"
    std::string q;
    long long per = 0;
    if (f >> q >> per && q != "max" && per > 0) {
        const long long lim = (atoll(q.c_str()) + per - 1) / per;
        if (lim > 0 && lim < n) n = (int)lim;
    }
    n /= std::max(1, o.local_ranks);
    return std::min(std::max(n, 1), 32); // the fills of a stack's layers stop scaling long before that
}
} // namespace pnr

using pnr::set_error;

// tracker tables for the 3-D (default) or the 2-D (single-slice stack, P == 1) branch of Tracker::Tracker: built on the host,
// resident on the device.  Rebuilt when pnr_set_volume changes the dimensionality.
static int load_tables(pnr_ctx *c, bool is2d)
{
    pnr::build_tables(c->prm, is2d, c->tab);
    const pnr::Tables &t = c->tab;
    const std::vector<float> sig(c->prm.sig, c->prm.sig + c->prm.nsig);
    pnr::Call call(c, "tracker tables");
    auto up = [&call](auto &dst, const auto &src) { // a device buffer of exactly the table's size (PNR_E_HIP without one), and its upload
        if (call.ok()) call.note(dst.alloc(src.size()));
        if (!src.empty()) call.up(dst.get(), src.data(), src.size());
    };
    up(c->d_p, t.p), up(c->d_u, t.u), up(c->d_w0, t.w0), up(c->d_w0cws, t.w0_cws), up(c->d_v, t.v), up(c->d_w, t.w), up(c->d_wcws, t.w_cws);
    up(c->d_tmpl, t.tmpl), up(c->d_corrc, t.corrc), up(c->d_sig, sig), up(c->d_M, t.M), up(c->d_moff, t.moff), up(c->d_rng, t.rng);
    up(c->d_grid, t.grid), up(c->d_axes, t.axes), up(c->d_axes_off, t.axes_off), up(c->d_wd, t.wd), up(c->d_share, t.share_tab), up(c->d_grows, t.grows);
    return call.finish(); // (sig ends here)
}

extern "C" {

const char *pnr_last_error(void) { return pnr::g_err; }

void pnr_default_params(pnr_params *p)
{
    std::memset(p, 0, sizeof(*p));
    p->sig[0] = 2; p->sig[1] = 4; p->sig[2] = 6; // README.md:17
    p->nsig = 3;
    p->somaradius = 0;
    p->tolerance = 5;
    p->znccth = 0.3f;
    p->kappa = 3;
    p->step = 2;
    p->ni = 200;
    p->np = 20;
    p->zdist = 2;
    p->nodepervol = 4;
    p->vol = 1;
    p->Kc = 20.0f;
    p->neff_ratio = 0.8f;
    p->alpha = .5f;
    p->beta = .5f;
    p->C = 500;
    p->rng_seed = 42;
    p->max_trace_count = 5000;
}

static int validate(const pnr_params &p)
{
    PNR_REQUIRE(p.nsig >= 1 && p.nsig <= PNR_MAX_SIGMAS, PNR_E_ARG, "neuritesigmas: need 1..%d sigmas", PNR_MAX_SIGMAS);
    for (int i = 0; i < p.nsig; i++) {
        PNR_REQUIRE(p.sig[i] > 0 && p.sig[i] <= 20, PNR_E_ARG, "neuritesigmas out of range");
        PNR_REQUIRE(i == 0 || p.sig[i] >= p.sig[i - 1], PNR_E_ARG, "neuritesigmas must be sorted ascending");
    }
    // messages follow Advantra_plugin.cpp:317-326
    PNR_REQUIRE(p.somaradius >= 0, PNR_E_ARG, "somaradius out of range");
    PNR_REQUIRE(p.somaradius <= 21, PNR_E_ARG, "somaradius %d too large (Gaussian radius 3*somaradius > 64)", p.somaradius);
    PNR_REQUIRE(p.tolerance >= 0, PNR_E_ARG, "tolerance out of range");
    PNR_REQUIRE(p.znccth >= 0 && p.znccth <= 1, PNR_E_ARG, "znccth out of range");
    PNR_REQUIRE(p.kappa >= 0 && p.kappa <= 5, PNR_E_ARG, "kappa out of range");
    PNR_REQUIRE(p.step >= 1 && p.step <= 8, PNR_E_ARG, "step out of range");
    PNR_REQUIRE(p.ni > 0, PNR_E_ARG, "ni out of range");
    PNR_REQUIRE(p.np > 0 && p.np <= 4096, PNR_E_ARG, "np out of range");
    PNR_REQUIRE(p.zdist >= 1, PNR_E_ARG, "zdist out of range");
    PNR_REQUIRE(p.nodepervol > 2 && p.nodepervol <= 20, PNR_E_ARG, "nodepervol out of range");
    PNR_REQUIRE(p.vol == 1 || p.vol == 5 || p.vol == 9 || p.vol == 11 || p.vol == 19 || p.vol == 27, PNR_E_ARG,
                "vol can be 1,5,9,11,19,27");
    return PNR_OK;
}

int pnr_create(const pnr_params *p, int device, pnr_ctx **out)
{
    PNR_REQUIRE(p && out, PNR_E_ARG, "null argument");
    *out = nullptr;
    int rc = validate(*p);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device: libpnr_hip has no CPU path (MI355X / gfx950 required)");
        return PNR_E_NODEVICE;
    }
    PNR_REQUIRE(device >= 0 && device < ndev, PNR_E_NODEVICE, "device %d not present (%d devices)", device, ndev);
    PNR_HIP(hipSetDevice(device));
    pnr_ctx *c = new pnr_ctx();
    c->prm = *p;
    if (c->prm.max_trace_count <= 0) c->prm.max_trace_count = 5000;
    c->device = device;
    if (hipStreamCreate(&c->own_stream) != hipSuccess) {
        delete c;
        set_error("hipStreamCreate failed");
        return PNR_E_HIP;
    }
    c->stream = c->own_stream;
    rc = load_tables(c, /*is2d*/ false);
    if (!rc && c->d_minmax.alloc(2) != hipSuccess) rc = PNR_E_HIP;
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = PNR_E_HIP;
    if (rc) {
        pnr_destroy(c);
        return rc;
    }
    *out = c;
    return PNR_OK;
}

void pnr_destroy(pnr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    pnr_persistent_destroy(c->job);
    pnr_phased_destroy(c->phased);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (int k = 0; k < pnr_ctx::J8_CHUNKS; k++)
        if (c->j8_ev[k]) (void)hipEventDestroy(c->j8_ev[k]);
    if (c->j8_start) (void)hipEventDestroy(c->j8_start);
    c->resolve_timers();
    for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c; // (every device and pinned buffer is a member that frees itself)
}

int pnr_set_stream(pnr_ctx *c, void *s)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_HIP(hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return PNR_OK;
}

int pnr_synchronize(pnr_ctx *c)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_HIP(hipStreamSynchronize(c->stream));
    return PNR_OK;
}

// a new or changed volume: nothing computed from the old one stays valid
static void invalidate_pipeline(pnr_ctx *c)
{
    c->have_j8 = false;
    c->have_v = c->have_scale = false;
    c->frangi_pruned = false;
    c->seeds.clear();
    c->have_soma = false;
}

static int set_dims(pnr_ctx *c, int64_t w, int64_t h, int64_t l)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    // P == 1 takes the reference's frangi2d / 2-D tracker branch (Advantra_plugin.cpp:2496-2497, :2526)
    PNR_REQUIRE(w >= 2 && h >= 2 && l >= 1, PNR_E_ARG, "volume must be at least 2x2x1");
    PNR_REQUIRE(w <= 1 << 20 && h <= 1 << 20 && l <= 1 << 20 && w * h < (1LL << 31), PNR_E_ARG, "volume extent too large");
    PNR_HIP(hipSetDevice(c->device));
    c->w = w; c->h = h; c->l = l;
    c->N = w * h * l;
    invalidate_pipeline(c);
    if ((l == 1) != c->tab.is2d) { // the tracker tables depend on the dimensionality (Tracker(..., P == 1, ...))
        PNR_HIP(hipDeviceSynchronize());
        const int rc = load_tables(c, l == 1);
        if (rc) return rc;
    }
    return PNR_OK;
}

int pnr_set_volume(pnr_ctx *c, const uint8_t *img, int64_t w, int64_t h, int64_t l)
{
    PNR_REQUIRE(img, PNR_E_ARG, "null image");
    int rc = set_dims(c, w, h, l);
    if (rc) return rc;
    c->d_img = nullptr; // never leave the context pointing at a freed image if the allocation below fails
    pnr::Call call(c, "pnr_set_volume");
    call.note(c->d_img_owned.reserve((size_t)c->N));
    call.up(c->d_img_owned.get(), img, (size_t)c->N);
    if ((rc = call.finish())) return rc;
    c->d_img = c->d_img_owned.get();
    return PNR_OK;
}

int pnr_set_volume_device(pnr_ctx *c, const void *dev_img, int64_t w, int64_t h, int64_t l)
{
    PNR_REQUIRE(dev_img, PNR_E_ARG, "null image");
    int rc = set_dims(c, w, h, l);
    if (rc) return rc;
    c->d_img_owned.reset();
    c->d_img = (const uint8_t *)dev_img;
    return PNR_OK;
}

// pnr_set_volume_u16[_device]: arguments first (a bad one keeps the previous volume), then the dimensions, then the map (volume.hip)
static int set_volume_u16(pnr_ctx *c, const void *img, bool host, int64_t w, int64_t h, int64_t l, int nchan, int channel,
                          const pnr_window *win, int32_t *lo_out, int32_t *hi_out)
{
    PNR_REQUIRE(c && img, PNR_E_ARG, "null argument");
    PNR_REQUIRE(nchan >= 1 && nchan <= (1 << 16), PNR_E_ARG, "nchan = %d outside [1, 65536]", nchan);
    PNR_REQUIRE(channel >= 0 && channel < nchan, PNR_E_ARG, "channel %d outside [0, %d)", channel, nchan);
    PNR_REQUIRE(((uintptr_t)img & 1) == 0, PNR_E_ARG, "16-bit image not 2-byte aligned");
    const pnr_window wd = win ? *win : pnr_window{-1, -1, 0, 0};
    if (wd.lo == -1 && wd.hi == -1) {
        PNR_REQUIRE(wd.sat_lo_ppm >= 0 && wd.sat_hi_ppm >= 0 && (int64_t)wd.sat_lo_ppm + wd.sat_hi_ppm < 1000000, PNR_E_ARG,
                    "saturation %d + %d ppm: each >= 0, together below 1e6", wd.sat_lo_ppm, wd.sat_hi_ppm);
    } else {
        PNR_REQUIRE(wd.lo >= 0 && wd.lo < wd.hi && wd.hi <= 65535, PNR_E_ARG, "window [%d, %d]: need 0 <= lo < hi <= 65535 (or -1, -1)", wd.lo, wd.hi);
        PNR_REQUIRE(wd.sat_lo_ppm == 0 && wd.sat_hi_ppm == 0, PNR_E_ARG, "a fixed window takes no saturation");
    }
    int rc = set_dims(c, w, h, l);
    if (rc) return rc;
    c->d_img = nullptr; // no volume until the map below has succeeded
    const uint16_t *src = (const uint16_t *)img;
    pnr::DevBuf<char> d_up;
    if (host) {
        const size_t bytes = (size_t)c->N * (size_t)nchan * 2;
        if ((rc = pnr::dev_alloc(d_up, bytes, "pnr_set_volume_u16", "for the 16-bit stack"))) return rc;
        pnr::Call call(c, "pnr_set_volume_u16");
        call.up(d_up.get(), img, bytes);
        if (!call.ok()) return call.finish();
        src = (const uint16_t *)d_up.get();
    }
    rc = pnr_volume_u16_run(c, src, nchan, channel, wd, lo_out, hi_out);
    if (d_up) (void)hipStreamSynchronize(c->stream); // (before d_up is freed)
    if (rc) return rc;
    c->d_img = c->d_img_owned.get();
    return PNR_OK;
}

int pnr_set_volume_u16(pnr_ctx *c, const uint16_t *img, int64_t w, int64_t h, int64_t l, int nchan, int channel, const pnr_window *win,
                       int32_t *lo_out, int32_t *hi_out)
{
    return set_volume_u16(c, img, true, w, h, l, nchan, channel, win, lo_out, hi_out);
}

int pnr_set_volume_u16_device(pnr_ctx *c, const void *dev_img, int64_t w, int64_t h, int64_t l, int nchan, int channel,
                              const pnr_window *win, int32_t *lo_out, int32_t *hi_out)
{
    return set_volume_u16(c, dev_img, false, w, h, l, nchan, channel, win, lo_out, hi_out);
}

int pnr_get_volume(pnr_ctx *c, uint8_t *img)
{
    PNR_REQUIRE(c && img, PNR_E_ARG, "null argument");
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "pnr_get_volume: no volume set");
    PNR_HIP(hipSetDevice(c->device));
    pnr::Call call(c, "pnr_get_volume");
    call.down(img, c->d_img, (size_t)c->N);
    return call.finish();
}

// what pnr_set_volume of the new bytes leaves: an owned volume of the same dimensions, no later pipeline state
static void replace_volume(pnr_ctx *c, pnr::DevBuf<uint8_t> &&v)
{
    c->d_img_owned = std::move(v); // (empty while the volume was borrowed: a borrowed volume is never written or freed)
    c->d_img = c->d_img_owned.get();
    invalidate_pipeline(c);
    c->have_graph = false;
}

// pnr_filter_volume: arguments first, then the state; the context changes only after the filtered volume is complete (filter.hip)
int pnr_filter_volume(pnr_ctx *c, const pnr_filter_opts *opts)
{
    PNR_REQUIRE(c && opts, PNR_E_ARG, "null argument");
    PNR_REQUIRE(opts->median == 0 || opts->median == 2 || opts->median == 3, PNR_E_ARG, "pnr_filter_volume: median = %d, not 0, 2 or 3", opts->median);
    PNR_REQUIRE(opts->tophat_r >= 0 && opts->tophat_r <= PNR_TOPHAT_MAX_R, PNR_E_ARG, "pnr_filter_volume: tophat_r = %d outside [0, %d]", opts->tophat_r, PNR_TOPHAT_MAX_R);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "pnr_filter_volume: no volume set");
    if (!opts->median && !opts->tophat_r) return PNR_OK;
    PNR_HIP(hipSetDevice(c->device));
    pnr::DevBuf<uint8_t> out;
    const int rc = pnr_filter_run(c, *opts, out);
    if (!rc) replace_volume(c, std::move(out));
    return rc;
}

// pnr_label_components / pnr_despeckle_volume (components.hip): arguments first, then the state
static int components_args(pnr_ctx *c, const char *who, const pnr_components_opts *opts, pnr_components_opts &o)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    o = opts ? *opts : pnr_components_opts{-1, 26, 1};
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, o.thr);
    PNR_REQUIRE(o.connectivity == 6 || o.connectivity == 26, PNR_E_ARG, "%s: connectivity = %d, not 6 or 26", who, o.connectivity);
    PNR_REQUIRE(o.min_size >= 1, PNR_E_ARG, "%s: min_size = %lld must be at least 1", who, (long long)o.min_size);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "%s: no volume set", who);
    PNR_REQUIRE(c->N <= 0xfffffffeLL, PNR_E_ARG, "%s: %lld voxels, at most 2^32 - 2", who, (long long)c->N);
    return PNR_OK;
}

int pnr_label_components(pnr_ctx *c, const pnr_components_opts *opts, pnr_components_info *info, int32_t *label_out, pnr_component *comps, int64_t cap)
{
    static const char *who = "pnr_label_components";
    pnr_components_opts o;
    PNR_REQUIRE(cap >= 0, PNR_E_ARG, "%s: cap = %lld is negative", who, (long long)cap);
    const int rc = components_args(c, who, opts, o);
    if (rc) return rc;
    PNR_HIP(hipSetDevice(c->device));
    return pnr_components_run(c, who, o, info, label_out, comps, cap, nullptr);
}

int pnr_despeckle_volume(pnr_ctx *c, const pnr_components_opts *opts, pnr_components_info *info)
{
    static const char *who = "pnr_despeckle_volume";
    pnr_components_opts o;
    int rc = components_args(c, who, opts, o);
    if (rc) return rc;
    PNR_HIP(hipSetDevice(c->device));
    if (o.min_size == 1) return info ? pnr_components_run(c, who, o, info, nullptr, nullptr, 0, nullptr) : PNR_OK; // nothing can be dropped
    pnr::DevBuf<uint8_t> out;
    if (!(rc = pnr_components_run(c, who, o, info, nullptr, nullptr, 0, &out))) replace_volume(c, std::move(out));
    return rc;
}

// pnr_distance_transform (edt.hip): arguments first, then the state; the pipeline state of the context is neither needed nor touched
int pnr_distance_transform(pnr_ctx *c, const pnr_edt_opts *opts, pnr_edt_info *info, float *d2_out, const float *xyz, int64_t n, float *d2_at)
{
    static const char *who = "pnr_distance_transform";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_edt_opts o = opts ? *opts : pnr_edt_opts{-1, 64};
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, o.thr);
    PNR_REQUIRE(o.rmax >= 1 && o.rmax <= PNR_EDT_MAX_R, PNR_E_ARG, "%s: rmax = %d outside [1, %d]", who, o.rmax, PNR_EDT_MAX_R);
    PNR_REQUIRE(n >= 0 && n <= PNR_RADIUS_MAX_N && (n == 0 || (xyz && d2_at)), PNR_E_ARG, "%s: n = %lld positions (at most 2^28) need xyz and d2_at", who, (long long)n);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "%s: no volume set", who);
    PNR_REQUIRE(c->N <= 0xfffffffeLL, PNR_E_ARG, "%s: %lld voxels, at most 2^32 - 2", who, (long long)c->N);
    PNR_HIP(hipSetDevice(c->device));
    return pnr_edt_run(c, who, o, info, d2_out, xyz, n, d2_at);
}

// pnr_skeletonize (thin.hip): arguments first, then the state; the pipeline state of the context is neither needed nor touched
int pnr_skeletonize(pnr_ctx *c, const pnr_thin_opts *opts, pnr_thin_info *info, uint8_t *skel_out, int64_t *vox_out, uint8_t *deg_out, int64_t cap)
{
    static const char *who = "pnr_skeletonize";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_thin_opts o = opts ? *opts : pnr_thin_opts{-1, 0};
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, o.thr);
    PNR_REQUIRE(o.max_rounds >= 0, PNR_E_ARG, "%s: max_rounds = %d is negative", who, o.max_rounds);
    PNR_REQUIRE(cap >= 0, PNR_E_ARG, "%s: cap = %lld is negative", who, (long long)cap);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "%s: no volume set", who);
    PNR_REQUIRE(c->N <= 0xfffffffeLL, PNR_E_ARG, "%s: %lld voxels, at most 2^32 - 2", who, (long long)c->N);
    PNR_HIP(hipSetDevice(c->device));
    return pnr_thin_run(c, who, o, info, skel_out, vox_out, deg_out, cap);
}

// pnr_skeleton_forest: pure host.  Kruskal over the 26-adjacent pairs under (len2, lo, hi); every key is distinct, so the forest is unique
int pnr_skeleton_forest(const int64_t *vox, int64_t k, int64_t w, int64_t h, int64_t l, pnr_bridge *edges_out, int64_t cap, int64_t *n_edges)
{
    static const char *who = "pnr_skeleton_forest";
    PNR_REQUIRE(n_edges, PNR_E_ARG, "null argument");
    PNR_REQUIRE(k >= 0 && k <= 0x7fffffffLL && (k == 0 || vox), PNR_E_ARG, "%s: k = %lld voxels (0 to 2^31 - 1) need vox", who, (long long)k);
    PNR_REQUIRE(w >= 1 && h >= 1 && l >= 1 && w < (1LL << 31) && h < (1LL << 31) && l < (1LL << 31) && w * h <= (1LL << 40) / l, PNR_E_ARG, "%s: grid %lld x %lld x %lld", who,
                (long long)w, (long long)h, (long long)l);
    PNR_REQUIRE(cap >= 0, PNR_E_ARG, "%s: cap = %lld is negative", who, (long long)cap);
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
    *n_edges = (int64_t)kept.size();
    const size_t fill = edges_out ? (size_t)std::min<int64_t>(cap, *n_edges) : 0;
    for (size_t i = 0; i < fill; i++) edges_out[i] = pnr_bridge{kept[i].lo, kept[i].hi, sqrtf((float)kept[i].len2)};
    return PNR_OK;
}

// pnr_geodesic_distance (geodesic.hip): arguments first, then the state; the pipeline state of the context is neither needed nor touched
int pnr_geodesic_distance(pnr_ctx *c, const float *src_xyz, const int32_t *src_label, int64_t n_src, const pnr_geo_opts *opts, pnr_geo_info *info, uint32_t *d_out,
                          int32_t *label_out, const float *at_xyz, int64_t m, uint32_t *d_at, int32_t *label_at, int32_t path_cap, int32_t *path_len, int64_t *path_vox)
{
    static const char *who = "pnr_geodesic_distance";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_geo_opts o = opts ? *opts : pnr_geo_opts{0, 0x7fffffffu, nullptr};
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, o.thr);
    PNR_REQUIRE(o.dmax >= 1 && o.dmax <= 0x7fffffffu, PNR_E_ARG, "%s: dmax = %u outside [1, 2^31 - 1]", who, o.dmax);
    for (int v = 0; o.cost && v < 256; v++) PNR_REQUIRE(o.cost[v] >= 1, PNR_E_ARG, "%s: cost[%d] = 0, every entry is at least 1", who, v);
    PNR_REQUIRE(n_src >= 0 && n_src <= PNR_RADIUS_MAX_N && (n_src == 0 || src_xyz), PNR_E_ARG, "%s: n_src = %lld sources (at most 2^28) need src_xyz", who, (long long)n_src);
    for (int64_t i = 0; src_label && i < n_src; i++) PNR_REQUIRE(src_label[i] >= 0, PNR_E_ARG, "%s: label[%lld] = %d is negative", who, (long long)i, src_label[i]);
    PNR_REQUIRE(path_cap >= 0 && path_cap <= PNR_GEO_MAX_PATH, PNR_E_ARG, "%s: path_cap = %d outside [0, %d]", who, path_cap, PNR_GEO_MAX_PATH);
    PNR_REQUIRE(m >= 0 && m <= PNR_RADIUS_MAX_N && (m == 0 || (at_xyz && (d_at || label_at || path_cap > 0))), PNR_E_ARG,
                "%s: m = %lld targets (at most 2^28) need at_xyz and one of d_at, label_at and path_cap > 0", who, (long long)m);
    PNR_REQUIRE(m == 0 || path_cap == 0 || (path_len && path_vox), PNR_E_ARG, "%s: path_cap = %d needs path_len and path_vox", who, path_cap);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "%s: no volume set", who);
    PNR_REQUIRE(c->N <= 0xfffffffeLL, PNR_E_ARG, "%s: %lld voxels, at most 2^32 - 2", who, (long long)c->N);
    PNR_HIP(hipSetDevice(c->device));
    return pnr_geodesic_run(c, who, o, pnr_geo_call{src_xyz, src_label, n_src, info, d_out, label_out, at_xyz, m, d_at, label_at, path_cap, path_len, path_vox});
}

// pnr_measure_radii: arguments first, then the state; the pipeline state of the context (Frangi, seeds, graph) is neither needed nor touched
int pnr_measure_radii(pnr_ctx *c, const float *xyz, int64_t n, const pnr_radius_opts *opts, int32_t *k_out, int32_t *thr_used)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_radius_opts o = opts ? *opts : pnr_radius_opts{-1, 50, 32, 1};
    PNR_REQUIRE(o.rmax >= 1 && o.rmax <= PNR_RADIUS_MAX, PNR_E_ARG, "pnr_measure_radii: rmax = %d outside [1, %d]", o.rmax, PNR_RADIUS_MAX);
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "pnr_measure_radii: thr = %d outside [-1, 255]", o.thr);
    PNR_REQUIRE(o.rel_pct >= 0 && o.rel_pct <= 100, PNR_E_ARG, "pnr_measure_radii: rel_pct = %d outside [0, 100]", o.rel_pct);
    PNR_REQUIRE(o.bg_permille >= 0 && o.bg_permille <= 999, PNR_E_ARG, "pnr_measure_radii: bg_permille = %d outside [0, 999]", o.bg_permille);
    PNR_REQUIRE(n >= 0 && n <= PNR_RADIUS_MAX_N && (n == 0 || (xyz && k_out)), PNR_E_ARG, "pnr_measure_radii: n = %lld positions (at most 2^28) need xyz and k_out", (long long)n);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "pnr_measure_radii: no volume set");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_radius_run(c, xyz, n, o, k_out, thr_used);
}

// ---- tree distance (distance.hip): arguments first; neither a volume nor any pipeline state is needed or touched ----
static bool all_finite(const float *v, int64_t count)
{
    for (int64_t i = 0; i < count; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

int pnr_point_segment_distance(pnr_ctx *c, const float *pts, int64_t n, const float *seg_a, const float *seg_b, int64_t m, float *d_out, int32_t *j_out)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(m >= 1 && m <= PNR_DISTANCE_MAX_N && seg_a && seg_b, PNR_E_ARG, "pnr_point_segment_distance: m = %lld segments (1 to 2^22) need seg_a and seg_b", (long long)m);
    PNR_REQUIRE(n >= 0 && n <= PNR_DISTANCE_MAX_N && (n == 0 || (pts && d_out)), PNR_E_ARG, "pnr_point_segment_distance: n = %lld points (at most 2^22) need pts and d_out", (long long)n);
    PNR_REQUIRE(all_finite(seg_a, 3 * m) && all_finite(seg_b, 3 * m) && all_finite(pts, 3 * n), PNR_E_ARG, "pnr_point_segment_distance: a coordinate is not finite");
    if (n == 0) return PNR_OK;
    PNR_HIP(hipSetDevice(c->device));
    return pnr_distance_run(c, pts, n, seg_a, seg_b, m, d_out, j_out);
}

int pnr_tree_sample(const float *xyz, const int32_t *parent, int64_t n, float zscale, float step, float *pts_out, int32_t *owner_out, int64_t cap, int64_t *n_out)
{
    PNR_REQUIRE(n >= 0 && n <= PNR_DISTANCE_MAX_N && (n == 0 || (xyz && parent)) && n_out && cap >= 0, PNR_E_ARG, "pnr_tree_sample: n = %lld nodes (at most 2^22) need xyz, parent and n_out", (long long)n);
    PNR_REQUIRE(std::isfinite(zscale) && zscale > 0.f, PNR_E_ARG, "pnr_tree_sample: zscale = %g must be positive", (double)zscale);
    PNR_REQUIRE(std::isfinite(step) && step >= 0.f, PNR_E_ARG, "pnr_tree_sample: step = %g must not be negative", (double)step);
    return pnr::tree_sample(xyz, parent, n, zscale, step, pts_out, owner_out, cap, n_out);
}

namespace {
// one side of pnr_tree_distance: the sample points with their nodes, and the segments (a = the node, b = its parent or itself)
struct TreeSide {
    std::vector<float> pts, a, b, d;
    std::vector<int32_t> owner;
    int64_t np = 0, n = 0;
};
int tree_side(const char *which, const float *xyz, const int32_t *parent, int64_t n, const pnr_distance_opts &o, TreeSide &s)
{
    PNR_REQUIRE(n >= 1 && n <= PNR_DISTANCE_MAX_N && xyz && parent, PNR_E_ARG, "pnr_tree_distance: tree %s has %lld nodes (1 to 2^22)", which, (long long)n);
    int rc = pnr::tree_sample(xyz, parent, n, o.zscale, o.step, nullptr, nullptr, 0, &s.np);
    if (rc) return rc;
    PNR_REQUIRE(s.np <= PNR_DISTANCE_MAX_N, PNR_E_ARG, "pnr_tree_distance: tree %s has %lld sample points (at most 2^22): raise the step", which, (long long)s.np);
    s.n = n;
    s.pts.resize((size_t)s.np * 3);
    s.owner.resize((size_t)s.np);
    s.d.resize((size_t)s.np);
    if ((rc = pnr::tree_sample(xyz, parent, n, o.zscale, o.step, s.pts.data(), s.owner.data(), s.np, &s.np))) return rc;
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
} // namespace

int pnr_tree_distance(pnr_ctx *c, const float *xyzA, const int32_t *parentA, int64_t nA, const float *xyzB, const int32_t *parentB, int64_t nB,
                      const pnr_distance_opts *opts, pnr_distance_result *result, float *dA_out, int32_t *ownerA_out, int64_t capA, float *dB_out,
                      int32_t *ownerB_out, int64_t capB)
{
    PNR_REQUIRE(c && result, PNR_E_ARG, "null argument");
    const pnr_distance_opts o = opts ? *opts : pnr_distance_opts{1.f, 1.f, 2.f};
    PNR_REQUIRE(std::isfinite(o.zscale) && o.zscale > 0.f, PNR_E_ARG, "pnr_tree_distance: zscale = %g must be positive", (double)o.zscale);
    PNR_REQUIRE(std::isfinite(o.step) && o.step >= 0.f, PNR_E_ARG, "pnr_tree_distance: step = %g must not be negative", (double)o.step);
    PNR_REQUIRE(std::isfinite(o.thr), PNR_E_ARG, "pnr_tree_distance: thr is not finite");
    PNR_REQUIRE(capA >= 0 && capB >= 0, PNR_E_ARG, "pnr_tree_distance: negative capacity");
    TreeSide A, B;
    int rc = tree_side("A", xyzA, parentA, nA, o, A);
    if (!rc) rc = tree_side("B", xyzB, parentB, nB, o, B);
    if (rc) return rc;
    PNR_HIP(hipSetDevice(c->device));
    if ((rc = pnr_distance_run(c, A.pts.data(), A.np, B.a.data(), B.b.data(), B.n, A.d.data(), nullptr))) return rc;
    if ((rc = pnr_distance_run(c, B.pts.data(), B.np, A.a.data(), A.b.data(), A.n, B.d.data(), nullptr))) return rc;
    direction_metrics(A.d, o.thr, result->ab);
    direction_metrics(B.d, o.thr, result->ba);
    result->sd = (result->ab.mean + result->ba.mean) / 2;
    result->ssd = (result->ab.ssd + result->ba.ssd) / 2;
    result->pct = (result->ab.pct + result->ba.pct) / 2;
    result->hausdorff = std::max(result->ab.max, result->ba.max);
    const size_t ka = (size_t)std::min(capA, A.np), kb = (size_t)std::min(capB, B.np);
    if (dA_out) std::memcpy(dA_out, A.d.data(), 4 * ka);
    if (ownerA_out) std::memcpy(ownerA_out, A.owner.data(), 4 * ka);
    if (dB_out) std::memcpy(dB_out, B.d.data(), 4 * kb);
    if (ownerB_out) std::memcpy(ownerB_out, B.owner.data(), 4 * kb);
    return PNR_OK;
}

// ---- joining the forest (join.hip): arguments first; neither a volume nor any pipeline state is needed or touched ----
int pnr_nearest_other(pnr_ctx *c, const float *xyz, const int32_t *label, int64_t n, float *d_out, int32_t *j_out)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(n >= 1 && n <= PNR_JOIN_MAX_N && xyz && label && d_out && j_out, PNR_E_ARG, "pnr_nearest_other: n = %lld points (1 to 2^22) need xyz, label, d_out and j_out", (long long)n);
    PNR_REQUIRE(all_finite(xyz, 3 * n), PNR_E_ARG, "pnr_nearest_other: a coordinate is not finite");
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
    PNR_REQUIRE(std::isfinite(o.zscale) && o.zscale > 0.f, PNR_E_ARG, "pnr_join_trees: zscale = %g must be positive", (double)o.zscale);
    PNR_REQUIRE(std::isfinite(o.gap) && o.gap >= 0.f, PNR_E_ARG, "pnr_join_trees: gap = %g must not be negative", (double)o.gap);
    PNR_REQUIRE(o.root < n, PNR_E_ARG, "pnr_join_trees: root = %d outside [-1, %lld)", o.root, (long long)n);
    PNR_REQUIRE(cap_bridges >= 0 && (cap_bridges == 0 || bridges_out), PNR_E_ARG, "pnr_join_trees: cap_bridges = %lld needs bridges_out", (long long)cap_bridges);
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
    int rc = pnr::join_bridges(c, scaled.data(), parent, n, o.gap, bridges, &trees_in, &c->join_rounds);
    if (rc) return rc;
    if ((rc = pnr::join_reroot(parent, n, bridges.data(), (int64_t)bridges.size(), o.root, parent_out, order_out, comp_out, &trees_out))) return rc;
    *n_bridges = (int64_t)bridges.size();
    if (bridges_out) std::memcpy(bridges_out, bridges.data(), sizeof(pnr_bridge) * (size_t)std::min<int64_t>(cap_bridges, *n_bridges));
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
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, o.thr);
    PNR_REQUIRE(std::isfinite(o.step) && o.step >= 0.f, PNR_E_ARG, "%s: step = %g must not be negative", who, (double)o.step);
    for (int v = 0; o.cost && v < 256; v++) PNR_REQUIRE(o.cost[v] >= 1, PNR_E_ARG, "%s: cost[%d] = 0, every entry is at least 1", who, v);
    PNR_REQUIRE(cap_bridges >= 0 && (cap_bridges == 0 || bridges_out), PNR_E_ARG, "%s: cap_bridges = %lld needs bridges_out", who, (long long)cap_bridges);
    PNR_REQUIRE(cap_path >= 0 && (cap_path == 0 || path_vox), PNR_E_ARG, "%s: cap_path = %lld needs path_vox", who, (long long)cap_path);
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "%s: no volume set", who);
    PNR_REQUIRE(c->N <= 0xfffffffeLL, PNR_E_ARG, "%s: %lld voxels, at most 2^32 - 2", who, (long long)c->N);
    PNR_HIP(hipSetDevice(c->device));
    std::vector<pnr_geo_bridge> bridges;
    std::vector<int64_t> chain;
    const int rc = pnr_geojoin_run(c, xyz, parent, n, o, info, bridges, chain);
    if (rc) return rc;
    *n_bridges = (int64_t)bridges.size();
    *n_path = (int64_t)chain.size();
    if (bridges_out) std::memcpy(bridges_out, bridges.data(), sizeof(pnr_geo_bridge) * (size_t)std::min<int64_t>(cap_bridges, *n_bridges));
    if (path_vox) std::memcpy(path_vox, chain.data(), sizeof(int64_t) * (size_t)std::min<int64_t>(cap_path, *n_path));
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

// ---- rendering the tree (render.hip): arguments first; pnr_render_tree needs no volume, neither call touches the pipeline state ----
static pnr_render_opts default_render_opts(const pnr_render_opts *opts) { return opts ? *opts : pnr_render_opts{1.f, 1.f, 0.f, -1}; }
static int render_grid_ok(const char *who, int64_t w, int64_t h, int64_t l)
{
    const int64_t lim = 0x7fffffffll;
    PNR_REQUIRE(w >= 1 && h >= 1 && l >= 1 && w <= lim && h <= lim && l <= lim && w <= (1ll << 40) / h && w * h <= (1ll << 40) / l, PNR_E_ARG,
                "%s: the grid %lld x %lld x %lld needs sides from 1 and at most 2^40 voxels", who, (long long)w, (long long)h, (long long)l);
    return PNR_OK;
}
static int render_tree_ok(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_render_opts &o)
{
    PNR_REQUIRE(n >= 0 && n <= PNR_RENDER_MAX_N && (n == 0 || (xyz && radius && parent)), PNR_E_ARG, "%s: n = %lld nodes (at most 2^22) need xyz, radius and parent", who, (long long)n);
    PNR_REQUIRE(o.thr >= -1 && o.thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, o.thr);
    return PNR_OK;
}

int pnr_render_tree(pnr_ctx *c, const float *xyz, const float *radius, const int32_t *parent, int64_t n, int64_t w, int64_t h, int64_t l,
                    const pnr_render_opts *opts, int32_t *label_out, uint8_t *mask_out)
{
    static const char *who = "pnr_render_tree";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_render_opts o = default_render_opts(opts);
    int rc = render_tree_ok(who, xyz, radius, parent, n, o);
    if (!rc) rc = render_grid_ok(who, w, h, l);
    pnr::RenderTree t;
    if (!rc) rc = pnr::render_prepare(who, xyz, radius, parent, n, o, t);
    if (rc) return rc;
    PNR_HIP(hipSetDevice(c->device));
    return pnr_render_run(c, who, t, w, h, l, nullptr, 0, label_out, mask_out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int pnr_tree_coverage(pnr_ctx *c, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_render_opts *opts, pnr_coverage *cov,
                      int64_t *seg_vox, int64_t *seg_fg, int64_t *seg_sum, uint8_t *mask_out, uint8_t *residual_out)
{
    static const char *who = "pnr_tree_coverage";
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    const pnr_render_opts o = default_render_opts(opts);
    int rc = render_tree_ok(who, xyz, radius, parent, n, o);
    pnr::RenderTree t;
    if (!rc) rc = pnr::render_prepare(who, xyz, radius, parent, n, o, t);
    if (rc) return rc;
    PNR_REQUIRE(c->d_img, PNR_E_STATE, "pnr_tree_coverage: no volume set");
    PNR_HIP(hipSetDevice(c->device));
    pnr_coverage r;
    std::memset(&r, 0, sizeof(r));
    if ((rc = pnr_render_run(c, who, t, c->w, c->h, c->l, c->d_img, o.thr, nullptr, mask_out, residual_out, &r, seg_vox, seg_fg, seg_sum))) return rc;
    r.covered = r.n_fg ? (double)r.n_both / (double)r.n_fg : 0.0;
    r.on_signal = r.n_tree ? (double)r.n_both / (double)r.n_tree : 0.0;
    r.covered_intensity = r.sum_fg ? (double)r.sum_both / (double)r.sum_fg : 0.0;
    if (cov) *cov = r;
    return PNR_OK;
}

// test tap (pnr_hip_test.h): the work items of a render, pure host
int pnr_render_items(const float *xyz, const float *radius, const int32_t *parent, int64_t n, int64_t w, int64_t h, int64_t l, const pnr_render_opts *opts,
                     int64_t piece, int64_t box, int64_t *items_out, int64_t cap, int64_t *count)
{
    static const char *who = "pnr_render_items";
    PNR_REQUIRE(count && piece >= 0 && box >= 0 && (cap <= 0 || items_out), PNR_E_ARG, "%s: piece and box (not negative) need a count, and items_out for cap = %lld", who, (long long)cap);
    const pnr_render_opts o = default_render_opts(opts);
    int rc = render_tree_ok(who, xyz, radius, parent, n, o);
    if (!rc) rc = render_grid_ok(who, w, h, l);
    pnr::RenderTree t;
    if (!rc) rc = pnr::render_prepare(who, xyz, radius, parent, n, o, t);
    if (rc) return rc;
    int64_t k = 0;
    pnr::render_items(t, w, h, l, piece, box, [&](const pnr::RenderItem &it) {
        if (k < cap) {
            const int64_t row[7] = {it.seg, it.x0, it.y0, it.z0, it.x1, it.y1, it.z1};
            std::copy(row, row + 7, items_out + 7 * k);
        }
        k++;
        return true;
    });
    *count = k;
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
    int64_t k = 0;
    pnr::pair_tiles(n, m, split, budget, [&](const pnr::PairTile &t) {
        if (k < cap) {
            const int64_t row[7] = {t.p0, t.p1, t.s0, t.s1, t.split, t.gx, t.gy};
            std::copy(row, row + 7, tiles + 7 * k);
        }
        k++;
        return true;
    });
    *count = k;
    return PNR_OK;
}

int pnr_frangi(pnr_ctx *c, float *Jmin, float *Jmax)
{
    PNR_REQUIRE(c && c->d_img, PNR_E_STATE, "pnr_frangi: no volume set");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_frangi_run(c, Jmin, Jmax);
}

int pnr_frangi_slab(pnr_ctx *c, int64_t z_keep0, int64_t z_keep1, float *Jmin, float *Jmax)
{
    PNR_REQUIRE(c && c->d_img, PNR_E_STATE, "pnr_frangi_slab: no volume set");
    PNR_REQUIRE(c->l > 1, PNR_E_ARG, "pnr_frangi_slab: a single-slice stack has no z-slabs");
    PNR_REQUIRE(z_keep0 >= 0 && z_keep0 < z_keep1 && z_keep1 <= c->l, PNR_E_ARG, "kept planes [%lld,%lld) outside [0,%lld)", (long long)z_keep0,
                (long long)z_keep1, (long long)c->l);
    PNR_HIP(hipSetDevice(c->device));
    return pnr_frangi_run_range(c, z_keep0, z_keep1, /*finish*/ false, Jmin, Jmax);
}

int pnr_quantise_j8(pnr_ctx *c, float Jmin, float Jmax)
{
    PNR_REQUIRE(c && c->d_img, PNR_E_STATE, "pnr_quantise_j8: no volume set");
    PNR_HIP(hipSetDevice(c->device));
    if (c->frangi_pruned && !(Jmin == 0.f && Jmax >= c->Jmax_run)) {
        // the last run skipped the solver below the first J8 level of ITS extremes (Jmin = 0, Jmax at least its own maximum): the
        // global extremes of a sharded stack satisfy that; anything else needs the exact response
        c->frangi_exact_once = true;
        c->frangi_recomputes++;
        if (c->opt.trace_timing || c->opt.seed_timing) fprintf(stderr, "[pnr frangi] pnr_quantise_j8(%g, %g): extremes the pruned run did not assume -- exact re-run of every scale\n", Jmin, Jmax);
        const int rc = pnr_frangi_run_range(c, c->fr_zs0, c->fr_zs1, false, nullptr, nullptr);
        if (rc) return rc;
    }
    return pnr_j8_run(c, Jmin, Jmax);
}

int pnr_get_frangi(pnr_ctx *c, float *J, uint8_t *J8, uint8_t *Vx, uint8_t *Vy, uint8_t *Vz)
{
    PNR_REQUIRE(c && c->have_j8 && c->d_J.get(), PNR_E_STATE, "pnr_get_frangi: run pnr_frangi first");
    const size_t n = (size_t)c->N;
    int rc = PNR_OK;
    if ((J || Vx || Vy || Vz) && c->frangi_pruned) {
        // the last run skipped the solver where the response could not reach J8 = 1 (option frangi_prune): J8, the extremes and the
        // seeds are exact, the f32 J and the winning scale of J8 = 0 voxels are not -- recompute without the shortcut, same extremes
        const float jmin = c->Jmin, jmax = c->Jmax;
        c->frangi_exact_once = true;
        c->frangi_recomputes++;
        if (c->opt.trace_timing || c->opt.seed_timing) fprintf(stderr, "[pnr frangi] pnr_get_frangi: J / V asked for after a pruned run -- exact re-run of every scale\n");
        rc = pnr_frangi_run_range(c, c->fr_zs0, c->fr_zs1, false, nullptr, nullptr);
        if (!rc) rc = pnr_j8_run(c, jmin, jmax);
        if (rc) return rc;
    }
    if (Vx || Vy || Vz) rc = pnr_frangi_materialise_v(c); // the pipeline itself only needs the directions at the seeds
    if (rc) return rc;
    pnr::Call call(c, "pnr_get_frangi");
    if (J) call.down(J, c->d_J.get(), n);
    if (J8) call.down(J8, c->d_J8.get(), n);
    if (Vx) call.down(Vx, c->d_Vx.get(), n);
    if (Vy) call.down(Vy, c->d_Vy.get(), n);
    if (Vz) call.down(Vz, c->d_Vz.get(), n);
    return call.finish();
}

int pnr_gaussian(pnr_ctx *c, float sig, float *F)
{
    PNR_REQUIRE(c && c->d_img && F, PNR_E_STATE, "pnr_gaussian: no volume set");
    PNR_REQUIRE(sig > 0, PNR_E_ARG, "sigma must be positive");
    int rc = pnr_ensure_frangi_buffers(c);
    if (!rc) rc = pnr_ensure_tmpA(c);
    if (rc) return rc;
    rc = pnr_gaussian_run(c, sig, c->d_tmpA.get());
    if (rc) return rc;
    pnr::Call call(c, "pnr_gaussian");
    call.down(F, c->d_tmpA.get(), (size_t)c->N);
    return call.finish();
}

int pnr_hessian(pnr_ctx *c, float sig, float *Dzz, float *Dyy, float *Dyz, float *Dxx, float *Dxy, float *Dxz)
{
    PNR_REQUIRE(c && c->d_img, PNR_E_STATE, "pnr_hessian: no volume set");
    PNR_REQUIRE(c->l > 1, PNR_E_ARG, "pnr_hessian taps the 3-D Hessian: not defined for a single-slice stack");
    PNR_REQUIRE(sig > 0, PNR_E_ARG, "sigma must be positive");
    int rc = pnr_ensure_frangi_buffers(c);
    if (rc) return rc;
    pnr::CallBuf buf; // the six volumes (freed when the call returns)
    pnr::Part<float> part[6];
    for (auto &p : part) p = buf.add<float>((size_t)c->N);
    if ((rc = buf.alloc("pnr_hessian"))) return rc;
    float *d[6];
    for (int k = 0; k < 6; k++) d[k] = part[k];
    rc = pnr_hessian_run(c, sig, d);
    float *hst[6] = {Dzz, Dyy, Dyz, Dxx, Dxy, Dxz};
    pnr::Call call(c, "pnr_hessian");
    for (int k = 0; k < 6 && !rc; k++)
        if (hst[k]) call.down(hst[k], part[k]);
    if (!rc) rc = call.finish();
    c->have_j8 = false; // tmp buffers were reused
    return rc;
}

int pnr_set_j8_v(pnr_ctx *c, const uint8_t *J8, const uint8_t *Vx, const uint8_t *Vy, const uint8_t *Vz)
{
    PNR_REQUIRE(c && c->N > 0, PNR_E_STATE, "pnr_set_j8_v: set a volume first (for the dimensions)");
    PNR_REQUIRE(J8 && Vx && Vy && Vz, PNR_E_ARG, "null argument");
    int rc = pnr_ensure_frangi_buffers(c);
    if (!rc) rc = pnr_ensure_v(c);
    if (rc) return rc;
    const size_t n = (size_t)c->N;
    pnr::Call call(c, "pnr_set_j8_v");
    call.up(c->d_J8.get(), J8, n);
    call.up(c->d_Vx.get(), Vx, n);
    call.up(c->d_Vy.get(), Vy, n);
    call.up(c->d_Vz.get(), Vz, n);
    if ((rc = call.finish())) return rc;
    c->have_j8 = true;
    c->have_v = true;
    c->have_scale = false;
    c->frangi_pruned = false; // what is in HBM now is the caller's, not a run of pnr_frangi
    return PNR_OK;
}

int pnr_extract_seeds_range(pnr_ctx *c, int64_t z0, int64_t z1, const pnr_seed **seeds, int64_t *n)
{
    PNR_REQUIRE(c && seeds && n, PNR_E_ARG, "null argument");
    PNR_HIP(hipSetDevice(c->device));
    int rc = pnr_seeds_run(c, z0, z1);
    if (rc) return rc;
    *seeds = c->seeds.data();
    *n = (int64_t)c->seeds.size();
    return PNR_OK;
}

int pnr_extract_seeds(pnr_ctx *c, const pnr_seed **seeds, int64_t *n)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    return pnr_extract_seeds_range(c, 0, c->l, seeds, n);
}

int pnr_seed_handover(pnr_ctx *c, int64_t z0, int64_t z1, int32_t *vmin, int32_t *vmax, int64_t *ltot, int64_t *key_off, int64_t *keys,
                      int64_t cap_keys, int64_t *n_keys, uint8_t *layers, int32_t *restored)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_seed_handover_run(c, z0, z1, vmin, vmax, ltot, key_off, keys, cap_keys, n_keys, layers, restored);
}

int pnr_phased_likelihood(pnr_ctx *c, int64_t nt, const float *poses, const float *centroids, const int32_t *modes, float *corr,
                          int32_t *uidx, int32_t *cmap, int32_t *flags, int32_t *info)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(nt >= 1, PNR_E_ARG, "pnr_phased_likelihood: bad number of traces");
    PNR_REQUIRE(poses && centroids && modes, PNR_E_ARG, "null argument");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_phased_likelihood_run(c, nt, poses, centroids, modes, corr, uidx, cmap, flags, info);
}

int pnr_phased_decide(pnr_ctx *c, int64_t nt, const pnr_phd_in *in, pnr_phd_out *out)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(nt >= 1, PNR_E_ARG, "pnr_phased_decide: bad number of traces");
    PNR_REQUIRE(in && out && in->flags && in->seeds && in->part && in->prior && in->idxres && in->xcs && in->corr && in->cmap, PNR_E_ARG, "null argument");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_phased_decide_run(c, nt, in, out);
}

int pnr_zncc_batch(pnr_ctx *c, const float *pos_dir, int64_t n, float *corr, float *sig)
{
    PNR_REQUIRE(c && (n == 0 || (pos_dir && corr)), PNR_E_ARG, "null argument");
    PNR_REQUIRE(n >= 0, PNR_E_ARG, "negative count");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_zncc_run(c, pos_dir, n, corr, sig);
}

// the three steps of the seed filter (Advantra_plugin.cpp:2561-2586); score_only / presorted let several GPUs score their own
// seeds and sort the merged list
static int seed_filter(pnr_ctx *c, pnr_seed *seeds, int64_t n, int64_t *n_out, bool score, bool sort)
{
    PNR_REQUIRE(c && n_out && (n == 0 || seeds), PNR_E_ARG, "null argument");
    *n_out = 0;
    if (n == 0) return PNR_OK;
    if (score && c->prm.somaradius > 0) { // seeds inside a soma are dropped before they are scored (:2561-2564)
        PNR_REQUIRE(c->have_soma, PNR_E_STATE, "somaradius > 0: call pnr_soma before the seeds are filtered");
        int64_t m = 0;
        for (int64_t i = 0; i < n; i++) {
            const int64_t j = (int64_t)(int)std::round(seeds[i].z) * c->w * c->h + (int64_t)(int)std::round(seeds[i].y) * c->w + (int)std::round(seeds[i].x);
            if (c->soma_map.find(j) == c->soma_map.end()) seeds[m++] = seeds[i];
        }
        n = m;
        if (n == 0) return PNR_OK;
    }
    if (score) {
        std::vector<float> pd((size_t)n * 6), corr((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            float *q = &pd[(size_t)i * 6];
            q[0] = seeds[i].x; q[1] = seeds[i].y; q[2] = seeds[i].z;
            q[3] = seeds[i].vx; q[4] = seeds[i].vy; q[5] = seeds[i].vz;
        }
        int rc = pnr_zncc_batch(c, pd.data(), n, corr.data(), nullptr);
        if (rc) return rc;
        for (int64_t i = 0; i < n; i++) seeds[i].corr = corr[i];
    }
    std::vector<pnr_seed> kept;
    for (int64_t i = 0; i < n; i++)
        if (!(seeds[i].corr < c->prm.znccth)) kept.push_back(seeds[i]); // erase if corr < znccth (:2571)
    std::vector<int64_t> order(kept.size());
    std::iota(order.begin(), order.end(), 0);
    // std::sort with CompareSeedCorr is unstable in the reference; ties are broken by original index here
    if (sort) std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return kept[a].corr > kept[b].corr; });
    for (size_t i = 0; i < order.size(); i++) seeds[i] = kept[order[i]];
    *n_out = (int64_t)kept.size();
    return PNR_OK;
}

int pnr_score_filter_sort_seeds(pnr_ctx *c, pnr_seed *seeds, int64_t n, int64_t *n_out) { return seed_filter(c, seeds, n, n_out, true, true); }
int pnr_score_filter_seeds(pnr_ctx *c, pnr_seed *seeds, int64_t n, int64_t *n_out) { return seed_filter(c, seeds, n, n_out, true, false); }
int pnr_sort_seeds(pnr_ctx *c, pnr_seed *seeds, int64_t n, int64_t *n_out) { return seed_filter(c, seeds, n, n_out, false, true); }

int pnr_trace_batch(pnr_ctx *c, const pnr_seed *seeds, int64_t n, int32_t *T, int32_t *stop, pnr_xest *xc, int dbg_iters,
                    float *xfilt, int32_t *idxres, float *neff)
{
    PNR_REQUIRE(c && (n == 0 || (seeds && T && stop && xc)), PNR_E_ARG, "null argument");
    PNR_REQUIRE(n >= 0, PNR_E_ARG, "negative count");
    PNR_HIP(hipSetDevice(c->device));
    return pnr_trace_run(c, seeds, n, T, stop, xc, dbg_iters, xfilt, idxres, neff, /*use_density*/ 0);
}

// ---- soma path ---------------------------------------------------------------------------
int pnr_soma(pnr_ctx *c, uint8_t *E8_out, int32_t *threshold, int64_t *n_soma)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_HIP(hipSetDevice(c->device));
    int rc = pnr_soma_run(c, E8_out, threshold);
    if (rc) return rc;
    if (n_soma) *n_soma = (int64_t)c->soma_nodes.size();
    return PNR_OK;
}

int pnr_get_soma(pnr_ctx *c, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int64_t *vox, int32_t *lab, int64_t cap_vox, int64_t *n_vox)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(c->have_soma, PNR_E_STATE, "pnr_soma has not run");
    if (n_nodes) *n_nodes = (int64_t)c->soma_nodes.size();
    if (n_vox) *n_vox = (int64_t)c->soma_vox.size();
    if (nodes) std::memcpy(nodes, c->soma_nodes.data(), sizeof(pnr_node) * (size_t)std::min<int64_t>(cap_nodes, (int64_t)c->soma_nodes.size()));
    const size_t m = (size_t)std::min<int64_t>(cap_vox, (int64_t)c->soma_vox.size());
    if (vox) std::memcpy(vox, c->soma_vox.data(), 8 * m);
    if (lab) std::memcpy(lab, c->soma_lab.data(), 4 * m);
    return PNR_OK;
}

// ---- host replay ------------------------------------------------------------------------
// a node graph into the caller's buffers: the counts, and as much of either array as its capacity holds
static int put_graph(const std::vector<pnr_node> &gn, const std::vector<int32_t> &gl, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links,
                     int64_t cap_links, int64_t *n_links)
{
    *n_nodes = (int64_t)gn.size();
    *n_links = (int64_t)gl.size() / 2;
    if (nodes) std::memcpy(nodes, gn.data(), sizeof(pnr_node) * (size_t)std::min<int64_t>(cap_nodes, *n_nodes));
    if (links) std::memcpy(links, gl.data(), 8 * (size_t)std::min<int64_t>(cap_links, *n_links));
    return PNR_OK;
}
int pnr_replay_traces_ctx(pnr_ctx *c, const pnr_seed *seeds, int64_t n, const int32_t *T, const pnr_xest *xc, pnr_node *nodes,
                          int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used)
{
    PNR_REQUIRE(c && n_nodes && n_links && (n == 0 || (seeds && T && xc)), PNR_E_ARG, "null argument");
    PNR_REQUIRE(c->w > 0, PNR_E_STATE, "no volume set");
    PNR_REQUIRE(c->prm.somaradius == 0 || c->have_soma, PNR_E_STATE, "somaradius > 0: call pnr_soma first");
    pnr::Replayer r(c->prm, c->w, c->h, c->l);
    r.set_soma(&c->soma_map, c->soma_nodes);
    r.add(seeds, n, T, xc);
    if (n_traces_used) *n_traces_used = r.trace_count;
    return put_graph(r.nodes, r.links, nodes, cap_nodes, n_nodes, links, cap_links, n_links);
}

int pnr_replay_traces(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n,
                      const int32_t *T, const pnr_xest *xc, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes,
                      int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used)
{
    PNR_REQUIRE(p && n_nodes && n_links && (n == 0 || (seeds && T && xc)), PNR_E_ARG, "null argument");
    PNR_REQUIRE(w > 0 && h > 0 && l > 0, PNR_E_ARG, "bad dimensions");
    pnr::Replayer r(*p, w, h, l);
    r.add(seeds, n, T, xc);
    if (n_traces_used) *n_traces_used = r.trace_count;
    return put_graph(r.nodes, r.links, nodes, cap_nodes, n_nodes, links, cap_links, n_links);
}

// the graph of the last pnr_trace_replay / pnr_trace_replay_sharded stays in the context (pnr_get_graph): a caller whose buffers
// were too small fetches it again instead of tracing again
static int store_graph(pnr_ctx *c, pnr::Replayer &r, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                       int64_t *n_links, int64_t *n_traces_used)
{
    c->graph_nodes.swap(r.nodes);
    c->graph_links.swap(r.links);
    c->graph_traces = r.trace_count;
    c->have_graph = true;
    if (n_traces_used) *n_traces_used = c->graph_traces;
    return put_graph(c->graph_nodes, c->graph_links, nodes, cap_nodes, n_nodes, links, cap_links, n_links);
}

int pnr_get_graph(pnr_ctx *c, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links)
{
    PNR_REQUIRE(c && n_nodes && n_links, PNR_E_ARG, "null argument");
    PNR_REQUIRE(c->have_graph, PNR_E_STATE, "no node graph: pnr_trace_replay has not run");
    return put_graph(c->graph_nodes, c->graph_links, nodes, cap_nodes, n_nodes, links, cap_links, n_links);
}

int pnr_get_trace_log(pnr_ctx *c, int32_t *rec, int64_t cap, int64_t *n)
{
    PNR_REQUIRE(c && n, PNR_E_ARG, "null argument");
    PNR_REQUIRE(c->have_graph, PNR_E_STATE, "no node graph: pnr_trace_replay has not run");
    *n = (int64_t)c->graph_log.size() / 5;
    if (rec) std::memcpy(rec, c->graph_log.data(), 20 * (size_t)std::min<int64_t>(cap, *n));
    return PNR_OK;
}

static int trace_replay_impl(pnr_ctx *c, const pnr_seed *seeds, int64_t n, int64_t first_batch, const pnr::ShardSpec &sh, pnr_node *nodes,
                             int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used,
                             int64_t *n_iterations)
{
    PNR_REQUIRE(c && n_nodes && n_links && (n == 0 || seeds), PNR_E_ARG, "null argument");
    const int ni = c->prm.ni;
    // Sharded: a rank that fails here, before its scheduler runs, still owes the other ranks the exchange they are about to enter
    // (include/pnr_hip.h: "a rank that fails says so in one last exchange") -- one block with the abort word set.  n == 0 is the
    // same on every rank and exchanges nothing.
    auto prepare = [&]() -> int {
        PNR_REQUIRE(c->d_img, PNR_E_STATE, "no volume set");
        PNR_HIP(hipSetDevice(c->device));
        PNR_REQUIRE(c->prm.somaradius == 0 || c->have_soma, PNR_E_STATE, "somaradius > 0: call pnr_soma first");
        PNR_REQUIRE((c->smc_driver == 0 && !c->opt.replay_batches) || sh.world <= 1, PNR_E_STATE,
                    "sharded tracing needs the phased driver with the streaming scheduler");
        return pnr_density_reset(c);
    };
    c->have_graph = false;
    c->graph_log.clear();
    int rc = prepare();
    if (rc) {
        if (n > 0) pnr::abort_exchange(sh, ni);
        return rc;
    }
    pnr::Replayer r(c->prm, c->w, c->h, c->l);
    r.set_soma(&c->soma_map, c->soma_nodes);
    std::vector<pnr::Replayer::TraceEnd> ends;
    if (c->opt.trace_log) r.log = &ends;
    int64_t iters = 0;
    // phased driver: a window of trace slots refilled as traces stop (smc_phased.hip); `first_batch` has no meaning there
    const bool streaming = c->smc_driver == 0 && !c->opt.replay_batches;
    if (streaming) {
        rc = pnr_trace_replay_stream(c, seeds, n, r, sh, &iters);
        if (rc) return rc;
        n = 0; // nothing left for the batch loop below
    }
    // persistent driver: strictly sequential seed-rank batches (128, 256, ... 1024 seeds): the freshest map a batch scheme can
    // have.  (Several batches in flight on separate streams were slower: they must be collected in rank order, so the in-flight
    // count collapses behind every slow batch, and a staler map costs iterations.)
    int64_t batch = first_batch > 0 ? first_batch : 128;
    const int64_t growth_pct = std::max(100, c->opt.batch_growth);
    const int64_t batch_max = std::max(1, c->opt.batch_max);
    std::vector<pnr_seed> bs;
    std::vector<int32_t> T, stop;
    std::vector<pnr_xest> xc;
    for (int64_t next = 0; next < n && !r.stopped;) {
        const int64_t i1 = std::min(n, next + std::min(batch, batch_max));
        bs.clear();
        for (int64_t i = next; i < i1; i++) // a seed on a saturated voxel is skipped by the replay whatever its traces are: not launched
            if (!r.seed_saturated(seeds[i])) bs.push_back(seeds[i]);
        next = i1;
        if (batch < batch_max) batch = std::max<int64_t>(batch + 1, batch * growth_pct / 100);
        const int64_t m = (int64_t)bs.size();
        T.assign((size_t)(2 * m), 0);
        stop.assign((size_t)(2 * m), 0);
        xc.resize((size_t)(2 * m) * ni);
        rc = pnr_trace_run(c, bs.data(), m, T.data(), stop.data(), xc.data(), 0, nullptr, nullptr, nullptr, /*use_density*/ 1);
        if (rc) return rc;
        int64_t bi = 0, bmax = 0;
        for (int64_t j = 0; j < 2 * m; j++) {
            const int64_t e = std::min<int64_t>(T[(size_t)j] + 1, ni);
            bi += e;
            bmax = std::max(bmax, e);
        }
        iters += bi;
        if (c->opt.trace_timing)
            fprintf(stderr, "[pnr trace] batch of %lld seeds launched: %lld iterations, longest trace %lld, nodes so far %zu\n", (long long)m,
                    (long long)bi, (long long)bmax, r.nodes.size());
        r.touched.clear();
        r.log_base = (int64_t)ends.size() / 2; // (batch mode: rank among the launched seeds)
        r.add(bs.data(), m, T.data(), xc.data());
        rc = pnr_density_update(c, r);
        if (rc) return rc;
    }
    for (const auto &e : ends) c->graph_log.insert(c->graph_log.end(), {e.seed, e.dir, e.ti_limit, e.reason, e.value});
    if (n_iterations) *n_iterations = iters;
    return store_graph(c, r, nodes, cap_nodes, n_nodes, links, cap_links, n_links, n_traces_used);
}

// Trace + replay with early DENSITY stops (the production form of the trace loop, Advantra_plugin.cpp:2658-2710).
// Tracing every seed to its map-free end wastes most GPU iterations: in the reference a trace stops as
// soon as it runs into voxels that earlier traces already filled (DENSITY stop, tracker.cpp:855,870-882),
// and a seed on a filled voxel is never traced (:2669-2670).  The density map produced by the replay of
// lower-ranked seeds is kept on the GPU; the kernel ends a trace at the first iteration whose centroid
// voxel is already saturated in that (stale) map.  A stale map only under-counts, so a trace is never cut
// earlier than the sequential reference would cut it, and the replay -- which applies the true map --
// produces exactly the same nodes and links as the one-shot form.
int pnr_trace_replay(pnr_ctx *c, const pnr_seed *seeds, int64_t n, int64_t first_batch, pnr_node *nodes, int64_t cap_nodes,
                     int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used,
                     int64_t *n_iterations)
{
    return trace_replay_impl(c, seeds, n, first_batch, pnr::ShardSpec{}, nodes, cap_nodes, n_nodes, links, cap_links, n_links, n_traces_used, n_iterations);
}

int pnr_trace_replay_sharded(pnr_ctx *c, const pnr_seed *seeds, int64_t n, int rank, int world, pnr_allgather_fn exchange, void *user,
                             pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links,
                             int64_t *n_traces_used, int64_t *n_iterations)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(world >= 1 && rank >= 0 && rank < world, PNR_E_ARG, "rank %d outside a world of %d", rank, world);
    PNR_REQUIRE(world == 1 || exchange, PNR_E_ARG, "sharded tracing needs an exchange callback");
    pnr::ShardSpec sh;
    sh.rank = rank; sh.world = world; sh.exchange = exchange; sh.user = user; sh.block_bytes = c->opt.exchange_block;
    return trace_replay_impl(c, seeds, n, 0, sh, nodes, cap_nodes, n_nodes, links, cap_links, n_links, n_traces_used, n_iterations);
}

// ---- the scheduler of pnr_trace_replay[_sharded] over a HOST engine that plays map-free traces (no GPU involved) -----------
namespace {
struct PlaybackEngine final : pnr::StreamEngine {
    // (s_*: the state wait() hands to the scheduler -- the one behind the first poll - lag steps of the last launch, as PhasedEngine's)
    struct Slot { bool used = false, done = false, s_done = false; int it = 0, T = 0, Tfree = 0, s_it = 0, s_T = 0; std::vector<pnr_xest> xc; };
    const pnr_params &prm;
    int64_t W, H;
    int ni, nslots;
    pnr_trace_fn fn;
    void *user;
    std::vector<Slot> sl;
    std::vector<std::vector<int>> active; // per group
    // stream order, modelled: a control() is queued on its group's stream and has only run for sure once that group has been waited
    // for (or settled); until then no OTHER group may be handed a slot it names (the HIP engine would race: advisor finding, round 3)
    std::vector<int> ctl_pending; // per slot: the group whose control() names it and may not have run yet, or -1
    int s_active[4] = {0, 0, 0, 0};
    std::unordered_map<int64_t, uint8_t> den;
    std::string msg;
    int64_t steps = 0;
    PlaybackEngine(const pnr_params &p, int64_t w, int64_t h, int window, pnr_trace_fn f, void *u)
        : prm(p), W(w), H(h), ni(p.ni), nslots(window), fn(f), user(u), sl((size_t)window), active(4), ctl_pending((size_t)window, -1) {}
    const char *error() const override { return msg.c_str(); }
    int slots() const override { return nslots; }
    int max_groups() const override { return 4; }
    int admit(int g, const int *slots, const float *s6, int m) override
    {
        for (int j = 0; j < m; j++) {
            if (ctl_pending[(size_t)slots[j]] >= 0 && ctl_pending[(size_t)slots[j]] != g) {
                msg = "slot handed to another trace group before the control() that frees it has run";
                return PNR_E_STATE;
            }
            Slot &s = sl[(size_t)slots[j]];
            s = Slot();
            s.used = true;
            s.xc.assign((size_t)ni, pnr_xest{});
            int32_t T = 0;
            const int rc = fn(user, s6 + (size_t)j * 6, &T, s.xc.data());
            if (rc) { msg = "trace callback failed"; return PNR_E_STATE; }
            s.Tfree = T;
            active[(size_t)g].push_back(slots[j]);
        }
        return PNR_OK;
    }
    void snapshot(int g)
    {
        s_active[g] = (int)active[(size_t)g].size();
        for (Slot &s : sl) { s.s_done = s.done; s.s_it = s.it; s.s_T = s.T; } // (all slots: PhasedEngine copies the whole flag array, too)
    }
    int launch(int g, int, int poll, int lag) override
    {
        // what ph_update does with a trace, on the recorded map-free result: iteration `it` fails (T = it), or succeeds and its
        // centroid voxel is saturated in the replayed map (DENSITY stop, T = it + 1), or the trace goes on
        for (int k = 0; k < poll; k++) {
            std::vector<int> keep;
            for (int slot : active[(size_t)g]) {
                Slot &s = sl[(size_t)slot];
                if (s.it >= s.Tfree || s.it >= ni) { s.T = s.Tfree; s.done = true; continue; }
                const pnr_xest &e = s.xc[(size_t)s.it];
                const int64_t v = (int64_t)(int)std::round(e.z) * W * H + (int64_t)(int)std::round(e.y) * W + (int)std::round(e.x);
                auto f = den.find(v);
                s.it++;
                if (f != den.end() && (int)f->second >= prm.nodepervol) { s.T = s.it; s.done = true; continue; }
                keep.push_back(slot);
            }
            active[(size_t)g].swap(keep);
            steps++;
            if (k == poll - 1 - lag) snapshot(g);
        }
        return PNR_OK;
    }
    int wait(int g, int *act) override
    {
        *act = s_active[g];
        for (int &p : ctl_pending) if (p == g) p = -1;
        return PNR_OK;
    }
    int settle(int g) override
    {
        for (int &p : ctl_pending) if (p == g) p = -1;
        return PNR_OK;
    }
    bool finished(int, int slot, int *T) const override { *T = sl[(size_t)slot].s_T; return sl[(size_t)slot].s_done; }
    const pnr_xest *rows(int slot) const override { return sl[(size_t)slot].xc.data(); }
    int progress(int, int slot) const override { return sl[(size_t)slot].s_it; }
    int control(int g, const int *pause, int np, const int *resume, int nr) override
    {
        std::vector<int> &a = active[(size_t)g];
        for (int j = 0; j < np; j++) {
            ctl_pending[(size_t)pause[j]] = g;
            auto f = std::find(a.begin(), a.end(), pause[j]);
            if (f == a.end()) { // (stopped by itself in the steps that ran behind the state the scheduler decided on)
                if (!sl[(size_t)pause[j]].done) { msg = "pause of a trace that is not stepped"; return PNR_E_STATE; }
                continue;
            }
            a.erase(f);
        }
        for (int j = 0; j < nr; j++) {
            if (std::find(a.begin(), a.end(), resume[j]) != a.end()) { msg = "resume of a trace that is stepped"; return PNR_E_STATE; }
            a.push_back(resume[j]);
        }
        return PNR_OK;
    }
    int density_update(const pnr::Replayer &r, int) override
    {
        for (int64_t v : r.touched) den[v] = (uint8_t)r.den_at(v);
        return PNR_OK;
    }
    void drain() override {}
};
} // namespace

int pnr_sched_playback(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n, int rank, int world,
                       pnr_allgather_fn exchange, void *xuser, int64_t block_bytes, pnr_trace_fn trace, void *tuser, int window, int groups,
                       int poll, int look0, int look_pct, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                       int64_t *n_links, int64_t *n_traces_used, int64_t *n_iterations)
{
    if (window < 2) window = 2; // (this entry point has always clamped; only pnr_sched_playback2 treats a window below 2 as a set-up failure)
    return pnr_sched_playback2(p, w, h, l, seeds, n, rank, world, exchange, xuser, block_bytes, trace, tuser, window, groups, poll, look0, look_pct,
                               /*tentative*/ 1, /*target*/ -1, /*lag*/ -1, nodes, cap_nodes, n_nodes, links, cap_links, n_links, n_traces_used, n_iterations);
}

int pnr_sched_playback2(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n, int rank, int world,
                        pnr_allgather_fn exchange, void *xuser, int64_t block_bytes, pnr_trace_fn trace, void *tuser, int window, int groups,
                        int poll, int look0, int look_pct, int tentative, int target, int lag, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes,
                        int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used, int64_t *n_iterations)
{
    PNR_REQUIRE(p && trace && n_nodes && n_links && (n == 0 || seeds), PNR_E_ARG, "null argument");
    PNR_REQUIRE(w > 0 && h > 0 && l > 0, PNR_E_ARG, "bad dimensions");
    PNR_REQUIRE(world >= 1 && rank >= 0 && rank < world && (world == 1 || exchange), PNR_E_ARG, "bad rank / world / exchange");
    pnr::ShardSpec sh;
    sh.rank = rank; sh.world = world; sh.exchange = exchange; sh.user = xuser; sh.block_bytes = block_bytes;
    if (window < 2) { // the playback engine's "set-up failure" (what an out-of-memory GPU is to the HIP engine): the other ranks must hear of it
        set_error("playback engine: a window of %d trace slots", window);
        if (n > 0) pnr::abort_exchange(sh, p->ni);
        return PNR_E_ARG;
    }
    pnr::Replayer r(*p, w, h, l);
    window &= ~1;
    PlaybackEngine eng(*p, w, h, window, trace, tuser);
    pnr::SchedOptions o;
    o.window = window; o.groups = std::max(1, groups); o.poll = std::max(1, poll);
    o.look0 = std::max(0, look0); o.look_pct = look_pct;
    o.tentative = tentative != 0;
    o.target = std::max(-1, target);
    o.lag = std::max(-1, lag);
    pnr::SchedStats st;
    std::string err;
    const int rc = pnr::run_stream(eng, seeds, n, p->ni, o, sh, r, &st, err);
    if (rc) { set_error("%s", err.c_str()); return rc; }
    put_graph(r.nodes, r.links, nodes, cap_nodes, n_nodes, links, cap_links, n_links);
    if (n_traces_used) *n_traces_used = r.trace_count;
    if (n_iterations) *n_iterations = st.iters;
    return PNR_OK;
}

// ---- options ----------------------------------------------------------------------------
namespace {
struct OptEntry { const char *key; int pnr::Options::*i32; int64_t pnr::Options::*i64; int64_t lo, hi; };
const OptEntry OPTS[] = {
    {"window", &pnr::Options::window, nullptr, 0, 1 << 20},      {"look0", &pnr::Options::look0, nullptr, 0, 1 << 24},
    {"look_pct", &pnr::Options::look_pct, nullptr, -1, 100000},   {"poll", &pnr::Options::poll, nullptr, 0, 1024},
    {"groups", &pnr::Options::groups, nullptr, 0, 4},            {"split_x10", &pnr::Options::split_x10, nullptr, 0, 10000},
    {"max_split", &pnr::Options::max_split, nullptr, 1, 4096},   {"stash_mb", nullptr, &pnr::Options::stash_mb, 1, 1 << 20},
    {"host_threads", &pnr::Options::host_threads, nullptr, 0, 1024}, {"local_ranks", &pnr::Options::local_ranks, nullptr, 1, 1024},
    {"trace_timing", &pnr::Options::trace_timing, nullptr, 0, 1}, {"seed_timing", &pnr::Options::seed_timing, nullptr, 0, 1},
    {"trace_log", &pnr::Options::trace_log, nullptr, 0, 1},
    {"replay_batches", &pnr::Options::replay_batches, nullptr, 0, 1}, {"batch_growth", &pnr::Options::batch_growth, nullptr, 100, 100000},
    {"batch_max", &pnr::Options::batch_max, nullptr, 1, 1 << 24}, {"no_stash", &pnr::Options::no_stash, nullptr, 0, 1},
    {"exchange_block", nullptr, &pnr::Options::exchange_block, 0, 1 << 28}, {"frangi_prune", &pnr::Options::frangi_prune, nullptr, 0, 1},
    {"cube_copy", &pnr::Options::cube_copy, nullptr, 0, 1},      {"gauss_march", &pnr::Options::gauss_march, nullptr, 0, 1},
    {"tentative", &pnr::Options::tentative, nullptr, 0, 1},      {"target", &pnr::Options::target, nullptr, -1, 1 << 20},
    {"sums_deep", &pnr::Options::sums_deep, nullptr, -1, 1},      {"sums_deep_max", &pnr::Options::sums_deep_max, nullptr, 0, 1 << 20},
    {"lag", &pnr::Options::lag, nullptr, -1, 1023},               {"profile_every", &pnr::Options::profile_every, nullptr, 1, 1024},
    {"overfill", &pnr::Options::overfill, nullptr, 0, 1},        {"concentrate", &pnr::Options::concentrate, nullptr, 0, 100},
    {"share_scales", &pnr::Options::share_scales, nullptr, 0, 1}, {"share_min", &pnr::Options::share_min, nullptr, 0, 1 << 20},
    {"hess_chunk", &pnr::Options::hess_chunk, nullptr, 0, 1 << 20},
    {"dist_split", &pnr::Options::dist_split, nullptr, 0, 1 << 22}, {"dist_pairs_per_launch", nullptr, &pnr::Options::dist_pairs_per_launch, 0, 1ll << 44},
    {"join_split", &pnr::Options::join_split, nullptr, 0, 1 << 22}, {"join_pairs_per_launch", nullptr, &pnr::Options::join_pairs_per_launch, 0, 1ll << 44},
    {"render_piece", &pnr::Options::render_piece, nullptr, 0, 1 << 20}, {"render_box", nullptr, &pnr::Options::render_box, 0, 1 << 24},
    {"render_items_per_launch", nullptr, &pnr::Options::render_items_per_launch, 0, 1 << 24},
    {"geo_iters", &pnr::Options::geo_iters, nullptr, 0, 1 << 16}, {"geo_tiles_per_launch", &pnr::Options::geo_tiles_per_launch, nullptr, 0, 1 << 24},
    {"geojoin_tiles_per_launch", &pnr::Options::geojoin_tiles_per_launch, nullptr, 0, 1 << 24},
};
} // namespace

int pnr_set_option(pnr_ctx *c, const char *key, int64_t value)
{
    PNR_REQUIRE(c && key, PNR_E_ARG, "null argument");
    if (std::strcmp(key, "recon_timing") == 0) { // process-wide: pnr_reconstruct takes no context
        PNR_REQUIRE(value == 0 || value == 1, PNR_E_ARG, "option recon_timing = %lld outside [0, 1]", (long long)value);
        advantra::set_recon_timing(value != 0);
        return PNR_OK;
    }
    for (const OptEntry &e : OPTS)
        if (std::strcmp(e.key, key) == 0) {
            PNR_REQUIRE(value >= e.lo && value <= e.hi, PNR_E_ARG, "option %s = %lld outside [%lld, %lld]", key, (long long)value, (long long)e.lo, (long long)e.hi);
            if (e.i32) c->opt.*(e.i32) = (int)value; else c->opt.*(e.i64) = value;
            return PNR_OK;
        }
    set_error("unknown option '%s'", key);
    return PNR_E_ARG;
}

int pnr_get_option(pnr_ctx *c, const char *key, int64_t *value)
{
    PNR_REQUIRE(c && key && value, PNR_E_ARG, "null argument");
    if (std::strcmp(key, "recon_timing") == 0) { *value = advantra::recon_timing() ? 1 : 0; return PNR_OK; }
    if (std::strcmp(key, "host_threads_effective") == 0) { *value = pnr::host_threads(c->opt); return PNR_OK; }
    if (std::strcmp(key, "join_rounds") == 0) { *value = c->join_rounds; return PNR_OK; }
    if (std::strcmp(key, "geo_rounds") == 0) { *value = c->geo_rounds; return PNR_OK; }
    if (std::strcmp(key, "geo_visits") == 0) { *value = c->geo_visits; return PNR_OK; }
    if (std::strcmp(key, "geojoin_rounds") == 0) { *value = c->geojoin_rounds; return PNR_OK; }
    if (std::strcmp(key, "render_items") == 0) { *value = c->render_items; return PNR_OK; }
    if (std::strcmp(key, "render_pairs") == 0) { *value = c->render_pairs; return PNR_OK; }
    if (std::strcmp(key, "frangi_recomputes") == 0) { *value = c->frangi_recomputes; return PNR_OK; } // exact Frangi re-runs so far (one pnr_frangi of GPU time each)
    for (const OptEntry &e : OPTS)
        if (std::strcmp(e.key, key) == 0) {
            *value = e.i32 ? (int64_t)(c->opt.*(e.i32)) : c->opt.*(e.i64);
            return PNR_OK;
        }
    set_error("unknown option '%s'", key);
    return PNR_E_ARG;
}

// The one front of the four pnr_reconstruct* forms.  c (nullable): its GPU runs the two neighbour stages, else the host alone.  staged: the
// list behind `stage` with its links (pairs) comes back; else the tree, out_links = the parents.  The plugin constants stand for values <= 0.
static int reconstruct_front(pnr_ctx *c, bool staged, int stage, const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                             float sig2radius, int refine_iter, float epsilon2, float group_radius, int tree_size_min, pnr_node *out_nodes, int64_t cap_nodes,
                             int64_t *n_out_nodes, int32_t *out_links, int64_t cap_links, int64_t *n_out_links)
{
    PNR_REQUIRE(nodes && n_nodes >= 1 && n_out_nodes && (!staged || n_out_links) && (n_links == 0 || links), PNR_E_ARG, "null argument");
    PNR_REQUIRE(!staged || (stage >= advantra::RECON_N0RES && stage <= advantra::RECON_N2TREE), PNR_E_ARG, "stage %d outside [1, 4]", stage);
    PNR_REQUIRE(!c || refine_iter <= PNR_RECON_MAX_ITER, PNR_E_ARG, "refine_iter = %d above %d", refine_iter, PNR_RECON_MAX_ITER);
    for (int64_t k = 0; k < 2 * n_links; k++) PNR_REQUIRE(links[k] >= 0 && links[k] < n_nodes, PNR_E_ARG, "link index out of range");
    advantra::ReconParams rp;
    if (trace_rsmpl > 0) rp.trace_rsmpl = trace_rsmpl;
    if (sig2radius > 0) rp.sig2radius = sig2radius;
    if (refine_iter > 0) rp.refine_iter = refine_iter;
    if (epsilon2 > 0) rp.epsilon2 = epsilon2;
    if (group_radius > 0) rp.group_radius = group_radius;
    if (!staged) {
        if (tree_size_min > 0) rp.tree_size_min = tree_size_min;
        rp.single_tree = tree_size_min < 0;
    }
    if (c) {
        rp.shift = [c](const std::vector<advantra::P4> &src, float s2r, int iters, float eps2, std::vector<advantra::P4> &res) {
            return pnr_recon_shift(c, src, s2r, iters, eps2, res);
        };
        rp.balls = [c](const std::vector<advantra::P4> &pos, float rad, advantra::BallLists &out) { return pnr_recon_balls(c, pos, rad, out); };
    } else {
        rp.threads = pnr::host_threads(pnr::Options()); // rank 0 post-processes alone: every CPU this process may use
    }
    std::vector<pnr_node> in(nodes, nodes + n_nodes), out;
    std::vector<int32_t> lk(links, links + 2 * n_links), par, sl;
    if (int rc = advantra::reconstruct(in, lk, rp, out, par, staged ? stage : advantra::RECON_FINAL, staged ? &sl : nullptr)) return rc;
    if (staged) return put_graph(out, sl, out_nodes, cap_nodes, n_out_nodes, out_links, cap_links, n_out_links);
    *n_out_nodes = (int64_t)out.size();
    const size_t m = (size_t)std::min<int64_t>(cap_nodes, *n_out_nodes);
    if (out_nodes) std::memcpy(out_nodes, out.data(), sizeof(pnr_node) * m);
    if (out_links) std::memcpy(out_links, par.data(), 4 * m);
    return PNR_OK;
}

int pnr_reconstruct(const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                    float sig2radius, int refine_iter, float epsilon2, float group_radius, int tree_size_min,
                    pnr_node *out_nodes, int32_t *out_parent, int64_t cap, int64_t *n_out)
{
    return reconstruct_front(nullptr, false, 0, nodes, n_nodes, links, n_links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, tree_size_min, out_nodes,
                             cap, n_out, out_parent, cap, nullptr);
}

int pnr_reconstruct_stage(const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl, float sig2radius,
                          int refine_iter, float epsilon2, float group_radius, int stage, pnr_node *out_nodes, int64_t cap_nodes,
                          int64_t *n_out_nodes, int32_t *out_links, int64_t cap_links, int64_t *n_out_links)
{
    return reconstruct_front(nullptr, true, stage, nodes, n_nodes, links, n_links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, 0, out_nodes,
                             cap_nodes, n_out_nodes, out_links, cap_links, n_out_links);
}

int pnr_reconstruct_ctx(pnr_ctx *c, const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                        float sig2radius, int refine_iter, float epsilon2, float group_radius, int tree_size_min,
                        pnr_node *out_nodes, int32_t *out_parent, int64_t cap, int64_t *n_out)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null argument");
    return reconstruct_front(c, false, 0, nodes, n_nodes, links, n_links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, tree_size_min, out_nodes, cap,
                             n_out, out_parent, cap, nullptr);
}

int pnr_reconstruct_stage_ctx(pnr_ctx *c, const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                              float sig2radius, int refine_iter, float epsilon2, float group_radius, int stage, pnr_node *out_nodes,
                              int64_t cap_nodes, int64_t *n_out_nodes, int32_t *out_links, int64_t cap_links, int64_t *n_out_links)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null argument");
    return reconstruct_front(c, true, stage, nodes, n_nodes, links, n_links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, 0, out_nodes, cap_nodes,
                             n_out_nodes, out_links, cap_links, n_out_links);
}

int pnr_get_table(pnr_ctx *c, const char *name, void *out, int64_t cap, int64_t *n)
{
    PNR_REQUIRE(c && name && n, PNR_E_ARG, "null argument");
    const pnr::Tables &t = c->tab;
    const void *src = nullptr;
    size_t cnt = 0;
    std::string nm(name);
    auto fv = [&](const std::vector<float> &v) { src = v.data(); cnt = v.size(); };
    std::vector<float> tmp;
    if (nm == "p") fv(t.p);
    else if (nm == "u") fv(t.u);
    else if (nm == "w0") fv(t.w0);
    else if (nm == "w0_cws") fv(t.w0_cws);
    else if (nm == "v") fv(t.v);
    else if (nm == "w") fv(t.w);
    else if (nm == "w_cws") fv(t.w_cws);
    else if (nm == "model_avg") fv(t.mavg);
    else if (nm == "rng") { src = t.rng.data(); cnt = t.rng.size(); }
    else if (nm == "scale_share") { src = t.share_tab.data(); cnt = t.share_tab.size(); } // int32 words
    else if (nm.rfind("model_vuw", 0) == 0 || nm.rfind("model_wgt", 0) == 0 || nm.rfind("gauss_xy", 0) == 0 ||
             nm.rfind("gauss_z", 0) == 0) {
        const size_t pre = (nm[0] == 'm') ? 9 : (nm[6] == 'x' ? 8 : 7);
        const int s = std::atoi(nm.c_str() + pre);
        PNR_REQUIRE(s >= 0 && s < t.nsig, PNR_E_ARG, "sigma index out of range in '%s'", name);
        if (nm[0] == 'g') fv(nm[6] == 'x' ? t.gxy[s] : t.gz[s]);
        else if (nm[6] == 'w') { src = t.mwgt.data() + t.moff[s]; cnt = (size_t)t.M[s]; }
        else {
            tmp.resize((size_t)t.M[s] * 3);
            for (int k = 0; k < t.M[s]; k++)
                for (int q = 0; q < 3; q++) tmp[(size_t)k * 3 + q] = t.tmpl[((size_t)t.moff[s] + k) * 4 + q];
            fv(tmp);
        }
    } else {
        set_error("unknown table '%s'", name);
        return PNR_E_ARG;
    }
    *n = (int64_t)cnt;
    if (out && cap > 0) std::memcpy(out, src, std::min<size_t>(cnt, (size_t)cap) * 4);
    return PNR_OK;
}

int pnr_set_smc_driver(pnr_ctx *c, int driver)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(driver == 0 || driver == 1, PNR_E_ARG, "smc driver must be 0 (phased) or 1 (persistent), got %d", driver);
    c->smc_driver = driver;
    return PNR_OK;
}

int pnr_set_profiling(pnr_ctx *c, int enable)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    c->profiling = enable != 0;
    return PNR_OK;
}

int pnr_get_kernel_ms(pnr_ctx *c, const char *group, double *ms, int64_t *launches)
{
    PNR_REQUIRE(c && group && ms, PNR_E_ARG, "null argument");
    c->resolve_timers();
    if (std::strcmp(group, "render") == 0) { // the two halves of a render are timed apart
        double a = 0, b = 0;
        int64_t la = 0, lb = 0;
        pnr_get_kernel_ms(c, "render_scatter", &a, &la);
        pnr_get_kernel_ms(c, "render_finish", &b, &lb);
        *ms = a + b;
        if (launches) *launches = la + lb;
        return PNR_OK;
    }
    if (std::strcmp(group, "components") == 0) { // one sub-group per phase (components.hip)
        *ms = 0;
        if (launches) *launches = 0;
        for (const char *g : {"components_threshold", "components_local", "components_merge", "components_flatten", "components_number", "components_stats", "components_finish"}) {
            double a = 0;
            int64_t la = 0;
            pnr_get_kernel_ms(c, g, &a, &la);
            *ms += a;
            if (launches) *launches += la;
        }
        return PNR_OK;
    }
    if (std::strcmp(group, "edt") == 0) { // one sub-group per kernel (edt.hip)
        *ms = 0;
        if (launches) *launches = 0;
        for (const char *g : {"edt_threshold", "edt_x", "edt_y", "edt_z", "edt_stats", "edt_sample"}) {
            double a = 0;
            int64_t la = 0;
            pnr_get_kernel_ms(c, g, &a, &la);
            *ms += a;
            if (launches) *launches += la;
        }
        return PNR_OK;
    }
    if (std::strcmp(group, "thin") == 0) { // one sub-group per phase (thin.hip)
        *ms = 0;
        if (launches) *launches = 0;
        for (const char *g : {"thin_threshold", "thin_init", "thin_mark", "thin_pass", "thin_list", "thin_finish"}) {
            double a = 0;
            int64_t la = 0;
            pnr_get_kernel_ms(c, g, &a, &la);
            *ms += a;
            if (launches) *launches += la;
        }
        return PNR_OK;
    }
    if (std::strcmp(group, "geodesic") == 0) { // one sub-group per phase (geodesic.hip)
        *ms = 0;
        if (launches) *launches = 0;
        for (const char *g : {"geodesic_threshold", "geodesic_init", "geodesic_compact", "geodesic_relax", "geodesic_stats", "geodesic_split", "geodesic_sample", "geodesic_paths"}) {
            double a = 0;
            int64_t la = 0;
            pnr_get_kernel_ms(c, g, &a, &la);
            *ms += a;
            if (launches) *launches += la;
        }
        return PNR_OK;
    }
    if (std::strcmp(group, "geojoin") == 0) { // the two passes of a Boruvka round (geojoin.hip)
        double a = 0, b = 0;
        int64_t la = 0, lb = 0;
        pnr_get_kernel_ms(c, "geojoin_meet_w", &a, &la);
        pnr_get_kernel_ms(c, "geojoin_meet_e", &b, &lb);
        *ms = a + b;
        if (launches) *launches = la + lb;
        return PNR_OK;
    }
    auto it = c->timers.find(group);
    *ms = (it == c->timers.end()) ? 0.0 : it->second.ms;
    if (launches) *launches = (it == c->timers.end()) ? 0 : it->second.launches;
    return PNR_OK;
}

int pnr_reset_kernel_ms(pnr_ctx *c)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    c->resolve_timers();
    c->timers.clear();
    return PNR_OK;
}

int pnr_expf_batch(pnr_ctx *c, const float *x, int64_t n, float *y)
{
    PNR_REQUIRE(c && (n == 0 || (x && y)), PNR_E_ARG, "null argument");
    return pnr_expf_run(c, x, n, y);
}

int pnr_eigen_batch(pnr_ctx *c, const double *A, int64_t n, double *V, double *d)
{
    PNR_REQUIRE(c && n >= 0 && (n == 0 || (A && d)), PNR_E_ARG, "null argument");
    return pnr_eigen_run(c, A, n, V, d);
}

} // extern "C"
