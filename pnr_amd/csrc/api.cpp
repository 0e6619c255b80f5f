// api.cpp -- the extern "C" boundary of libpnr_hip.so (include/pnr_hip.h), first part: the context's life-cycle with its parameter
// validation (Advantra::dofunc, Advantra_plugin.cpp:317-326), the volume, the options, the kernel timers and the tracker tables; and the
// one error text of the library.  The pipeline's entry points are in api_pipeline.cpp, the volume and tree tools in api_tools.cpp, the
// scheduler over a host engine in playback.cpp; the argument rules they share are in args.h.
#include "args.h"
#include "call.h"
#include "volume.h"
#include "../host/reconstruct.h"
#include <cstdlib>
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

// a new or changed volume: nothing computed from the old one stays valid
static void invalidate_pipeline(pnr_ctx *c)
{
    c->have_j8 = false;
    c->have_v = c->have_scale = false;
    c->frangi_pruned = false;
    c->seeds.clear();
    c->have_soma = false;
}

namespace pnr {
// what pnr_set_volume of the new bytes leaves: an owned volume of the same dimensions, no later pipeline state
void replace_volume(pnr_ctx *c, DevBuf<uint8_t> &&v)
{
    c->d_img_owned = std::move(v); // (empty while the volume was borrowed: a borrowed volume is never written or freed)
    c->d_img = c->d_img_owned.get();
    invalidate_pipeline(c);
    c->have_graph = false;
}
} // namespace pnr

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
    PNR_TRY(validate(*p));
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
    int rc = load_tables(c, /*is2d*/ false);
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
        PNR_TRY(load_tables(c, l == 1));
    }
    return PNR_OK;
}

int pnr_set_volume(pnr_ctx *c, const uint8_t *img, int64_t w, int64_t h, int64_t l)
{
    PNR_REQUIRE(img, PNR_E_ARG, "null image");
    PNR_TRY(set_dims(c, w, h, l));
    c->d_img = nullptr; // never leave the context pointing at a freed image if the allocation below fails
    pnr::Call call(c, "pnr_set_volume");
    call.note(c->d_img_owned.reserve((size_t)c->N));
    call.up(c->d_img_owned.get(), img, (size_t)c->N);
    PNR_TRY(call.finish());
    c->d_img = c->d_img_owned.get();
    return PNR_OK;
}

int pnr_set_volume_device(pnr_ctx *c, const void *dev_img, int64_t w, int64_t h, int64_t l)
{
    PNR_REQUIRE(dev_img, PNR_E_ARG, "null image");
    PNR_TRY(set_dims(c, w, h, l));
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
    PNR_TRY(set_dims(c, w, h, l));
    c->d_img = nullptr; // no volume until the map below has succeeded
    const uint16_t *src = (const uint16_t *)img;
    pnr::DevBuf<char> d_up;
    if (host) {
        const size_t bytes = (size_t)c->N * (size_t)nchan * 2;
        PNR_TRY(pnr::dev_alloc(d_up, bytes, "pnr_set_volume_u16", "for the 16-bit stack"));
        pnr::Call call(c, "pnr_set_volume_u16");
        call.up(d_up.get(), img, bytes);
        if (!call.ok()) return call.finish();
        src = (const uint16_t *)d_up.get();
    }
    const int rc = pnr_volume_u16_run(c, src, nchan, channel, wd, lo_out, hi_out);
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
    PNR_TRY(pnr::args::volume_set(c, "pnr_get_volume"));
    PNR_HIP(hipSetDevice(c->device));
    pnr::Call call(c, "pnr_get_volume");
    call.down(img, c->d_img, (size_t)c->N);
    return call.finish();
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
    {"morph_iters", &pnr::Options::morph_iters, nullptr, 0, 1 << 16}, {"morph_tiles_per_launch", &pnr::Options::morph_tiles_per_launch, nullptr, 0, 1 << 24},
    {"ws_iters", &pnr::Options::ws_iters, nullptr, 0, 1 << 16}, {"ws_tiles_per_launch", &pnr::Options::ws_tiles_per_launch, nullptr, 0, 1 << 24},
    {"lt_slab_vox", nullptr, &pnr::Options::lt_slab_vox, 0, 1ll << 40},
};
// what pnr_get_option reads besides: counters the calls leave in the context
struct Counter { const char *key; int64_t pnr_ctx::*count; };
const Counter COUNTERS[] = {
    {"join_rounds", &pnr_ctx::join_rounds},       {"geo_rounds", &pnr_ctx::geo_rounds},     {"geo_visits", &pnr_ctx::geo_visits},
    {"geojoin_rounds", &pnr_ctx::geojoin_rounds}, {"render_items", &pnr_ctx::render_items}, {"render_pairs", &pnr_ctx::render_pairs},
    {"morph_rounds", &pnr_ctx::morph_rounds},     {"morph_visits", &pnr_ctx::morph_visits},
    {"ws_rounds", &pnr_ctx::ws_rounds},           {"ws_visits", &pnr_ctx::ws_visits},
    {"frangi_recomputes", &pnr_ctx::frangi_recomputes}, // exact Frangi re-runs so far (one pnr_frangi of GPU time each)
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
    for (const Counter &k : COUNTERS)
        if (std::strcmp(k.key, key) == 0) { *value = c->*(k.count); return PNR_OK; }
    for (const OptEntry &e : OPTS)
        if (std::strcmp(e.key, key) == 0) {
            *value = e.i32 ? (int64_t)(c->opt.*(e.i32)) : c->opt.*(e.i64);
            return PNR_OK;
        }
    set_error("unknown option '%s'", key);
    return PNR_E_ARG;
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
    pnr::put(out, cap, (const uint32_t *)src, (int64_t)cnt); // (every table has 4-byte entries)
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

// the groups pnr_get_kernel_ms sums under one name.  A table, not a prefix rule: "smc" is a group of its own beside "smc_sums" and the
// rest, and "geodesic_relax" counts under "geodesic" also when pnr_geodesic_bridges runs it
namespace {
struct Umbrella { const char *group; const char *members[9]; }; // (members: NULL-terminated)
const Umbrella UMBRELLAS[] = {
    {"render", {"render_scatter", "render_finish"}}, // the two halves of a render are timed apart
    {"components", {"components_threshold", "components_local", "components_merge", "components_flatten", "components_number", "components_stats", "components_finish"}},
    {"edt", {"edt_threshold", "edt_x", "edt_y", "edt_z", "edt_stats", "edt_sample"}},
    {"thin", {"thin_threshold", "thin_init", "thin_mark", "thin_pass", "thin_list", "thin_finish"}},
    {"geodesic", {"geodesic_threshold", "geodesic_init", "geodesic_compact", "geodesic_relax", "geodesic_stats", "geodesic_split", "geodesic_sample", "geodesic_paths"}},
    {"geojoin", {"geojoin_meet_w", "geojoin_meet_e"}}, // the two passes of a Boruvka round
    {"morph", {"morph_init", "morph_compact", "morph_relax", "morph_finish"}},
    {"watershed", {"watershed_init", "watershed_compact", "watershed_flood", "watershed_label", "watershed_finish"}},
};
} // namespace

int pnr_get_kernel_ms(pnr_ctx *c, const char *group, double *ms, int64_t *launches)
{
    PNR_REQUIRE(c && group && ms, PNR_E_ARG, "null argument");
    c->resolve_timers();
    const char *const self[2] = {group, nullptr};
    const char *const *member = self;
    for (const Umbrella &u : UMBRELLAS)
        if (std::strcmp(u.group, group) == 0) member = u.members;
    double sum = 0;
    int64_t n = 0;
    for (; *member; member++) {
        const auto it = c->timers.find(*member);
        if (it != c->timers.end()) sum += it->second.ms, n += it->second.launches;
    }
    *ms = sum;
    if (launches) *launches = n;
    return PNR_OK;
}

int pnr_reset_kernel_ms(pnr_ctx *c)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    c->resolve_timers();
    c->timers.clear();
    return PNR_OK;
}

} // extern "C"
