// ctx.h -- internal state of one pnr_ctx (one GPU) and small helpers shared by the
// translation units of libpnr_hip.so.  Not part of the C ABI.
#pragma once
#include "../../include/pnr_hip.h"
#include "../../include/pnr_hip_test.h" // the test taps (implemented beside the product entry points)
#include "devbuf.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace pnr {

void set_error(const char *fmt, ...);

#define PNR_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            pnr::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return PNR_E_HIP;                                                                \
        }                                                                                    \
    } while (0)

#define PNR_REQUIRE(cond, code, ...)      \
    do {                                  \
        if (!(cond)) {                    \
            pnr::set_error(__VA_ARGS__);  \
            return (code);                \
        }                                 \
    } while (0)

// ---- host tables (tables.cpp): Tracker::Tracker (tracker.cpp:79-527) + Gaussian taps ----
struct Tables {
    int sz = 0, ndir = 50, nsig = 0;
    bool is2d = false; // built for a single-slice stack (P == 1)
    std::vector<float> p, u, d0, w0, w0_cws, v, w, w_cws; // p,u: sz x 3; w,w_cws: ndir x sz
    std::vector<int> M;                                   // samples per sigma
    std::vector<int> moff;                                // prefix offsets into tmpl
    std::vector<float> tmpl;                              // sum(M) x 4 : (v_off, u_off, w_off, wgt - avg)
    std::vector<float> mwgt;                              // sum(M)     : raw template weights
    std::vector<float> mavg, corrc;                       // per sigma
    std::vector<int> grid;                                // per sigma: nv, nu, nw, first sample
    std::vector<float> axes;                              // per sigma: vv[nv] | uu[nu] | ww[nw]
    std::vector<int> axes_off;                            // per sigma offset into axes
    std::vector<float> wd;                                // sum(M): wgt - avg
    float ext_v = 0, ext_uw = 0;                          // largest |vv| and |uu|,|ww|
    std::vector<float> ext_vs, ext_uws;                   // the same per sigma
    // scales whose template grid nests in another's (find_scale_pairs): a GUEST's samples are a subsequence, in order, of its
    // HOST's, so the phased driver samples the host only and reads the guest's samples from the host's stash
    struct ScalePair { int guest, host, v0, nv, u0, nu, w0, nw; }; // runs [x0, x0 + nx) of the host's axes that are the guest's
    std::vector<ScalePair> pairs;
    std::vector<int> share_tab;                           // device form (TabX::share): [0, 8) host of scale s or -1; [8, 16) s's first entry in grows
    std::vector<int> grows;                               // per guest: the host's stash row of each of its samples, in its own order
    int guest_mask = 0;                                   // bit s: scale s is a guest
    std::vector<uint32_t> rng;                            // np + 1 glibc rand() draws
    std::vector<std::vector<float>> gxy, gz;              // Gaussian taps per sigma
};
void build_tables(const pnr_params &p, bool is2d, Tables &t);
void find_scale_pairs(Tables &t); // (part of build_tables; t.pairs and the device tables from t.grid / t.axes / t.wd)
void glibc_rand_stream(uint32_t seed, int n, uint32_t *out);
int gaussian_taps(float sig, std::vector<float> &g); // returns radius L

// scheduler / host-side knobs of one context (pnr_set_option); none of them changes a result
struct Options {
    int window = 0;           // trace slots the streaming tracer keeps busy (0: automatic -- 1536 on one GPU with the tentative replay, 768 otherwise)
    int look0 = 0, look_pct = -1; // admission lookahead max(look0, frontier * look_pct / 100); 0 / -1 = automatic (stream_sched.h)
    int target = -1;          // running traces the admission keeps up (0: off, -1: automatic -- 120 on one GPU with the tentative replay)
    int sums_deep = -1;       // form of the ordered sums: -1 automatic (smc_phased.hip sums_deep()), 0 two buffers folded, 1 four buffers in turn
    int sums_deep_max = 96;   // ... automatic with several trace groups: the four-buffer form for launches of at most this many traces (round 4: 64 -> 96, -1 % on both bench workloads)
    int lag = -1;             // steps of a poll that run while the host works on the state in front of them (-1 automatic: stream_sched.h)
    int concentrate = 1;      // several trace groups: new seeds go to group 0 only while few traces survive a poll (experiment switch)
    int overfill = 1;         // the target is the mean over a poll, not the count at its start (experiment switch)
    int poll = 0;             // SMC steps between two polls; 0 = automatic (stream_sched.h run_stream: 2 on one or two GPUs, 4 from four ranks on)
    int groups = 0;           // trace groups on separate streams (0: automatic -- 2 on one GPU: one group's ordered sums overlap the other's sampling;
                              // 1 sharded: every poll is then an exchange, and small launches gain nothing from sharing the CUs)
    int split_x10 = 0;        // sampling work-groups per CU x 10 and launch; 0 = automatic (40 with one trace group, 22 with several)
    int max_split = 96;       // ... and at most this many per trace (round 4: 24 -> 96: the last few traces of a late poll are spread over the whole chip)
    int64_t stash_mb = 65536; // sample-stash budget
    int host_threads = 0;     // host worker threads of the seed flood fill / reconstruct(); 0 = hardware threads / local_ranks
    int local_ranks = 1;      // processes that share this host (one per GPU)
    int trace_timing = 0, seed_timing = 0; // statistics on stderr
    int profile_every = 1;    // with pnr_set_profiling: the streaming tracer times the kernels of every n-th poll of a trace group only and counts
                              // them n-fold (the event pairs around ~9000 launches per stack are 1.2 % of the bench step; every 4th: 0.3 %)
    int trace_log = 0;        // keep how every replayed trace ended (pnr_get_trace_log)
    int replay_batches = 0;   // 1: seed-rank batches instead of the streaming window (always so with the persistent driver)
    int batch_growth = 200, batch_max = 1024;
    int no_stash = 0;         // persistent driver: in-lane two-pass sums
    int frangi_prune = 1;       // skip the eigen-solver where the response cannot reach the first non-zero J8 level (frangi.hip)
    int hess_chunk = 0;         // at most this many planes per z-chunk of the Hessian stage, rounded down to whole marches (0: the automatic
                                // 2^27 voxels; frangi.hip hess_chunk_planes -- only ever lowers it: tests reach chunk boundaries on small stacks)
    int tentative = 1;          // streaming scheduler: pause traces that a tentative replay of everything recorded so far cuts (stream_sched.h)
    int gauss_march = 1;        // the fused x-y Gaussian marches down strips of a slice (gauss_xy_u8_m; 0: one 64 x 64 tile per work-group)
    int cube_copy = 1;          // phased driver: the cube of a trace is fetched from the image once per step (ph_cube) and copied by its sampling work-groups (0: each stages it itself)
    int share_scales = 1;       // phased driver: a scale whose template grid nests in another's is not sampled; its sums read the host's
                                // stash (tables.cpp find_scale_pairs; 0: every scale samples on its own -- the same results)
    int share_min = 0;          // ... in steps of at least this many traces (a guest's wave is not the longest of its trace, so small
                                // steps lose nothing by it: 0, not tuned on a workload of its own)
    int dist_split = 0;         // the pair minimum (pairmin.h pair_tiles) of pnr_point_segment_distance: segments per blockIdx.y slice of a launch (0:
                                // automatic -- enough slices to fill the chip), and
    int64_t dist_pairs_per_launch = 0; // at most this many (point, segment) pairs per launch (0: automatic, 2^34); neither changes a result: tests
                                       // reach slice and launch boundaries with them on small inputs
    int join_split = 0;         // the same two for the targets and (point, target) pairs of pnr_nearest_other / pnr_join_trees
    int64_t join_pairs_per_launch = 0;
    int render_piece = 0;       // pnr_render_tree / pnr_tree_coverage (render.h render_items): xy voxels of a segment's axis per piece (0: automatic, 16),
    int64_t render_box = 0;     // voxels per item: larger boxes are cut into sub-boxes (0: automatic, 2^15), and
    int64_t render_items_per_launch = 0; // items per rn_scatter launch (0: automatic, 2^18); none changes a result: tests reach piece, box and launch boundaries with them
    int geo_iters = 0;          // pnr_geodesic_distance (geodesic.hip): LDS iterations per tile visit (0: automatic, 128; 1: a tile that changed re-queues itself), and
    int geo_tiles_per_launch = 0; // tiles per geo_relax launch (0: automatic, 2^20); neither changes a result: tests reach the re-queue path and launch cuts with them
    int geojoin_tiles_per_launch = 0; // pnr_geodesic_bridges (geojoin.hip): tiles per launch of a meet pass (0: automatic, 2^20); changes no result: tests reach launch cuts with it
    int morph_iters = 0;        // pnr_morph_reconstruct / pnr_morph_volume (morph.hip): LDS iterations per tile visit (0: automatic, 64; 1: a tile that changed re-queues itself), and
    int morph_tiles_per_launch = 0; // tiles per morph_relax launch (0: automatic, 2^20); neither changes a result: tests reach the re-queue path and launch cuts with them
    int ws_iters = 0;           // pnr_watershed (watershed.hip): LDS iterations per tile visit of both passes (0: automatic, 64; 1: a tile that changed re-queues itself), and
    int ws_tiles_per_launch = 0; // tiles per ws_flood / ws_label launch (0: automatic, 2^20); neither changes a result: tests reach the re-queue path and launch cuts with them
    int64_t lt_slab_vox = 0;    // pnr_local_threshold[_volume] (threshold.hip): voxels per slab of whole planes (0: automatic, 2^24); changes no result: tests reach slab boundaries with it
    int64_t exchange_block = 0; // bytes per rank and exchange of the sharded tracer; 0 = automatic (256 KB / world, at least 32 KB)
};
int host_threads(const Options &o); // worker threads to use on this host

struct KernelTimer {
    double ms = 0;
    int64_t launches = 0;
};

} // namespace pnr

struct pnr_ctx {
    pnr_params prm;
    pnr::Options opt;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    pnr::Tables tab;

    // volume
    int64_t w = 0, h = 0, l = 0, N = 0;
    const uint8_t *d_img = nullptr; // device: a view of d_img_owned, or of borrowed memory (pnr_set_volume_device)
    pnr::DevBuf<uint8_t> d_img_owned;

    // Frangi state (HBM)
    pnr::DevBuf<float> d_tmpA, d_tmpB, d_J;
    pnr::DevBuf<uint8_t> d_Vx, d_Vy, d_Vz, d_J8;
    pnr::DevBuf<unsigned int> d_minmax;    // [0]=min bits, [1]=max bits
    pnr::DevBuf<float> d_F[PNR_MAX_SIGMAS]; // smoothed volume of every scale, kept for the direction bytes (frangi.hip)
    pnr::DevBuf<uint8_t> d_scale;          // per voxel: the scale whose response is in J
    bool frangi_pruned = false, frangi_exact_once = false; // J / the winning scale of J8 = 0 voxels are not exact (option frangi_prune); next run without it
    float Jmax_run = 0.f;                                   // the maximum the last Frangi run found itself (before pnr_quantise_j8)
    int64_t frangi_recomputes = 0;                          // exact re-runs pnr_get_frangi / pnr_quantise_j8 had to make (pnr_get_option "frangi_recomputes")
    int64_t fr_zs0 = 0, fr_zs1 = 0;                         // planes the extremes of the last Frangi run were taken over
    bool have_scale = false, have_v = false; // d_scale + d_F valid / the direction volumes Vx, Vy, Vz are filled
    pnr::DevBuf<float> d_taps;        // Gaussian taps of all scales (frangi.hip: TAPS_SLOT floats per pass, zero-padded)
    std::vector<float> taps_stage;    // their host staging (asynchronous uploads)
    pnr::DevBuf<float> d_qh;          // survivor queue of the Hessian stage: [region][6][entries]
    pnr::DevBuf<unsigned int> d_qidx, d_qcount;
    int64_t frangi_cap = 0;           // voxels the buffers above were sized for
    bool have_j8 = false;
    float Jmin = 0, Jmax = 0;

    // device tables
    pnr::DevBuf<float> d_p, d_u, d_w0, d_w0cws, d_v, d_w, d_wcws, d_tmpl, d_corrc, d_sig;
    pnr::DevBuf<int> d_M, d_moff, d_grid, d_axes_off;
    pnr::DevBuf<float> d_axes, d_wd;
    pnr::DevBuf<int> d_share, d_grows; // nested scales (Tables::share_tab, grows)
    pnr::DevBuf<uint32_t> d_rng;

    // SMC pass-1 sample stash (HBM scratch, sized at the first trace batch)
    pnr::DevBuf<float> d_stash;
    pnr::DevBuf<int> d_slot_busy;
    size_t stash_bytes = 0;
    int stash_slots = 0;

    // node-density map of earlier trace batches (u8 per voxel), read by smc_trace for early DENSITY stops
    pnr::DevBuf<uint8_t> d_den;
    int64_t den_cap = 0;
    pnr::DevBuf<long long> d_den_idx; // staging for the per-batch scatter of touched voxels
    pnr::DevBuf<uint8_t> d_den_val;

    struct pnr_persistent_bufs *job = nullptr; // device buffers of the persistent driver's batches (smc.hip; run on the ctx stream)
    struct pnr_phased *phased = nullptr; // state of the launch-per-phase SMC driver (smc_phased.hip)
    int smc_driver = 0;                  // 0: launch per phase (default), 1: one persistent work-group per trace

    // soma path (somaradius > 0): one SOMA node per region, sparse voxel -> node-index map (soma.hip)
    std::vector<pnr_node> soma_nodes;
    std::vector<int64_t> soma_vox;   // foreground voxels in raster order
    std::vector<int32_t> soma_lab;   // their region = index in the node list (1-based)
    std::unordered_map<int64_t, int32_t> soma_map;
    bool have_soma = false;

    // seeds
    pnr::PinBuf<unsigned char> h_j8, h_j8v; // pinned staging of the sparse J8 hand-over to the flood fill: bitmap | values (seeds.hip)
    static constexpr int J8_CHUNKS = 16;   // the download is cut into chunks of layers so that the flood fill starts on the first ones
    hipStream_t copy_stream = nullptr;
    hipEvent_t j8_ev[J8_CHUNKS] = {}, j8_start = nullptr;
    std::vector<pnr_seed> seeds;

    // node graph of the last pnr_trace_replay[_sharded] (pnr_get_graph)
    std::vector<pnr_node> graph_nodes;
    std::vector<int32_t> graph_links;
    int graph_traces = 0;
    bool have_graph = false;
    int64_t join_rounds = 0; // nearest-other passes of the last pnr_join_trees (pnr_get_option "join_rounds")
    int64_t render_items = 0, render_pairs = 0; // work items and (voxel, segment) tests of the last render (pnr_get_option "render_items" / "render_pairs")
    int64_t geo_rounds = 0, geo_visits = 0; // relaxation rounds and tile visits of the last pnr_geodesic_distance (pnr_get_option "geo_rounds" / "geo_visits")
    int64_t morph_rounds = 0, morph_visits = 0; // relaxation rounds and tile visits of the last morphological reconstruction (pnr_get_option "morph_rounds" / "morph_visits")
    int64_t ws_rounds = 0, ws_visits = 0; // relaxation rounds and tile visits of the last pnr_watershed, both passes together (pnr_get_option "ws_rounds" / "ws_visits")
    int64_t geojoin_rounds = 0; // Boruvka rounds of the last pnr_geodesic_bridges (pnr_get_option "geojoin_rounds")
    std::vector<int32_t> graph_log; // 5 ints per replayed trace (option "trace_log")

    // shell table of pnr_measure_radii (radius.hip): one per context, rebuilt when what it was built for changes (reallocated with rmax)
    pnr::DevBuf<uint32_t> d_rad_off;
    pnr::DevBuf<int> d_rad_start;
    int rad_rmax = 0; // (0: no table)
    uint32_t rad_zbits = 0; // the bits of zdist
    bool rad_2d = false;

    // profiling: HIP event pairs recorded on the ctx stream around each kernel group, resolved
    // lazily (no host sync inside the timed region)
    bool profiling = false;
    struct Pending {
        std::string group;
        hipEvent_t a, b;
        int launches;
        bool a_shared = false; // a is the b of the entry before (chained timers): not freed twice
        int weight = 1;        // sampled timers (option "profile_every"): this measurement stands for `weight` launches like it
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    hipEvent_t cur_a = nullptr, last_b = nullptr; // last_b: the closing event of the last toc(), reusable as the next opening event
    hipStream_t last_b_stream = nullptr;
    bool cur_a_shared = false;
    std::map<std::string, pnr::KernelTimer> timers;

    // grow-only named device scratch (per-layer tables, candidate keys, ...): nothing is allocated or freed inside a timed stage
    // once the first pass has sized it
    std::map<std::string, pnr::DevBuf<char>> scratch;
    template <typename T>
    int scratch_get(const char *name, size_t count, T **out)
    {
        pnr::DevBuf<char> &b = scratch[name];
        const size_t need = std::max<size_t>(count, 1) * sizeof(T);
        if (b.count() < need) {
            const size_t cap = need + need / 2;
            if (b.alloc(cap) != hipSuccess) { // (releasing the old one synchronises the device)
                pnr::set_error("hipMalloc of %zu B for scratch '%s' failed", cap, name);
                return PNR_E_NOMEM;
            }
        }
        *out = (T *)b.get();
        return PNR_OK;
    }

    hipEvent_t get_event()
    {
        if (!free_events.empty()) {
            hipEvent_t e = free_events.back();
            free_events.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    // chain = true: nothing was queued on the stream since the last toc() on it -- its closing event opens this timer as well (one
    // event per kernel instead of two in the SMC loops, where the events are ~2 % of a step)
    void tic(hipStream_t on = nullptr, bool chain = false)
    {
        if (!profiling) return;
        hipStream_t s = on ? on : stream;
        if (chain && last_b && last_b_stream == s) {
            cur_a = last_b;
            cur_a_shared = true;
            return;
        }
        cur_a = get_event();
        cur_a_shared = false;
        (void)hipEventRecord(cur_a, s);
    }
    void toc(const char *group, int launches = 1, hipStream_t on = nullptr, int weight = 1)
    {
        if (!profiling || !cur_a) return;
        hipStream_t s = on ? on : stream;
        hipEvent_t b = get_event();
        (void)hipEventRecord(b, s);
        pending.push_back(Pending{group, cur_a, b, launches, cur_a_shared, weight});
        cur_a = nullptr;
        last_b = b;
        last_b_stream = s;
    }
    void resolve_timers()
    {
        for (auto &p : pending) {
            (void)hipEventSynchronize(p.b);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, p.a, p.b);
            auto &t = timers[p.group];
            t.ms += (double)ms * p.weight;
            t.launches += (int64_t)p.launches * p.weight;
            if (!p.a_shared) free_events.push_back(p.a);
            free_events.push_back(p.b);
        }
        pending.clear();
        last_b = nullptr;
    }
};

// stage entry points implemented in the .hip files
int pnr_frangi_run(pnr_ctx *c, float *Jmin, float *Jmax);
int pnr_frangi_run_range(pnr_ctx *c, int64_t zs0, int64_t zs1, bool finish, float *Jmin, float *Jmax);
int pnr_j8_run(pnr_ctx *c, float jmin, float jmax);
int pnr_gaussian_run(pnr_ctx *c, float sig, float *d_out /*device N floats*/);
int pnr_hessian_run(pnr_ctx *c, float sig, float *const d_out[6]);
int pnr_seeds_run(pnr_ctx *c, int64_t z0, int64_t z1);
int pnr_seed_handover_run(pnr_ctx *c, int64_t z0, int64_t z1, int32_t *vmin, int32_t *vmax, int64_t *ltot, int64_t *key_off, int64_t *keys,
                          int64_t cap_keys, int64_t *n_keys, uint8_t *layers, int32_t *restored); // test tap (pnr_hip_test.h)
int pnr_soma_run(pnr_ctx *c, uint8_t *E8_out, int32_t *threshold);
int pnr_gauss_x_u8_launch(pnr_ctx *c, const uint8_t *src, float *dst, const float *d_taps, int L);
int pnr_ensure_tmpA(pnr_ctx *c); // the second Gaussian scratch volume / the direction volumes: allocated where they are used (frangi.hip)
int pnr_ensure_v(pnr_ctx *c);
int pnr_zncc_run(pnr_ctx *c, const float *h_pos_dir, int64_t n, float *h_corr, float *h_sig);
int pnr_trace_run(pnr_ctx *c, const pnr_seed *seeds, int64_t n, int32_t *T, int32_t *stop, pnr_xest *xc,
                  int dbg_iters, float *xfilt, int32_t *idxres, float *neff, int use_density);
namespace pnr { struct Replayer; struct ShardSpec; }
struct pnr_persistent_bufs;
void pnr_persistent_destroy(pnr_persistent_bufs *j);
struct pnr_phased;
int pnr_trace_run_phased(pnr_ctx *c, const pnr_seed *seeds, int64_t n, int32_t *T, int32_t *stop, pnr_xest *xc, int dbg_iters,
                         float *xfilt, int32_t *idxres, float *neff, int use_density);
int pnr_phased_likelihood_run(pnr_ctx *c, int64_t nt, const float *poses, const float *centroids, const int32_t *modes, float *corr,
                              int32_t *uidx, int32_t *cmap, int32_t *flags, int32_t *info); // test tap (pnr_hip_test.h)
int pnr_phased_decide_run(pnr_ctx *c, int64_t nt, const pnr_phd_in *in, pnr_phd_out *out); // test tap (pnr_hip_test.h)
void pnr_phased_destroy(pnr_phased *h);
int pnr_trace_replay_stream(pnr_ctx *c, const pnr_seed *seeds, int64_t n, pnr::Replayer &r, const pnr::ShardSpec &sh, int64_t *iters);
int pnr_density_reset(pnr_ctx *c);                       // zero the device density map (allocating it on first use)
int pnr_density_update(pnr_ctx *c, const pnr::Replayer &r, hipStream_t on = nullptr); // push the voxels touched since Replayer::touched was cleared
int pnr_expf_run(pnr_ctx *c, const float *x, int64_t n, float *y);
int pnr_eigen_run(pnr_ctx *c, const double *A, int64_t n, double *V, double *d); // test tap (pnr_hip_test.h)
int pnr_ensure_frangi_buffers(pnr_ctx *c);
int pnr_frangi_materialise_v(pnr_ctx *c);
int pnr_seed_dirs(pnr_ctx *c, const long long *d_idx, int n, unsigned char *d_dirs); // 0: done, 1: gather from the volumes, < 0: error
