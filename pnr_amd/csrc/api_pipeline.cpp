// api_pipeline.cpp -- the extern "C" boundary of libpnr_hip.so (include/pnr_hip.h), second part: the entry points of the pipeline in its
// order -- Frangi, seeds with the seed filter/sort (Advantra_plugin.cpp:2561-2586), soma, trace, the host replay of the trace bookkeeping
// (tracker.cpp:825-933 + Advantra_plugin.cpp:2602-2710), reconstruct -- and the test taps on single stages of it (include/pnr_hip_test.h).
#include "args.h"
#include "call.h"
#include "replay.h"
#include "stream_sched.h"
#include "../host/reconstruct.h"
#include "recon.h"
#include <numeric>

using pnr::put_graph;
namespace args = pnr::args;

extern "C" {

int pnr_frangi(pnr_ctx *c, float *Jmin, float *Jmax)
{
    PNR_TRY(args::volume_set(c, "pnr_frangi"));
    PNR_HIP(hipSetDevice(c->device));
    return pnr_frangi_run(c, Jmin, Jmax);
}

int pnr_frangi_slab(pnr_ctx *c, int64_t z_keep0, int64_t z_keep1, float *Jmin, float *Jmax)
{
    PNR_TRY(args::volume_set(c, "pnr_frangi_slab"));
    PNR_REQUIRE(c->l > 1, PNR_E_ARG, "pnr_frangi_slab: a single-slice stack has no z-slabs");
    PNR_REQUIRE(z_keep0 >= 0 && z_keep0 < z_keep1 && z_keep1 <= c->l, PNR_E_ARG, "kept planes [%lld,%lld) outside [0,%lld)", (long long)z_keep0,
                (long long)z_keep1, (long long)c->l);
    PNR_HIP(hipSetDevice(c->device));
    return pnr_frangi_run_range(c, z_keep0, z_keep1, /*finish*/ false, Jmin, Jmax);
}

int pnr_quantise_j8(pnr_ctx *c, float Jmin, float Jmax)
{
    PNR_TRY(args::volume_set(c, "pnr_quantise_j8"));
    PNR_HIP(hipSetDevice(c->device));
    if (c->frangi_pruned && !(Jmin == 0.f && Jmax >= c->Jmax_run)) {
        // the last run skipped the solver below the first J8 level of ITS extremes (Jmin = 0, Jmax at least its own maximum): the
        // global extremes of a sharded stack satisfy that; anything else needs the exact response
        c->frangi_exact_once = true;
        c->frangi_recomputes++;
        if (c->opt.trace_timing || c->opt.seed_timing) fprintf(stderr, "[pnr frangi] pnr_quantise_j8(%g, %g): extremes the pruned run did not assume -- exact re-run of every scale\n", Jmin, Jmax);
        PNR_TRY(pnr_frangi_run_range(c, c->fr_zs0, c->fr_zs1, false, nullptr, nullptr));
    }
    return pnr_j8_run(c, Jmin, Jmax);
}

// what a read-back of the Frangi outputs needs in HBM first: the exact J (`exact`: J or a direction volume is asked for) and the
// direction volumes (`dirs`)
static int frangi_for_readback(pnr_ctx *c, bool exact, bool dirs)
{
    PNR_REQUIRE(c && c->have_j8 && c->d_J.get(), PNR_E_STATE, "pnr_get_frangi: run pnr_frangi first");
    if (exact && c->frangi_pruned) {
        // the last run skipped the solver where the response could not reach J8 = 1 (option frangi_prune): J8, the extremes and the
        // seeds are exact, the f32 J and the winning scale of J8 = 0 voxels are not -- recompute without the shortcut, same extremes
        const float jmin = c->Jmin, jmax = c->Jmax;
        c->frangi_exact_once = true;
        c->frangi_recomputes++;
        if (c->opt.trace_timing || c->opt.seed_timing) fprintf(stderr, "[pnr frangi] pnr_get_frangi: J / V asked for after a pruned run -- exact re-run of every scale\n");
        PNR_TRY(pnr_frangi_run_range(c, c->fr_zs0, c->fr_zs1, false, nullptr, nullptr));
        PNR_TRY(pnr_j8_run(c, jmin, jmax));
    }
    if (dirs) PNR_TRY(pnr_frangi_materialise_v(c)); // the pipeline itself only needs the directions at the seeds
    return PNR_OK;
}

int pnr_get_frangi(pnr_ctx *c, float *J, uint8_t *J8, uint8_t *Vx, uint8_t *Vy, uint8_t *Vz)
{
    PNR_TRY(frangi_for_readback(c, J || Vx || Vy || Vz, Vx || Vy || Vz));
    const size_t n = (size_t)c->N;
    pnr::Call call(c, "pnr_get_frangi");
    if (J) call.down(J, c->d_J.get(), n);
    if (J8) call.down(J8, c->d_J8.get(), n);
    if (Vx) call.down(Vx, c->d_Vx.get(), n);
    if (Vy) call.down(Vy, c->d_Vy.get(), n);
    if (Vz) call.down(Vz, c->d_Vz.get(), n);
    return call.finish();
}

// test tap (pnr_hip_test.h): pnr_get_frangi of the box [lo, hi) alone, plane by plane as 2-D copies
int pnr_get_frangi_box(pnr_ctx *c, const int64_t *lo, const int64_t *hi, float *J, uint8_t *J8, uint8_t *Vx, uint8_t *Vy, uint8_t *Vz)
{
    PNR_REQUIRE(c && lo && hi, PNR_E_ARG, "null argument");
    const int64_t ext[3] = {c->l, c->h, c->w};
    for (int a = 0; a < 3; a++)
        PNR_REQUIRE(lo[a] >= 0 && lo[a] < hi[a] && hi[a] <= ext[a], PNR_E_ARG, "pnr_get_frangi_box: [%lld, %lld) outside [0, %lld) on axis %d", (long long)lo[a],
                    (long long)hi[a], (long long)ext[a], a);
    PNR_TRY(frangi_for_readback(c, J || Vx || Vy || Vz, Vx || Vy || Vz));
    const size_t bh = (size_t)(hi[1] - lo[1]), bw = (size_t)(hi[2] - lo[2]), w = (size_t)c->w, h = (size_t)c->h;
    pnr::Call call(c, "pnr_get_frangi_box");
    const auto box = [&](void *dst, const void *src, size_t es) {
        if (!dst) return;
        for (int64_t z = lo[0]; z < hi[0] && call.ok(); z++)
            call.note(hipMemcpy2DAsync((char *)dst + (size_t)(z - lo[0]) * bh * bw * es, bw * es, (const char *)src + (((size_t)z * h + (size_t)lo[1]) * w + (size_t)lo[2]) * es, w * es,
                                       bw * es, bh, hipMemcpyDeviceToHost, call.stream()));
    };
    box(J, c->d_J.get(), 4);
    box(J8, c->d_J8.get(), 1);
    box(Vx, c->d_Vx.get(), 1);
    box(Vy, c->d_Vy.get(), 1);
    box(Vz, c->d_Vz.get(), 1);
    return call.finish();
}

int pnr_gaussian(pnr_ctx *c, float sig, float *F)
{
    PNR_REQUIRE(c && c->d_img && F, PNR_E_STATE, "pnr_gaussian: no volume set"); // (its own line: a null output is answered the same way)
    PNR_REQUIRE(sig > 0, PNR_E_ARG, "sigma must be positive");
    PNR_TRY(pnr_ensure_frangi_buffers(c));
    PNR_TRY(pnr_ensure_tmpA(c));
    PNR_TRY(pnr_gaussian_run(c, sig, c->d_tmpA.get()));
    pnr::Call call(c, "pnr_gaussian");
    call.down(F, c->d_tmpA.get(), (size_t)c->N);
    return call.finish();
}

int pnr_hessian(pnr_ctx *c, float sig, float *Dzz, float *Dyy, float *Dyz, float *Dxx, float *Dxy, float *Dxz)
{
    PNR_TRY(args::volume_set(c, "pnr_hessian"));
    PNR_REQUIRE(c->l > 1, PNR_E_ARG, "pnr_hessian taps the 3-D Hessian: not defined for a single-slice stack");
    PNR_REQUIRE(sig > 0, PNR_E_ARG, "sigma must be positive");
    PNR_TRY(pnr_ensure_frangi_buffers(c));
    pnr::CallBuf buf; // the six volumes (freed when the call returns)
    pnr::Part<float> part[6];
    for (auto &p : part) p = buf.add<float>((size_t)c->N);
    PNR_TRY(buf.alloc("pnr_hessian"));
    float *d[6];
    for (int k = 0; k < 6; k++) d[k] = part[k];
    int rc = pnr_hessian_run(c, sig, d);
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
    PNR_TRY(pnr_ensure_frangi_buffers(c));
    PNR_TRY(pnr_ensure_v(c));
    const size_t n = (size_t)c->N;
    pnr::Call call(c, "pnr_set_j8_v");
    call.up(c->d_J8.get(), J8, n);
    call.up(c->d_Vx.get(), Vx, n);
    call.up(c->d_Vy.get(), Vy, n);
    call.up(c->d_Vz.get(), Vz, n);
    PNR_TRY(call.finish());
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
    PNR_TRY(pnr_seeds_run(c, z0, z1));
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
    PNR_TRY(args::ctx_device(c));
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
        PNR_TRY(pnr_zncc_batch(c, pd.data(), n, corr.data(), nullptr));
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
    PNR_TRY(args::ctx_device(c));
    PNR_TRY(pnr_soma_run(c, E8_out, threshold));
    if (n_soma) *n_soma = (int64_t)c->soma_nodes.size();
    return PNR_OK;
}

int pnr_get_soma(pnr_ctx *c, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int64_t *vox, int32_t *lab, int64_t cap_vox, int64_t *n_vox)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_REQUIRE(c->have_soma, PNR_E_STATE, "pnr_soma has not run");
    if (n_nodes) *n_nodes = (int64_t)c->soma_nodes.size();
    if (n_vox) *n_vox = (int64_t)c->soma_vox.size();
    pnr::put(nodes, cap_nodes, c->soma_nodes);
    pnr::put(vox, cap_vox, c->soma_vox);
    pnr::put(lab, cap_vox, c->soma_lab.data(), (int64_t)c->soma_vox.size()); // (one label per voxel: under the voxels' count)
    return PNR_OK;
}

// ---- host replay ------------------------------------------------------------------------
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
    pnr::put(rec, cap, c->graph_log, 5);
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
        PNR_TRY(pnr_trace_replay_stream(c, seeds, n, r, sh, &iters));
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
        PNR_TRY(pnr_trace_run(c, bs.data(), m, T.data(), stop.data(), xc.data(), 0, nullptr, nullptr, nullptr, /*use_density*/ 1));
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
        PNR_TRY(pnr_density_update(c, r));
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
    pnr::put(out_nodes, cap_nodes, out);
    pnr::put(out_links, cap_nodes, par.data(), *n_out_nodes); // (one parent per node)
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
