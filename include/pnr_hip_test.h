/*
 * pnr_hip_test.h -- TEST TAPS of libpnr_hip.so.  Not part of the drop-in boundary (include/pnr_hip.h): nothing a host of the
 * reference's pipeline calls.  These entry points expose single stages of the device code so that tests/ can compare them with the
 * oracle and with the reference-generated fixtures (tests/golden/), and let the multi-process tests drive the scheduler with a
 * host engine.  Same conventions as pnr_hip.h (int status, pnr_last_error()); file:line = /root/reference/pnr-vaa3d/.
 */
#ifndef PNR_HIP_TEST_H
#define PNR_HIP_TEST_H
#include "pnr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test taps: Frangi::imgaussian (frangi.cpp:647) and Frangi::hessian3d (:291) for one sigma.
 * Host outputs, N floats each; Hessian order Dzz,Dyy,Dyz,Dxx,Dxy,Dxz (any may be NULL). */
int pnr_gaussian(pnr_ctx *ctx, float sig, float *F);
int pnr_hessian(pnr_ctx *ctx, float sig, float *Dzz, float *Dyy, float *Dyz, float *Dxx, float *Dxy, float *Dxz);
/* Feed externally produced J8/V (host, N each) instead of pnr_frangi's: lets extractSeeds be
 * tested in isolation exactly like SeedExtractor::extractSeeds(tolerance,J8,...,Vx,Vy,Vz). */
int pnr_set_j8_v(pnr_ctx *ctx, const uint8_t *J8, const uint8_t *Vx, const uint8_t *Vy, const uint8_t *Vz);
/* pnr_get_frangi of the box lo <= (z, y, x) < hi alone (lo, hi: three values each, z first): the same volumes in HBM, with the same
 * exact re-run first where J or a direction volume is asked for after a pruned run, but only the box is copied, into dense host arrays
 * of (hi[0] - lo[0]) x (hi[1] - lo[1]) x (hi[2] - lo[2]) elements (any may be NULL).  For stacks whose whole f32 J a test cannot
 * afford to download (above 2^31 voxels: 9 GB). */
int pnr_get_frangi_box(pnr_ctx *ctx, const int64_t *lo, const int64_t *hi, float *J, uint8_t *J8, uint8_t *Vx, uint8_t *Vy, uint8_t *Vz);

/* What the GPU half of pnr_extract_seeds_range hands to the host's flood fill for the layers [z0, z1) of the context's J8 (same
 * argument rules), nl = z1 - z0 layers: the stage runs as it does there (extremes, bitmap and row counts, row prefix, keys and
 * compacted values, the chunked download on the second stream), then both streams are waited for.  Per layer: vmin / vmax [nl] the
 * extremes as the device computed them; ltot [nl] the pixels above the minimum; key_off [nl + 1] and keys, the candidate keys
 * ((int)((v - vmin) * vFactor) << 32 | y * w + x, seed.cpp:616-632) sorted ascending inside each layer -- *n_keys receives their
 * number, they are written only if it is <= cap_keys (*n_keys > cap_keys: call again); layers [nl][h][w] the layer as the fill's own
 * loader rebuilds it from the downloaded bits and values; restored [nl] 1 where the loader's image is uniformly the layer minimum
 * again after its restore step (one loader takes all the layers in turn, as a fill thread does: a pixel a restore misses shows in
 * the next layer as well).  Any output may be NULL.  Neither the seed list of the context nor a later pnr_extract_seeds changes. */
int pnr_seed_handover(pnr_ctx *ctx, int64_t z0, int64_t z1, int32_t *vmin, int32_t *vmax, int64_t *ltot, int64_t *key_off,
                      int64_t *keys, int64_t cap_keys, int64_t *n_keys, uint8_t *layers, int32_t *restored);

/* The likelihood half of one step of the phased SMC driver (smc_phased.hip) over nt traces whose poses the caller gives, all in one
 * step list: the placement, fast words and duplicate search of ph_predict (compiled in a form that takes the particles as they are
 * instead of drawing them), ph_cube (option "cube_copy"), ph_sample and ph_sums, launched as a production step of nt traces launches
 * them, with the context's options "split_x10", "max_split", "cube_copy", "sums_deep", "share_scales", "share_min".  np = the
 * context's particle count, S its number of scales, np_pad = (np + 1 + 63) / 64 * 64.
 *   poses [nt][np][6] the particles (x, y, z, vx, vy, vz), exact duplicates allowed; centroids [nt][6] the pending centroid;
 *   modes [nt]: PNR_PHL_FIRST no pending centroid, as at iteration 0 (the closing chain reads zeros; centroids[j] is not used),
 *               PNR_PHL_REGULAR particles and centroid, PNR_PHL_TAIL the centroid only (one chain; poses[j] is not used).
 * NaN and out-of-volume poses are legal, as in a trace.  Outputs (host, any may be NULL): corr [nt][S][np_pad] the correlation per
 * scale and CHAIN (0 beyond a trace's chains); uidx [nt][np_pad] chain -> particle (np = the centroid, which closes the list; -1
 * beyond); cmap [nt][np_pad] particle -> chain (-1 beyond np, and in a tail pass); flags [nt][PNR_PHL_FLAGS] the trace's flag words
 * (PNR_PHL_OX.. below); info [8]: np_pad, S, sampling work-groups per trace, 1 if guest scales read their hosts' stash, 1 for the
 * deep form of the sums, 1 if ph_cube ran, chain groups per trace of the sums launch, rounds the traces were evaluated in (1 unless
 * the sample stash does not hold them all; the forms are those of the first round).
 * PNR_E_ARG: nt < 1, no volume, not the phased driver, ni < 2, a mode out of range. */
enum { PNR_PHL_FIRST = 0, PNR_PHL_REGULAR = 1, PNR_PHL_TAIL = 2 };
enum { PNR_PHL_FLAGS = 16,                   /* words per trace; those the step's likelihood half writes: */
       PNR_PHL_OX = 5, PNR_PHL_OY = 6, PNR_PHL_OZ = 7, /* the cube's origin in the volume */
       PNR_PHL_Y0 = 8, PNR_PHL_Y1 = 9, PNR_PHL_Z0 = 10, PNR_PHL_Z1 = 11, /* rows / planes of the cube that are staged: [y0, y1) x [z0, z1) */
       PNR_PHL_FAST = 12,                    /* bit s: all templates of scale s inside cube and volume; bit 8 + s: inside the volume */
       PNR_PHL_NCH = 13 };                   /* chains: distinct particle poses + 1 (1 in a tail pass) */
int pnr_phased_likelihood(pnr_ctx *ctx, int64_t nt, const float *poses, const float *centroids, const int32_t *modes, float *corr,
                          int32_t *uidx, int32_t *cmap, int32_t *flags, int32_t *info);

/* The decision half of one step of the phased SMC driver over nt traces whose whole state the caller gives, all in the step list
 * `lp`: ph_update (pending centroid and its stop test, maximum over the scales, weights, N_eff, CDF, centroid, stop tests, systematic
 * resampling, the hand-over into the next list), then ph_predict of the FOLLOWING step on the list ph_update filled (the drawing of
 * the next particles, priors, duplicate search) -- the production kernels with the launch parameters of a production step, every
 * trace at its own iteration.  np, S, ni, Kc, znccth, neff_ratio, nodepervol = the context's; np_pad = (np + 1 + 63) / 64 * 64.
 * Inputs, in the device's layout (host arrays):
 *   flags [nt][PNR_PHL_FLAGS]: PNR_PHL_IT the trace's iteration (0..ni), PNR_PHL_RES whether the step before resampled, PNR_PHL_STOP /
 *     PNR_PHL_T / PNR_PHL_PAUSE on entry, PNR_PHL_NCH the chains of corr (the centroid's is the last); seeds [nt][6];
 *   part [nt][2][np][9]: half it & 1 the particles of the iteration (x, y, z, vx, vy, vz, then w, corr, sig), the other half those of
 *     it - 1; prior [nt][np]; idxres [nt][np] the resampling of the step before (0..np-1 each, read only with PNR_PHL_RES);
 *   xcs [nt][2][8]: half (it & 1) ^ 1 the pending centroid; corr [nt][S][np_pad] the GIVEN correlations per scale and chain, cmap
 *     [nt][np_pad] particle -> chain (several particles may share one); draws [np + 1] instead of the context's rand() stream, or
 *     NULL; den [w * h * l] a density map for the DENSITY stop, or NULL for none.
 * Outputs (host, any may be NULL), after ph_update: part_u, xcs_u, idxres_u, prior_u, flags_u as the inputs; neff [nt][ni] (row it;
 * 0 where not written); oxc [nt][ni][8] the records of the pending iterations (0 elsewhere); oT / ostop [nt] (-1 where not written);
 * cnt_next and list_next [nt] the next step's list (-1 beyond).  After ph_predict: part_p, prior_p, flags_p, uidx [nt][np_pad] (-1
 * where not written), cmap_p (the same), cnt_p [2] both list counters.
 * mode PNR_PHD_PREDICT runs ph_predict alone, on the list `lp` and at the traces' own iterations -- the only way to iter0New's draw,
 * which no ph_update precedes: the outputs after ph_update are then not written.
 * PNR_E_ARG: nt < 1 or more traces than the state holds, no volume, not the phased driver, lp, mode, an iteration, a chain count, a
 * chain or a resampling index out of range. */
enum { PNR_PHD_STEP = 0, PNR_PHD_PREDICT = 1 };
enum { PNR_PHL_RES = 0, PNR_PHL_STOP = 1, PNR_PHL_T = 2, PNR_PHL_IT = 3, PNR_PHL_DONE = 4, PNR_PHL_PAUSE = 14 };
typedef struct {
    const int32_t *flags; const float *seeds, *part, *prior; const int32_t *idxres; const float *xcs, *corr; const int32_t *cmap;
    const uint32_t *draws; const uint8_t *den; int32_t lp, mode;
} pnr_phd_in;
typedef struct {
    float *part_u, *neff, *xcs_u, *oxc; int32_t *oT, *ostop, *idxres_u; float *prior_u; int32_t *flags_u, *cnt_next, *list_next;
    float *part_p, *prior_p; int32_t *flags_p, *uidx, *cmap_p, *cnt_p;
} pnr_phd_out;
int pnr_phased_decide(pnr_ctx *ctx, int64_t nt, const pnr_phd_in *in, pnr_phd_out *out);

/* Tracker tables for parity tests: name in {"p","u","w0","w0_cws","v","w","w_cws","rng",
 * "model_vuw<s>","model_wgt<s>","model_avg","gauss_xy<s>","gauss_z<s>","scale_share"}.  Copies up to cap
 * 4-byte words into out; *n receives the element count.  "scale_share" (int32): [0, 8) the scale whose stash scale s reads under
 * option "share_scales" (its host; -1: s samples on its own), [8, 16) s's first entry in the row table. */
int pnr_get_table(pnr_ctx *ctx, const char *name, void *out, int64_t cap, int64_t *n);

/* expf used for the particle likelihood exp(Kc*corr) (tracker.cpp:1029,1136), exposed so the
 * tests can compare the device implementation with the host libm over many inputs. */
int pnr_expf_batch(pnr_ctx *ctx, const float *x, int64_t n, float *y);

/* Frangi::eigen_decomposition (frangi.cpp:1269-1306: tred2 :1309, tql2 :1390, the |lambda| re-sort :1286-1304) of n symmetric
 * 3 x 3 matrices through the DEVICE solver (frangi.hip eigen3), host arrays of row-major doubles: A [n][3][3] in, d [n][3] the
 * eigenvalues by ascending |lambda|, V [n][3][3] the eigenvectors in columns (column 0 = the axis direction, sign as the solver
 * leaves it).  V == NULL runs the eigenvalues-only form that the vesselness kernel (eigen_queue) compiles; V != NULL the full solver
 * of the direction kernel (vdir_points). */
int pnr_eigen_batch(pnr_ctx *ctx, const double *A, int64_t n, double *V, double *d);

/* The scheduler behind pnr_trace_replay[_sharded] (stream_sched.h) over a HOST engine that plays back map-free traces which
 * `trace(user, pos_dir[6], &T, xc[ni])` supplies (0 = ok; rows 0..min(T, ni)-1 of xc valid) -- pure host code, no GPU: the
 * multi-process tests drive the window / admission / exchange / replay logic with it, and a recorded workload can be
 * re-scheduled offline.  Same outputs as pnr_trace_replay_sharded.  look0 / look_pct: the admission lookahead (options of the same
 * name; 0 / -1 = automatic). */
typedef int (*pnr_trace_fn)(void *user, const float *pos_dir, int32_t *T, pnr_xest *xc);
int pnr_sched_playback(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n, int rank,
                       int world, pnr_allgather_fn exchange, void *exchange_user, int64_t block_bytes, pnr_trace_fn trace,
                       void *trace_user, int window, int groups, int poll, int look0, int look_pct, pnr_node *nodes, int64_t cap_nodes,
                       int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used,
                       int64_t *n_iterations_here);

/* The same with the scheduler's tentative replay switched on or off (pnr_sched_playback: on, as in pnr_trace_replay[_sharded]; option
 * "tentative"), the number of running traces the admission keeps up (option "target"; -1 = automatic, 0 = off) and the steps of a poll
 * that run on while the host works (option "lag"; -1 = automatic): results are identical either way, only the number of iterations run differs. */
int pnr_sched_playback2(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n, int rank,
                        int world, pnr_allgather_fn exchange, void *exchange_user, int64_t block_bytes, pnr_trace_fn trace,
                        void *trace_user, int window, int groups, int poll, int look0, int look_pct, int tentative, int target, int lag,
                        pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links,
                        int64_t *n_traces_used, int64_t *n_iterations_here);

/* pnr_reconstruct_stage with the device stages of pnr_reconstruct_ctx: the list behind stage 2 (_n1_, after the mean-shift) and
 * stage 3 (_n2_, after the grouping) can be compared with the host's one stage at a time.  Same arguments and rules otherwise. */
int pnr_reconstruct_stage_ctx(pnr_ctx *ctx, const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links,
                              float trace_rsmpl, float sig2radius, int refine_iter, float epsilon2, float group_radius, int stage,
                              pnr_node *out_nodes, int64_t cap_nodes, int64_t *n_out_nodes, int32_t *out_links, int64_t cap_links,
                              int64_t *n_out_links);

/* The shells of pnr_measure_radii's rule for (zdist, rmax, 2-D) as the device reads them, pure host code (no GPU): shell k =
 * entries [starts[k], starts[k + 1]) of dx / dy / dz, k = 0..rmax (starts: rmax + 2 entries; raster order inside a shell).  *n = the
 * number of offsets; up to cap of them are written; any array may be NULL. */
int pnr_radius_offsets(float zdist, int rmax, int is2d, int32_t *starts, int32_t *dx, int32_t *dy, int32_t *dz, int64_t cap, int64_t *n);

/* The launch plan of the all-pairs minimum behind pnr_point_segment_distance (n points x m segments) and pnr_nearest_other /
 * pnr_join_trees (n x n), pure host code (no GPU): the launches in their order, rows outer, 7 values each -- points [p0, p1), segments
 * or targets [s0, s1), the slice length `split`, the grid (x, y).  split / budget: the options *_split / *_pairs_per_launch (0 =
 * automatic).  *count = the number of launches; up to cap of them are written to tiles (cap x 7; NULL with cap = 0). */
int pnr_pair_tiles(int64_t n, int64_t m, int64_t split, int64_t budget, int64_t *tiles, int64_t cap, int64_t *count);

/* The work items of pnr_render_tree / pnr_tree_coverage for a tree on the grid w x h x l, pure host code (no GPU, no context): 7 values
 * each -- the segment, then the inclusive box x0, y0, z0, x1, y1, z1 (inside the grid) -- in segment order.  piece / box: the options
 * render_piece / render_box (0 = automatic).  Same argument rules as pnr_render_tree.  *count = the number of items; up to cap of them
 * are written to items_out (cap x 7; NULL with cap = 0): *count > cap: call again. */
int pnr_render_items(const float *xyz, const float *radius, const int32_t *parent, int64_t n, int64_t w, int64_t h, int64_t l, const pnr_render_opts *opts,
                     int64_t piece, int64_t box, int64_t *items_out, int64_t cap, int64_t *count);

/* The host's volume writer (pnr_amd/host/stack_io.h save_stack_u8), pure host code: img (w*h*l bytes, x fastest) as a multi-page
 * uncompressed 8-bit TIFF, or the bare bytes for a name ending in .raw; written to a temporary file, then renamed.  A file that would
 * pass classic TIFF's 4 GiB is refused from the dimensions alone (PNR_E_ARG, nothing is written; img may then be NULL). */
int pnr_test_write_tiff(const char *path, const uint8_t *img, int64_t w, int64_t h, int64_t l);

/* The kernels behind pnr_auto_threshold and pnr_local_threshold on bytes of any size, also below the 2 x 2 x 1 a context takes as its
 * volume (threshold.hip).  pnr_test_histogram: hist[256] = the histogram of the n host bytes (1 to 2^32), copied to device memory `offset`
 * (0..15) bytes past a 16-byte boundary.  pnr_test_local_threshold: the rule of pnr_local_threshold on the host volume vol (w x h x l, sides
 * from 1, x fastest; zdist is the context's) into out (w h l host bytes); opts as there.  The context's own volume is neither needed nor
 * touched. */
int pnr_test_histogram(pnr_ctx *ctx, const uint8_t *bytes, int64_t n, int32_t offset, uint64_t *hist);
int pnr_test_local_threshold(pnr_ctx *ctx, const uint8_t *vol, int64_t w, int64_t h, int64_t l, const pnr_local_opts *opts, pnr_local_info *info /* nullable */,
                             uint8_t *out);

/* Bytes of device and of pinned host memory the library holds at this moment, over all contexts and exchanges of the process
 * (every allocation goes through one owner type that counts them); either pointer may be NULL. */
int pnr_live_bytes(int64_t *device, int64_t *pinned);

#ifdef __cplusplus
}
#endif
#endif /* PNR_HIP_TEST_H */
