/*
 * pnr_hip.h -- C ABI of the MI355X (gfx950) implementation of the PNR / Advantra hot path:
 * multi-scale Frangi vesselness -> J8 -> per-layer seed extraction -> ZNCC seed scoring ->
 * batched SMC particle tracing -> host replay of the trace bookkeeping.
 *
 * This is the drop-in boundary: plain C types, no exceptions, no torch types.  Every entry
 * point names the reference interface it replaces (file:line relative to
 * /root/reference/pnr-vaa3d/).  The reference has no FFI of its own (it is one C++ plugin);
 * the call sites a maintainer re-points are Advantra_plugin.cpp:2488-2497 (Frangi),
 * :2499-2512 (J8), :2549 (extractSeeds), :2561-2586 (seed filter/sort), :2658-2710 (trace loop).
 * INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PNR_E_* code on failure;
 *     pnr_last_error() returns a thread-local message for the last failure.
 *   - volumes are uint8, x fastest: i = z*w*h + y*w + x (frangi.cpp:307); 16-bit and multi-channel stacks are windowed to
 *     8 bits on the GPU by pnr_set_volume_u16.
 *   - one pnr_ctx = one GPU = one host thread at a time (the reference is single-threaded).
 *   - the library FAILS (PNR_E_NODEVICE) when no HIP device is present: there is no CPU path.
 */
#ifndef PNR_HIP_H
#define PNR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNR_MAX_SIGMAS 8

enum {
    PNR_OK = 0,
    PNR_E_ARG = -1,      /* invalid argument / parameter out of range */
    PNR_E_NODEVICE = -2, /* no HIP device / device init failed */
    PNR_E_HIP = -3,      /* HIP runtime error (message has the call) */
    PNR_E_STATE = -4,    /* call order violated (e.g. seeds before frangi) */
    PNR_E_NOMEM = -5
};

/* input_PARA (Advantra_plugin.cpp:88-103) + the hard-wired constants of :63-83 */
typedef struct pnr_params {
    float sig[PNR_MAX_SIGMAS]; /* neuritesigmas, ascending (parse_csv_string :1885-1897) */
    int nsig;
    int somaradius;  /* > 0: soma path, call pnr_soma after pnr_set_volume (Advantra_plugin.cpp:2426-2448) */
    float tolerance; /* MaximumFinder tolerance on J8 */
    float znccth;
    float kappa;
    int step;
    int ni; /* SMC iterations per trace direction */
    int np; /* particles */
    float zdist;
    int nodepervol;
    int vol; /* 1,5,9,11,19,27 */
    float Kc;         /* 20   (:63) */
    float neff_ratio; /* 0.8  (:64) */
    float alpha;      /* 0.5  frangi_alfa (:66) */
    float beta;       /* 0.5  frangi_beta (:67) */
    float C;          /* 500  frangi_C    (:68) */
    uint32_t rng_seed;    /* replaces srand(time(NULL)) of tracker.cpp:1003,1098 */
    int max_trace_count;  /* 5000 MAX_TRACE_COUNT (:72) */
} pnr_params;

/* struct seed (seed.h:33-39) */
typedef struct pnr_seed {
    float x, y, z, vx, vy, vz, score, corr;
} pnr_seed;

/* struct X_est (tracker.h:19-23) */
typedef struct pnr_xest {
    float x, y, z, vx, vy, vz, sig, corr;
} pnr_xest;

/* class Node without its nbr vector (node.h:5-44); links are returned separately */
typedef struct pnr_node {
    float x, y, z, vx, vy, vz, corr, sig;
    int32_t type; /* node.cpp:14-21: AXON=2, END=6, UNDEFINED=7 */
} pnr_node;

typedef struct pnr_ctx pnr_ctx;

const char *pnr_last_error(void);
void pnr_default_params(pnr_params *p); /* README.md:17 example + plugin constants */

/* Validates like Advantra::dofunc (Advantra_plugin.cpp:317-326) and builds the Tracker tables
 * (Tracker::Tracker, tracker.cpp:79-527) on the host, uploads them.  device = HIP ordinal. */
int pnr_create(const pnr_params *p, int device, pnr_ctx **out);
void pnr_destroy(pnr_ctx *ctx);

/* Use an externally owned HIP stream (e.g. torch's current stream); NULL = ctx's own stream. */
int pnr_set_stream(pnr_ctx *ctx, void *hip_stream);
int pnr_synchronize(pnr_ctx *ctx);

/* data1d + in_sz of reconstruction_func (Advantra_plugin.cpp:2241-2255).  Host pointer is
 * borrowed for the call and copied to HBM; the _device variant borrows a device pointer that
 * must stay valid until the next set_volume/destroy (no copy).  l == 1 (a single slice) selects the reference's 2-D mode:
 * Frangi::frangi2d (frangi.cpp:392) and the is2d branches of the tracker (Advantra_plugin.cpp:2496-2497, :2526); the tracker
 * tables are rebuilt whenever the dimensionality changes.  2-D stacks are traced by the phased SMC driver only. */
int pnr_set_volume(pnr_ctx *ctx, const uint8_t *img, int64_t w, int64_t h, int64_t l);
int pnr_set_volume_device(pnr_ctx *ctx, const void *dev_img, int64_t w, int64_t h, int64_t l);

/* 16-bit input (12- / 16-bit microscope stacks, one or several interleaved channels).  The reference traces 8-bit data only
 * (channel c of what Vaa3D loaded, as unsigned char; frangi_C = 500 assumes 0-255 Hessian magnitudes), so a deeper stack is not
 * traced as it is: the selected channel is windowed to 8 bits on the GPU, by the conversion a user would otherwise make by hand,
 * and everything after it is the 8-bit pipeline.  Let x be the N samples of the channel (voxel i = element i * nchan + channel of
 * img) and s = x sorted ascending.
 *   window [lo, hi]: given (0 <= lo < hi <= 65535), or from the stack (lo = hi = -1): lo = s[k_lo], hi = s[k_hi] with
 *     k_lo = floor(N * sat_lo_ppm / 1e6), k_hi = N - 1 - floor(N * sat_hi_ppm / 1e6) (exact integers; sat_lo_ppm + sat_hi_ppm < 1e6);
 *     win = NULL = {-1, -1, 0, 0} = [min, max];
 *   mapping: hi > lo: out = (510 a + d) div 2d with a = clamp(v, lo, hi) - lo, d = hi - lo (255 a / d rounded half up: 0 at lo, 255
 *     at hi); hi == lo (a constant stack): 255 where v > lo, else 0.
 * Afterwards the context is what pnr_set_volume of the mapped bytes leaves (l == 1 selects the 2-D mode), the window used is
 * returned in lo_out / hi_out (nullable), and pnr_get_volume reads the bytes back.  The host variant copies img (nchan * N
 * samples) into a device buffer of the call; the device variant reads dev_img during the call only (it does not borrow it).  The
 * work runs on the context's stream (kernel times: group "volume").  PNR_E_ARG (nchan < 1, channel outside [0, nchan), a bad window,
 * sat_lo_ppm + sat_hi_ppm >= 1e6): the previous volume is kept; PNR_E_NOMEM: the context has no volume. */
typedef struct pnr_window {
    int32_t lo, hi;                 /* 0 <= lo < hi <= 65535: this window; lo = hi = -1: from the stack, by: */
    int32_t sat_lo_ppm, sat_hi_ppm; /* voxels clipped to 0 / to 255, parts per million of the channel's voxels */
} pnr_window;                       /* NULL = {-1, -1, 0, 0} = [min, max] */
int pnr_set_volume_u16(pnr_ctx *ctx, const uint16_t *img, int64_t w, int64_t h, int64_t l, int nchan, int channel,
                       const pnr_window *win, int32_t *lo_out, int32_t *hi_out);
int pnr_set_volume_u16_device(pnr_ctx *ctx, const void *dev_img, int64_t w, int64_t h, int64_t l, int nchan, int channel,
                              const pnr_window *win, int32_t *lo_out, int32_t *hi_out);
/* the 8-bit volume the context traces (owned or borrowed): N = w*h*l bytes */
int pnr_get_volume(pnr_ctx *ctx, uint8_t *img);

/* Frangi::frangi3d (frangi.cpp:152-289; called at Advantra_plugin.cpp:2496) followed by the
 * J -> J8 rule (:2499-2512).  Results stay in HBM; Jmin/Jmax are returned. */
int pnr_frangi(pnr_ctx *ctx, float *Jmin, float *Jmax);
/* z-slab sharding of Frangi / seed extraction over several GPUs: the context's volume is a slab of the stack WITH a
 * halo of ceil(3*sigma_max/zdist) + 2 planes on every cut side (the z pass of the Gaussian plus the radius-2 Hessian stencil), so
 * that the planes [z_keep0, z_keep1) of the slab are exactly what the whole stack would give.  pnr_frangi_slab runs every scale and
 * returns Jmin / Jmax over the kept planes only; after the ranks have reduced them to the global extremes, pnr_quantise_j8 applies
 * the J -> J8 rule (Advantra_plugin.cpp:2499-2512) and pnr_extract_seeds_range(z_keep0, z_keep1) gives the slab's seeds. */
int pnr_frangi_slab(pnr_ctx *ctx, int64_t z_keep0, int64_t z_keep1, float *Jmin, float *Jmax);
int pnr_quantise_j8(pnr_ctx *ctx, float Jmin, float Jmax);

/* Optional read-back of the Frangi outputs (any pointer may be NULL); N = w*h*l each.  J8 is always what pnr_frangi left in HBM.
 * With option frangi_prune (default 1) pnr_frangi skips the eigen-solver where the response provably cannot reach the first
 * non-zero J8 level: J8, Jmin / Jmax and everything at voxels with J8 > 0 (all seeds) are exact, but the f32 J and the winning
 * scale of J8 = 0 voxels are not -- so asking for J or for the direction volumes first recomputes the response without that
 * shortcut (one more pnr_frangi worth of GPU time; tests and diagnostics), and so does pnr_quantise_j8 when it is given extremes
 * the shortcut did not assume (Jmin other than 0, or a Jmax below the run's own maximum; the global extremes of a sharded stack
 * never are). */
int pnr_get_frangi(pnr_ctx *ctx, float *J, uint8_t *J8, uint8_t *Vx, uint8_t *Vy, uint8_t *Vz);
/* SeedExtractor::extractSeeds (seed.cpp:556-791; Advantra_plugin.cpp:2549).  Library-owned
 * array, valid until the next call or pnr_destroy.  z-major, value-descending-per-layer order. */
int pnr_extract_seeds(pnr_ctx *ctx, const pnr_seed **seeds, int64_t *n);
/* Same, restricted to layers [z0, z1): the unit of multi-GPU Frangi/seed sharding. */
int pnr_extract_seeds_range(pnr_ctx *ctx, int64_t z0, int64_t z1, const pnr_seed **seeds, int64_t *n);

/* Tracker::znccBBB (tracker.cpp:1891-1964) for n (pos,dir) pairs: pos_dir = n x 6 floats. */
int pnr_zncc_batch(pnr_ctx *ctx, const float *pos_dir, int64_t n, float *corr, float *sig);

/* Seed filter + sort (Advantra_plugin.cpp:2561-2586): corr = znccBBB(seed); drop corr < znccth;
 * sort by corr descending (ties: original order).  In place; *n_out <= n. */
int pnr_score_filter_sort_seeds(pnr_ctx *ctx, pnr_seed *seeds, int64_t n, int64_t *n_out);
/* The same in two halves, for one stack on several GPUs: every rank scores and filters the seeds of its own z-slab (order kept),
 * the merged list -- in the z-major order of the unsharded extraction -- is then sorted on every rank: the result is the list
 * pnr_score_filter_sort_seeds gives on one GPU (the sort is stable, ties keep the z-major order). */
int pnr_score_filter_seeds(pnr_ctx *ctx, pnr_seed *seeds, int64_t n, int64_t *n_out);
int pnr_sort_seeds(pnr_ctx *ctx, pnr_seed *seeds, int64_t n, int64_t *n_out);

/* Map-independent part of Tracker::trackPos / trackNeg (tracker.cpp:819-933 -> iter0New :1001,
 * iterINew :1096) for n seeds x 2 directions, all on the GPU.  Trace j = 2*i + dir (dir 1 =
 * negated seed direction).  Outputs (host, caller-allocated):
 *   T    [2n]        successful iterations (= ti_limit of a run without density/soma maps)
 *   stop [2n]        0 = ni reached, 1 = left the volume, 2 = centroid corr < znccth
 *   xc   [2n*ni]     centroid estimates; rows 0..min(T,ni-1) are valid
 * Optional debug taps for the first dbg_iters iterations of every trace (NULL to skip):
 *   xfilt [2n*dbg_iters*np*9]  particles (x,y,z,vx,vy,vz,w,corr,sig) (struct X, tracker.h:13-17)
 *   idxres[2n*dbg_iters*np]    resampled indices, neff [2n*dbg_iters] */
int pnr_trace_batch(pnr_ctx *ctx, const pnr_seed *seeds, int64_t n, int32_t *T, int32_t *stop,
                    pnr_xest *xc, int dbg_iters, float *xfilt, int32_t *idxres, float *neff);

/* Host replay of the sequential bookkeeping (trackPos :848-931 + trace loop
 * Advantra_plugin.cpp:2658-2710) over map-free traces, in seed order.  Pure host integer work.
 *   nodes: capacity cap_nodes (node 0 = dummy, :2416-2419); links: pairs (a,b) meaning
 *   a.nbr.push_back(b); b.nbr.push_back(a) in push order.  Returns counts through pointers. */
int pnr_replay_traces(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds,
                      int64_t n, const int32_t *T, const pnr_xest *xc, pnr_node *nodes,
                      int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                      int64_t *n_links, int64_t *n_traces_used);

/* Soma path (params.somaradius > 0; Advantra_plugin.cpp:2426-2448 and soma_extraction1 :1899-1915): xy erosion
 * (Frangi::imerode, frangi.cpp:880), xy Gaussian of the u8 stack (Frangi::imgaussian, frangi.cpp:786), maxentropy_th
 * (toolbox.cpp:657), binarise at > threshold, conn3d (toolbox.cpp:245) -> one SOMA node (x, y, z, sig = mean radius,
 * corr = -FLT_MAX, type 1) per 26-connected region and the map voxel -> node index the seed filter, the replay and the
 * trace kernels' early stop use.  Must run after pnr_set_volume and before pnr_frangi (it uses the Frangi scratch) whenever
 * somaradius > 0; with somaradius = 0 it records "no soma".  E8 (nullable, N bytes) receives the eroded + blurred stack.  The call's
 * own device buffers (taps, histogram, row tables, the compacted voxels) are freed before it returns; PNR_E_NOMEM: an allocation failed. */
int pnr_soma(pnr_ctx *ctx, uint8_t *E8, int32_t *threshold, int64_t *n_soma);
/* soma nodes (in node-list order, index k+1) and the sparse label map: foreground voxels in raster order with their node index */
int pnr_get_soma(pnr_ctx *ctx, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int64_t *vox, int32_t *label,
                 int64_t cap_vox, int64_t *n_vox);
/* pnr_replay_traces with the context's dimensions, parameters and soma (the node list then starts dummy, somas, ...) */
int pnr_replay_traces_ctx(pnr_ctx *ctx, const pnr_seed *seeds, int64_t n, const int32_t *T, const pnr_xest *xc,
                          pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                          int64_t *n_links, int64_t *n_traces_used);

/* Production form of the trace loop (Advantra_plugin.cpp:2658-2710): trace + replay with early DENSITY stops.  The
 * node-density map produced by the replay of lower-ranked seeds is kept on the GPU, which ends a trace at the first
 * iteration whose centroid voxel is already saturated there (what the reference's DENSITY stop, tracker.cpp:855, would
 * do at the latest), and seeds on saturated voxels are not launched (:2669-2670).  The GPU map only holds replayed
 * nodes, so it only under-counts and the node graph is identical to pnr_trace_batch + pnr_replay_traces.
 * Phased driver (default): a window of traces is kept full, finished traces are replayed in seed order and their slots
 * handed to the next seeds (first_batch is ignored).  Persistent driver: seed-rank batches of first_batch seeds,
 * doubling up to 1024 (<= 0: default 128).  *n_iterations = SMC iterations run. */
int pnr_trace_replay(pnr_ctx *ctx, const pnr_seed *seeds, int64_t n, int64_t first_batch, pnr_node *nodes,
                     int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links, int64_t *n_links,
                     int64_t *n_traces_used, int64_t *n_iterations);

/* The node graph of the last pnr_trace_replay / pnr_trace_replay_sharded stays in the context: a caller whose buffers were too
 * small (n_nodes > cap_nodes) allocates and fetches it here instead of tracing again. */
int pnr_get_graph(pnr_ctx *ctx, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                  int64_t *n_links);

/* How every replayed trace of the last pnr_trace_replay[_sharded] ended -- what the reference prints per trace at
 * tracker.cpp:866,879,908,916 -- when the option "trace_log" is set: 5 ints per trace, in replay order:
 * {seed rank, direction (0 = trackPos, 1 = trackNeg), ti_limit, reason, value}; reason 0 = TRACK LIMIT (value: bits of the last
 * corr), 1 = success=0 (value: bits of the failing iteration's corr), 2 = DENSITY (value: nodepervol), 3 = SOMA (value: node). */
int pnr_get_trace_log(pnr_ctx *ctx, int32_t *rec, int64_t cap, int64_t *n);

/* ---- one stack, several GPUs: the sorted seeds sharded over `world` processes (one pnr_ctx per GPU; BASELINE configs[3]) ----
 * The reference has no distributed code; what is kept is the result of its sequential trace loop
 * (Advantra_plugin.cpp:2658-2710).  Rank r traces the seeds r, r + world, ... of the SAME sorted list in its own window of trace
 * slots; after every poll the ranks all-gather the records of the traces that finished (one fixed-size block per rank) and every
 * rank replays them in global seed order, so that every GPU's density map holds the replayed nodes of all ranks: the early
 * DENSITY stops (tracker.cpp:855) and the seed skip rule (:2669-2670) work as on one GPU and every rank returns the same node
 * graph -- the graph of pnr_trace_replay on one GPU.
 *
 * The transport is the host's: `exchange(user, send, recv, bytes)` must behave like an all-gather of `bytes` bytes per rank
 * (recv = world x bytes, rank order) over whatever joins the processes -- RCCL / torch.distributed (pnr_amd/multigpu.py), MPI, a
 * thread barrier in tests -- and return 0.  It is called once per poll by every rank, the same number of times on all of them.
 * A rank that fails says so in one last exchange, so the others return PNR_E_STATE instead of waiting for it. */
typedef int (*pnr_allgather_fn)(void *user, const void *send, void *recv, int64_t bytes_per_rank);
int pnr_trace_replay_sharded(pnr_ctx *ctx, const pnr_seed *seeds, int64_t n, int rank, int world, pnr_allgather_fn exchange,
                             void *user, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links,
                             int64_t cap_links, int64_t *n_links, int64_t *n_traces_used, int64_t *n_iterations_here);

/* A ready-made exchange for ranks that share ONE host (the 8 GPUs of a node): an all-gather through POSIX shared memory.  The
 * records being exchanged live in pinned host memory and are consumed by the host replay, so a host-side transport saves the
 * host -> device -> xGMI -> device -> host round trip of a device collective (a few microseconds per exchange).  `name` must be the
 * same on all ranks and unique to the job; rank 0 creates the segment, the call returns when all `world` ranks are attached.
 * Pass pnr_shm_allgather as `exchange` and the handle as `user`.  capacity_bytes >= the largest block ever exchanged. */
typedef struct pnr_shm_exchange pnr_shm_exchange;
int pnr_shm_exchange_open(const char *name, int rank, int world, int64_t capacity_bytes, pnr_shm_exchange **out);
int pnr_shm_allgather(void *user, const void *send, void *recv, int64_t bytes_per_rank);
void pnr_shm_exchange_close(pnr_shm_exchange *x);

/* The same collectives over RCCL (xGMI between the GPUs of a node, the network across nodes) for hosts that are not Python
 * (advantra_cli --ranks N --exchange rccl; pnr_amd/multigpu.py reaches RCCL through torch.distributed instead): an ncclAllGather of one
 * fixed-size block per rank -- pass pnr_rccl_allgather as `exchange` and the handle as `user` -- and the 2-float all-reduce of
 * (Jmin, Jmax) of the z-slab Frangi (one ncclAllReduce(ncclMax) over (-min, max)).  The payloads are host data: every call stages
 * through pinned host memory and a device buffer on the exchange's own stream.  One rank calls pnr_rccl_unique_id and hands the 128
 * bytes to the others by any means (advantra_cli: the shared-memory segment; across nodes: the launcher); every rank then opens the
 * exchange with ITS device -- a collective call, one rank per GPU (RCCL refuses two ranks on one device).  librccl is opened at run
 * time, when the first of these calls is made; without it they fail with PNR_E_STATE.  capacity_bytes >= the largest block. */
typedef struct pnr_rccl_exchange pnr_rccl_exchange;
int pnr_rccl_unique_id(void *id128);
int pnr_rccl_exchange_open(const void *id128, int rank, int world, int device, int64_t capacity_bytes, pnr_rccl_exchange **out);
int pnr_rccl_allgather(void *user, const void *send, void *recv, int64_t bytes_per_rank);
int pnr_rccl_allreduce_minmax(pnr_rccl_exchange *x, float *min_inout, float *max_inout);
void pnr_rccl_exchange_close(pnr_rccl_exchange *x);

/* reconstruct() chain of the plugin (Advantra_plugin.cpp:2096-2181), pure host: link resampling
 * (TRACE_RSMPL) -> mean-shift refinement (SIG2RADIUS, REFINE_ITER, EPSILON2) -> sphere grouping (GROUP_RADIUS) ->
 * BFS trees -> drop trees < TREE_SIZE_MIN -> tree resampling.  Input: the node graph of pnr_trace_replay /
 * pnr_replay_traces.  Output: the tree list save_nodelist writes (node 0 dummy; parent -1 = root).  Values <= 0
 * select the plugin constants (1.0, 1.5, 4, 1e-4, 2.0, 10) -- except tree_size_min < 0, which selects the plugin's ENFORCE_SINGLE_TREE
 * branch (:81, :2142-2152): only the largest tree is kept (extract_largest_tree :546-589; the plugin names that file _Advantra1.swc). */
int pnr_reconstruct(const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                    float sig2radius, int refine_iter, float epsilon2, float group_radius, int tree_size_min,
                    pnr_node *out_nodes, int32_t *out_parent, int64_t cap, int64_t *n_out);

/* The same chain with its two neighbour stages -- the mean-shift refinement and the ball queries of the sphere grouping -- on
 * ctx's GPU (on its stream, see pnr_set_stream; device buffers are allocated per call and freed before it returns).  Same
 * arguments, defaults, tree_size_min < 0 branch, link validation and "*n_out > cap: call again" rule as pnr_reconstruct, and
 * identical output, byte for byte.  refine_iter above PNR_RECON_MAX_ITER is rejected (PNR_E_ARG); a failed device allocation
 * returns PNR_E_NOMEM.  Kernel times: pnr_get_kernel_ms group "recon". */
#define PNR_RECON_MAX_ITER 1000
int pnr_reconstruct_ctx(pnr_ctx *ctx, const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                        float sig2radius, int refine_iter, float epsilon2, float group_radius, int tree_size_min,
                        pnr_node *out_nodes, int32_t *out_parent, int64_t cap, int64_t *n_out);

/* The plugin's saveMidres taps inside reconstruct() (:2098-2141): the node list as it stands behind stage 1 = interpolate_nodelist
 * (_n0res_), 2 = non_blurring (_n1_), 3 = group1 (_n2_), 4 = compute_trees (_n2tree_).  out_links: pairs, every undirected link once
 * (stage 4: (child, parent)); counts are returned even when the buffers are too small. */
int pnr_reconstruct_stage(const pnr_node *nodes, int64_t n_nodes, const int32_t *links, int64_t n_links, float trace_rsmpl,
                          float sig2radius, int refine_iter, float epsilon2, float group_radius, int stage, pnr_node *out_nodes,
                          int64_t cap_nodes, int64_t *n_out_nodes, int32_t *out_links, int64_t cap_links, int64_t *n_out_links);

/* Node radii measured from the image (beyond the reference, whose SWC radius is SIG2RADIUS * the winning Frangi scale: two to four
 * values in all).  For n positions (x, y, z; f32, voxel indices as in pnr_node) the radius of the largest anisotropy-aware ball
 * around the position that is foreground, in whole xy voxels.  THE RULE (the contract; tests restate it in numpy).  Inputs: V, the
 * context's traced u8 volume (w x h x l, owned or borrowed; for 16-bit input the windowed bytes), zd = params.zdist, the options
 * {thr, rel_pct, rmax, bg_permille}.  All arithmetic is exact integer arithmetic unless marked f32; f32 operations are single IEEE
 * operations (-ffp-contract=off).
 *   Centre: per coordinate v with its extent n: c = (int) fminf(fmaxf(v + 0.5f, 0.f), (float)(n - 1)).  A position with any
 *     non-finite coordinate is not measured: k_out = -1.
 *   Shells: for integer offsets (dx, dy, dz) the f32 distance d2 = (float)(dx*dx + dy*dy) + (zd*(float)dz) * (zd*(float)dz).
 *     O_0 = {(0,0,0)}; O_k = {(dx,dy,dz) : (float)((k-1)*(k-1)) < d2 <= (float)(k*k)}, k = 1..rmax; in the 2-D mode (l == 1) only
 *     dz = 0 occurs.  Radii are therefore in xy-voxel units.  Voxels outside the volume are not counted at all, neither as total
 *     nor as background: a node at a face is measured on the part of the ball that exists.
 *   Threshold t: rel_pct == 0: t = thr; thr == -1: t = max(1, floor(sum(V) / N)), the global mean from the exact u64 sum.
 *     rel_pct in 1..100: per node t = max(1, ceil(rel_pct * m / 100)), m = the maximum of V over the in-volume voxels of
 *     O_0 u O_1 around c (thr is ignored).  A voxel is background when V < t.
 *   Radius: tot_k, bg_k = the in-volume voxels, and the background voxels among them, of O_0 u ... u O_k around c.  k* = the
 *     largest k in [0, rmax] such that 1000 * bg_j <= bg_permille * tot_j (64-bit products) holds for every j in 0..k; if it fails
 *     at j = 0 or j = 1, k* = 0.  k_out = k*.
 * Arguments (anything else: PNR_E_ARG): rmax 1..PNR_RADIUS_MAX, thr -1..255, rel_pct 0..100, bg_permille 0..999; opts = NULL =
 * {thr -1, rel_pct 50, rmax 32, bg_permille 1}; 0 <= n <= PNR_RADIUS_MAX_N (n = 0 is valid).  No volume in the context:
 * PNR_E_STATE.  thr_used (nullable) receives t of the absolute mode, 0 in the relative mode.  The call needs neither Frangi nor
 * seeds to have run and leaves the pipeline state of the context alone; it runs on the context's stream (pnr_set_stream), keeps the
 * shell table of (rmax, zdist, 2-D) on the device for the next call and frees every other device buffer before it returns
 * (PNR_E_NOMEM: an allocation failed).  Kernel times: pnr_get_kernel_ms group "radius". */
#define PNR_RADIUS_MAX 64
#define PNR_RADIUS_MAX_N (1 << 28)
typedef struct pnr_radius_opts {
    int32_t thr, rel_pct, rmax, bg_permille;
} pnr_radius_opts;
int pnr_measure_radii(pnr_ctx *ctx, const float *xyz /* n x 3 */, int64_t n, const pnr_radius_opts *opts /* NULL = defaults */,
                      int32_t *k_out /* n */, int32_t *thr_used /* nullable */);

/* Pre-filters of the traced volume (beyond the reference, which traces the stack as it was loaded): a 3 x 3 (x 3) median against
 * shot noise and a flat-box top-hat against uneven background, on the GPU, between pnr_set_volume* and pnr_soma / pnr_frangi.
 * THE RULE (the contract; tests restate it in numpy).  V is the context's traced u8 volume (w x h x l, owned or borrowed; for
 * 16-bit input the windowed bytes).  Both stages are exact integer operations; the median runs first, then the top-hat; a stage
 * whose option is 0 is skipped, both 0 is a valid no-op that leaves the context alone.
 *   median = 2: the 3 x 3 window in the plane of every slice (9 samples); median = 3: the 3 x 3 x 3 window (27 samples).
 *     Coordinates outside the volume are clamped to the edge (replicate, as Frangi::imgaussian does), so that every window has
 *     exactly 9 / 27 samples, duplicates included.  out = the sample of rank 4 (of 9) / rank 13 (of 27) in ascending order,
 *     0-based.  (For l == 1, median = 3 gives the bytes of median = 2.)
 *   tophat_r = R in 1..PNR_TOPHAT_MAX_R: a flat box with the half-widths rx = ry = R, rz = (int)((float)R / zd), zd = params.zdist
 *     (one IEEE f32 division); in the 2-D mode (l == 1) only dz = 0 exists.  B(p) = the voxels of the box around p that lie inside
 *     the volume (voxels outside are not in the window; a box larger than the stack is legal).  e(p) = min of V over B(p),
 *     o(p) = max of e over B(p), out(p) = V(p) - o(p); o <= V holds at every voxel, so nothing is clamped.
 * Arguments (anything else: PNR_E_ARG): opts non-NULL, median in {0, 2, 3}, tophat_r in 0..PNR_TOPHAT_MAX_R.  No volume in the
 * context: PNR_E_STATE.  Afterwards the context is what pnr_set_volume of the filtered bytes leaves: the same dimensions and 2-D
 * mode, an owned volume, and no later pipeline state (soma, Frangi, J8, seeds and the graph are invalidated).  pnr_get_volume
 * returns the filtered bytes and pnr_measure_radii measures on them (the rule of the windowed bytes of 16-bit input: the radius
 * is measured on what is traced).  A second call filters the filtered volume.  A borrowed device volume (pnr_set_volume_device) is
 * never written: the result is an owned buffer and the context stops borrowing.  The filter computes into buffers of the call and
 * the context's volume changes only once everything has succeeded: on any failure (PNR_E_NOMEM: an allocation failed) the context
 * still holds the unfiltered volume.  Device memory of the call: the filtered volume (N bytes) and, when both stages run, N bytes
 * more that are freed before the call returns.  All voxel indices are 64-bit.  The work runs on the context's stream
 * (pnr_set_stream); kernel times: pnr_get_kernel_ms group "filter". */
#define PNR_TOPHAT_MAX_R 64
typedef struct pnr_filter_opts {
    int32_t median;   /* 0 = off, 2 = 3 x 3 in every slice, 3 = 3 x 3 x 3 */
    int32_t tophat_r; /* 0 = off, 1..PNR_TOPHAT_MAX_R */
} pnr_filter_opts;
int pnr_filter_volume(pnr_ctx *ctx, const pnr_filter_opts *opts);

/* Tree distance: one SWC tree scored against another (beyond the reference, which has no evaluation code).  This follows the
 * published definition of Vaa3D's "neuron distance" (SD, SSD, %SSD): resample both trees, take the distance of every point of one
 * tree to the nearest line segment of the other, average in both directions, and report the share and the mean of the points
 * further away than 2 voxels.  Vaa3D's own digits are not pinned (none of its code was at hand); the contract is THE RULE below,
 * which the tests restate in numpy.  Every f32 operation is a single IEEE operation (-ffp-contract=off, correctly rounded division
 * and square root); parentheses give the order.
 *   Point to segment.  Point p, segment j = (a, b), all f32.  Per segment, computed once: ab = b - a;
 *     den = (ab.x*ab.x + ab.y*ab.y) + ab.z*ab.z;  r = den > 0 ? 1.0f / den : 0.0f.  Per pair: ap = p - a;
 *     num = (ap.x*ab.x + ap.y*ab.y) + ap.z*ab.z;  t = fminf(fmaxf(num * r, 0.f), 1.f);  e = p - (a + t*ab) componentwise (one
 *     multiply, one add, one subtract);  d2 = (e.x*e.x + e.y*e.y) + e.z*e.z.  Per point: d = sqrtf(min over j of d2), j* = the
 *     smallest j that attains the minimum.  A minimum does not depend on order: every tiling gives the same bits.  All inputs must
 *     be finite (PNR_E_ARG otherwise); the rule is meant for voxel coordinates (|v| < 2^60: no intermediate overflows).
 *   Tree.  n nodes xyz (f32) and parent[i] in [-1, n), any negative value = none: the layout of pnr_reconstruct's output, the caller
 *     drops the dummy node.  First z *= zscale (one f32 multiply; zscale > 0, default 1; pass zdist for distances in xy voxels).
 *     Segments: one per node, (x_i, x_parent[i]); a node without a parent gives (x_i, x_i): m = n, an isolated node still counts.
 *     Sample points, in node order: the node itself, then, if it has a parent and step > 0, the interior points of its segment:
 *     L = the f64 length sqrt((dx*dx + dy*dy) + dz*dz) of the segment, q = ceil(L / step), the points a + (b - a) * (k / q) for
 *     k = 1..q-1 with a = x_i, b = x_parent[i], computed in f64 and rounded to f32.  step = 0: the nodes only.  Host code.
 *   Metrics.  A direction X -> Y with the distances d_k of X's N points to Y's segments: mean = sum(d) / N; big = {k : d_k >= thr}
 *     (an f32 compare; thr default 2); ssd = sum over big of d / |big|, 0 when big is empty; pct = |big| / N; max = max d.  The sums
 *     are sequential f64 additions in point order, on the host.  Combined: sd, ssd, pct = the means (x + y) / 2 of the two
 *     directions, hausdorff = the larger max.
 * pnr_point_segment_distance: the GPU call of the first paragraph for n points against m segments (seg_a, seg_b: m x 3 each);
 *   d_out[n], j_out[n] (nullable).  1 <= m, 0 <= n (n = 0 is a valid no-op), both at most PNR_DISTANCE_MAX_N.  It needs no volume
 *   and leaves the pipeline state of the context alone; it runs on the context's stream (pnr_set_stream) in launches of a bounded
 *   number of pairs and frees every device buffer before it returns (PNR_E_NOMEM: an allocation failed).  Kernel times:
 *   pnr_get_kernel_ms group "distance".
 * pnr_tree_sample: the sample points of a tree, host only, no context.  *n_out = their number; the first min(cap, *n_out) are written
 *   to pts_out (x, y, z) and owner_out (the node of the point), either may be NULL: *n_out > cap: call again, as pnr_reconstruct.
 * pnr_tree_distance: both directions (A's points to B's segments, then B's to A's) on ctx's GPU and the metrics.  opts = NULL =
 *   {zscale 1, step 1, thr 2}.  dA_out / ownerA_out (nullable, capA entries) receive the distance and the node of A's first
 *   min(capA, result->ab.n) sample points, likewise for B.  PNR_E_ARG: an empty tree (n < 1) on either side, zscale <= 0, step < 0,
 *   a value that is not finite, a parent outside [-1, n), more than PNR_DISTANCE_MAX_N nodes or sample points on a side. */
#define PNR_DISTANCE_MAX_N (1 << 22)
typedef struct pnr_distance_opts {
    float zscale, step, thr;
} pnr_distance_opts; /* NULL = {1, 1, 2} */
typedef struct pnr_distance_dir {
    int64_t n, n_big; /* sample points of the source tree; those with d >= thr */
    double mean, ssd, pct, max;
} pnr_distance_dir;
typedef struct pnr_distance_result {
    pnr_distance_dir ab, ba; /* A's points against B's segments; B's points against A's */
    double sd, ssd, pct, hausdorff;
} pnr_distance_result;
int pnr_point_segment_distance(pnr_ctx *ctx, const float *pts /* n x 3 */, int64_t n, const float *seg_a /* m x 3 */, const float *seg_b /* m x 3 */,
                               int64_t m, float *d_out /* n */, int32_t *j_out /* n, nullable */);
int pnr_tree_sample(const float *xyz /* n x 3 */, const int32_t *parent /* n */, int64_t n, float zscale, float step, float *pts_out, int32_t *owner_out,
                    int64_t cap, int64_t *n_out);
int pnr_tree_distance(pnr_ctx *ctx, const float *xyzA, const int32_t *parentA, int64_t nA, const float *xyzB, const int32_t *parentB, int64_t nB,
                      const pnr_distance_opts *opts /* NULL = defaults */, pnr_distance_result *result, float *dA_out, int32_t *ownerA_out, int64_t capA,
                      float *dB_out, int32_t *ownerB_out, int64_t capB);

/* Joining the traced forest into one tree (beyond the reference, whose only tool against a forest is ENFORCE_SINGLE_TREE: every tree
 * but the largest is thrown away).  This is the step between a tracer and morphometry, a simulator or a tree comparison that Vaa3D
 * calls sort_neuron_swc: fragments whose closest nodes lie within a gap are bridged, the result is re-rooted and put in tree order.
 * Vaa3D's own digits are not pinned; the contract is THE RULE below, which the tests restate in numpy.  Every f32 operation is a
 * single IEEE operation (-ffp-contract=off); parentheses give the order.
 *   Input.  n nodes xyz (f32) and parent[i] in [-1, n), any negative value = none: the layout of pnr_reconstruct's output with the
 *     dummy node dropped, and of pnr_tree_distance.  Options {zscale, gap, root}.  First z *= zscale (one f32 multiply; zscale > 0,
 *     default 1).  The input trees are the connected components of the parent links.  PNR_E_ARG: a parent chain that does not end
 *     within n steps (a cycle), a coordinate that is not finite, a parent >= n.  Meant for voxel coordinates (|v| < 2^60).
 *   Pair weight.  For nodes i != j of DIFFERENT input trees: dx = x_i - x_j, likewise dy, dz; d2 = (dx*dx + dy*dy) + dz*dz, which is
 *     bit-symmetric in (i, j) because negation is exact.  The key of the pair is the triple (bits(d2), min(i, j), max(i, j)), compared
 *     lexicographically: d2 >= +0, so its bit pattern orders like its value, and no two pairs share a key.
 *   Bridges.  g2 = gap * gap (one f32 multiply); gap == 0: no limit.  The bridges are the edges of the UNIQUE minimum spanning forest
 *     of the graph whose vertices are the input trees and whose edges are all pairs with d2 <= g2, under that key order: what Kruskal's
 *     algorithm over the ascending pairs gives, and what Boruvka's rounds give in any order -- the result does not depend on tiling,
 *     slices, launches or round structure.  They are reported in ascending key order as (lo, hi, d = sqrtf(d2)).
 *   Re-rooting.  The output components are the components of {parent links} + {bridges}; each is a tree.  Its root is `root` if
 *     root >= 0 and the component holds that node, else the input root of the input tree with the most nodes in the component (ties:
 *     the smallest root index).  parent_out is the unique orientation of the component's edges away from that root; node order and
 *     xyz are not changed.
 *   Numbering and order.  comp_out[i]: the component of `root` first (if given), then the others by descending node count, ties by
 *     ascending root index.  order_out is a permutation of 0..n-1: the components in that numbering, each in depth-first pre-order
 *     from its root with the children visited in ascending node index -- a file written in order_out has every parent before its
 *     children.
 * pnr_nearest_other: the GPU call of the rule's inner search on coordinates as they are (no zscale).  For every point i with
 *   label[i] >= 0: d_out[i] = sqrtf of the minimum of d2 over the points j with label[j] >= 0 and label[j] != label[i], j_out[i] = the
 *   smallest j at the minimum; without such a point, and for a point with a negative label (neither source nor target), +inf and -1.
 *   1 <= n <= PNR_JOIN_MAX_N; all coordinates finite.  It needs no volume and leaves the pipeline state alone; it runs on the
 *   context's stream in launches of a bounded pair count and frees every device buffer before it returns (PNR_E_NOMEM: an allocation
 *   failed).  Kernel times: pnr_get_kernel_ms group "join".
 * pnr_join_trees: Boruvka's rounds on ctx's GPU -- labels = the current components, one nearest-other pass per round, the per-component
 *   minimum under the full key and the union-find on the host; a component whose best edge exceeds g2 can never be joined and leaves
 *   the search -- then the re-rooting.  opts = NULL = {1, 0, -1}; gap < 0 (or not finite), zscale <= 0 and root >= n are PNR_E_ARG.
 *   parent_out, order_out, comp_out (n entries each) and bridges_out (cap_bridges entries) are nullable; *n_bridges > cap_bridges: call
 *   again, as pnr_reconstruct.  n_trees_in / n_trees_out (nullable): input trees, output components.  pnr_get_option "join_rounds":
 *   the passes the last call took.
 * pnr_join_reroot: the re-rooting and ordering half alone, pure host, no context: the same code pnr_join_trees ends in.  PNR_E_ARG
 *   also for a bridge outside [0, n) or between two nodes of one (already joined) tree. */
#define PNR_JOIN_MAX_N (1 << 22)
typedef struct pnr_join_opts {
    float zscale, gap;
    int32_t root; /* a node index, or negative: none */
} pnr_join_opts; /* NULL = {1, 0, -1} */
typedef struct pnr_bridge {
    int32_t lo, hi;
    float d;
} pnr_bridge;
int pnr_nearest_other(pnr_ctx *ctx, const float *xyz /* n x 3 */, const int32_t *label /* n */, int64_t n, float *d_out /* n */, int32_t *j_out /* n */);
int pnr_join_trees(pnr_ctx *ctx, const float *xyz /* n x 3 */, const int32_t *parent /* n */, int64_t n, const pnr_join_opts *opts /* NULL = defaults */,
                   int32_t *parent_out, int32_t *order_out, int32_t *comp_out, pnr_bridge *bridges_out, int64_t cap_bridges, int64_t *n_bridges,
                   int64_t *n_trees_in, int64_t *n_trees_out);
int pnr_join_reroot(const int32_t *parent /* n */, int64_t n, const pnr_bridge *bridges, int64_t nb, int64_t root, int32_t *parent_out, int32_t *order_out,
                    int32_t *comp_out);

/* Rendering the tree into the stack (beyond the reference, which has no way back from the tree to the voxels).  This is the step Vaa3D
 * calls swc2mask: which voxels the tree occupies, and with the traced volume how much of the image's signal the trace explains, where it
 * does not (the residual) and which nodes run through background (the per-segment counts).  Vaa3D's own digits are not pinned; the
 * contract is THE RULE below, which the tests restate in numpy.  Every f32 operation is a single IEEE operation (-ffp-contract=off,
 * correctly rounded division); parentheses give the order.
 *   Input.  n nodes xyz (f32, voxel indices as in pnr_node), radius[i] (f32, xy voxels) and parent[i] in [-1, n), any negative value =
 *     none: the layout of pnr_tree_distance and pnr_join_trees.  A grid w x h x l.  Options {zscale, rscale, radd, thr}; opts = NULL =
 *     {1, 1, 0, -1}.
 *   Scaling.  Node z *= zscale (one multiply; zscale > 0).  rr_i = fmaxf(radius_i * rscale + radd, 0) (one multiply, one add).  Voxel
 *     (x, y, z) is the point p = ((float)x, (float)y, (float)z * zscale); with l == 1 only z = 0 exists.
 *   Segment i.  a = x_i, b = x_parent[i], ra = rr_i, rb = rr_parent[i]; without a parent b = a and rb = ra: a ball, so an isolated node
 *     still renders.  Computed once per segment, exactly as in the distance rule: ab = b - a, den = (ab.x*ab.x + ab.y*ab.y) + ab.z*ab.z,
 *     r = den > 0 ? 1.0f / den : 0.0f, and dr = rb - ra.
 *   Pair (p, i).  ap, num, t = fminf(fmaxf(num * r, 0.f), 1.f), e and d2 are those of the point-to-segment paragraph of
 *     pnr_point_segment_distance, operation for operation.  rt = ra + t * dr (one multiply, one add).  The voxel is inside segment i iff
 *     d2 <= rt * rt (one multiply, an f32 compare).
 *   Label.  L(p) = 1 + the smallest i whose test passes; 0 if none.  A minimum does not depend on order: every cut into pieces, boxes
 *     and launches gives the same bits.  mask(p) = L > 0 ? 255 : 0.
 *   Coverage, on the context's traced u8 volume V (w x h x l, owned or borrowed; windowed and pre-filtered as traced), whose dimensions
 *     are the grid.  t = thr, or for thr == -1: max(1, floor(sum(V) / N)) from the exact u64 sum -- the absolute mode of the radius
 *     rule.  Foreground means V >= t.  Exact u64 counts: n_vox, n_tree (L > 0), n_fg, n_both, sum_fg (the sum of V over the
 *     foreground), sum_both (the sum of V over the foreground under the tree).  Per segment i: seg_vox[i], seg_fg[i], seg_sum[i] =
 *     the voxels labelled i + 1, those of them that are foreground, and the sum of V over all of them.  Derived on the host as f64, 0
 *     when the denominator is 0: covered = n_both / n_fg, on_signal = n_both / n_tree, covered_intensity = sum_both / sum_fg.
 *     residual(p) = L > 0 ? 0 : V(p).
 *   Arguments (anything else: PNR_E_ARG): 0 <= n <= PNR_RENDER_MAX_N (n = 0 gives an all-zero label volume); w, h, l >= 1 (each below
 *     2^31, at most 2^40 voxels); every coordinate (also z * zscale) and radius finite, radius >= 0; zscale > 0, rscale >= 0, radd finite;
 *     every rr_i <= PNR_RENDER_MAX_R; parent < n; thr in -1..255.  Meant for voxel coordinates, as the distance rule.
 * pnr_render_tree: label_out / mask_out (N = w*h*l each, nullable) on any grid.  It needs no volume and leaves the pipeline state of the
 *   context alone.
 * pnr_tree_coverage: renders on the grid of the context's volume (PNR_E_STATE without one) and never writes V.  cov, the per-segment
 *   arrays (n each), mask_out and residual_out (N each) are all nullable.
 * Both run on the context's stream (pnr_set_stream), use 64-bit voxel indices throughout and free every device buffer before they
 *   return (PNR_E_NOMEM: an allocation failed; device memory of a call: 4 N bytes of labels, N more for each of mask and residual).
 *   The host cuts every segment along its axis into pieces of at most render_piece xy voxels, gives each piece the integer box of its
 *   sub-interval grown by max(ra, rb) + 1 and cuts boxes of more than render_box voxels; the pair test always uses the whole segment, so
 *   the options change no bit.  Kernel times: pnr_get_kernel_ms group "render" (= "render_scatter" + "render_finish"); pnr_get_option
 *   "render_items" / "render_pairs": the work items and (voxel, segment) tests of the last call. */
#define PNR_RENDER_MAX_N (1 << 22)
#define PNR_RENDER_MAX_R 1024
typedef struct pnr_render_opts {
    float zscale, rscale, radd;
    int32_t thr;
} pnr_render_opts; /* NULL = {1, 1, 0, -1} */
typedef struct pnr_coverage {
    int64_t n_vox, n_tree, n_fg, n_both, sum_fg, sum_both;
    int32_t thr_used, pad;
    double covered, on_signal, covered_intensity;
} pnr_coverage;
int pnr_render_tree(pnr_ctx *ctx, const float *xyz /* n x 3 */, const float *radius /* n */, const int32_t *parent /* n */, int64_t n, int64_t w, int64_t h,
                    int64_t l, const pnr_render_opts *opts /* NULL = defaults */, int32_t *label_out /* N, nullable */, uint8_t *mask_out /* N, nullable */);
int pnr_tree_coverage(pnr_ctx *ctx, const float *xyz /* n x 3 */, const float *radius /* n */, const int32_t *parent /* n */, int64_t n,
                      const pnr_render_opts *opts /* NULL = defaults */, pnr_coverage *cov, int64_t *seg_vox, int64_t *seg_fg, int64_t *seg_sum /* n each, nullable */,
                      uint8_t *mask_out, uint8_t *residual_out /* N each, nullable */);

/* Connected components of the traced volume (beyond the reference, which has no component code outside its soma path).  Two uses:
 * before tracing, small bright blobs that the median and the top-hat leave -- debris, hot-pixel clusters -- are cleared, as Vaa3D
 * pipelines remove small foreground components (pnr_despeckle_volume); after tracing, the components of the residual
 * (pnr_tree_coverage) are the list of what the trace missed (pnr_label_components).
 * THE RULE (the contract; tests restate it in numpy).  Everything is an exact integer operation.  V is the context's traced u8 volume
 * (w x h x l, owned or borrowed; for 16-bit input the windowed bytes, after pnr_filter_volume the filtered bytes), N = w * h * l.
 *   Options {thr, connectivity, min_size}; opts = NULL = {-1, 26, 1}.
 *   Foreground: V >= t.  t = thr, or for thr == -1: max(1, floor(sum(V) / N)) from the exact u64 sum -- the rule of pnr_tree_coverage
 *     and of the radius's absolute mode (the same kernel).  thr = 0 makes every voxel foreground.  t is reported as thr_used.
 *   Neighbours: two foreground voxels are neighbours, for connectivity = 6, when they differ by 1 in exactly one coordinate; for
 *     connectivity = 26, when they differ by at most 1 in every coordinate and are not equal.  With l == 1 that is 4- and
 *     8-connectivity in the plane; nothing special-cases it.
 *   Component: a class of the transitive closure of the neighbour relation.  first = its smallest linear index x + w * (y + h * z).
 *     The kept components (size >= min_size) are numbered 1..K in ascending first.  label(p) = that number; 0 for background and for
 *     the voxels of components below min_size.
 *   Per kept component a pnr_component of exact integers: first, size, sum (of V), sx, sy, sz (the sums of the voxel coordinates: the
 *     centroid is s / size), the inclusive bounding box x0, y0, z0, x1, y1, z1 and vmax (the maximum of V).
 *   Summary pnr_components_info: n_vox = N, n_fg, n_comp = K (kept), n_small / vox_small (the components below min_size and their
 *     voxels), largest (the largest size; 0 without a kept component), thr_used.
 *   Integer sums, minima and maxima do not depend on order: the rule fixes every bit, whatever the tiling, launch cut or atomic
 *     arrival order.
 * pnr_label_components: never writes V and leaves the pipeline state of the context alone, as pnr_tree_coverage.  info, label_out (N)
 *   and comps are nullable; the first min(cap, n_comp) entries of comps are filled, info->n_comp is always the full count.
 * pnr_despeckle_volume: out(p) = V(p) if p is background or belongs to a kept component, else 0: the foreground components smaller
 *   than min_size are cleared, nothing else changes.  Afterwards the context is what pnr_filter_volume leaves: an owned volume of the
 *   same dimensions and 2-D mode, the later pipeline state invalidated; a borrowed device volume is never written, and V is replaced
 *   only once everything has succeeded.  min_size = 1 is a valid no-op that leaves the context alone (info, if given, is filled).
 * Arguments (anything else: PNR_E_ARG): thr in -1..255, connectivity in {6, 26}, min_size >= 1; N at most 2^32 - 2 (the links between
 *   voxels are u32 indices -- the largest configured stack, 2048 x 2048 x 512, has 2^31 voxels; all other index arithmetic is 64-bit);
 *   cap >= 0; label_out with more than 2^31 - 1 kept components.  No volume in the context: PNR_E_STATE.  PNR_E_NOMEM: an allocation
 *   failed.
 * Both run on the context's stream (pnr_set_stream) and free every device buffer of the call before they return.  Device memory of a
 *   call, with K_all = the components before min_size: 8 N bytes (4 N of links that become the labels, 4 N of component ids), N / 1024
 *   bytes of counts, 72 K_all bytes of statistics, and for pnr_despeckle_volume the N bytes of the new volume, which stay.  Kernel times:
 *   pnr_get_kernel_ms group "components" = the sum of "components_threshold" (the byte sum of thr = -1), "components_local",
 *   "components_merge", "components_flatten", "components_number", "components_stats" and "components_finish". */
typedef struct pnr_components_opts {
    int32_t thr, connectivity;
    int64_t min_size;
} pnr_components_opts; /* NULL = {-1, 26, 1} */
typedef struct pnr_component {
    int64_t first, size, sum, sx, sy, sz;
    int32_t x0, y0, z0, x1, y1, z1, vmax, pad;
} pnr_component;
typedef struct pnr_components_info {
    int64_t n_vox, n_fg, n_comp, n_small, vox_small, largest;
    int32_t thr_used, pad;
} pnr_components_info;
int pnr_label_components(pnr_ctx *ctx, const pnr_components_opts *opts /* NULL = defaults */, pnr_components_info *info /* nullable */,
                         int32_t *label_out /* N, nullable */, pnr_component *comps /* nullable */, int64_t cap);
int pnr_despeckle_volume(pnr_ctx *ctx, const pnr_components_opts *opts /* NULL = defaults */, pnr_components_info *info /* nullable */);

/* Exact anisotropic Euclidean distance transform of the traced volume (beyond the reference): every foreground voxel gets its squared
 * distance to the nearest background voxel, in xy-voxel units with z counted zdist-fold.  pnr_measure_radii answers the same question
 * at a list of points in whole numbers; this is the whole stack, sub-voxel: sqrt(D2) at a node's voxel is its radius, the maximum of
 * D2 is the thickest point of the stack (where a soma is, and how large somaradius has to be), D2 over a component of the residual is
 * how thick what the trace missed is.
 * THE RULE (the contract; tests restate it in numpy).  V is the context's traced u8 volume (w x h x l, owned or borrowed; for 16-bit
 * input the windowed bytes, after pnr_filter_volume / pnr_despeckle_volume the filtered bytes), N = w * h * l, zd = params.zdist (>= 1).
 *   Options {thr, rmax}; opts = NULL = {-1, 64}.
 *   Foreground: V >= t.  t = thr, or for thr == -1: max(1, floor(sum(V) / N)) from the exact u64 sum -- the rule of the radii, the
 *     coverage and the components (the same kernel).  t is reported as thr_used.  Background: V < t.
 *   Distance: for a foreground voxel p and a background voxel q INSIDE the volume, with the integer offsets (dx, dy, dz) = q - p:
 *     d2(p, q) = (float)(dx*dx + dy*dy) + (zd*(float)dz) * (zd*(float)dz) -- the f32 expression of the radius rule's shells, single IEEE
 *     operations (-ffp-contract=off).
 *   Output: cap = (float)(rmax*rmax); D2(p) = min(cap, min over all background q of d2(p, q)); background voxels get D2 = 0.  Voxels
 *     outside the volume do not exist and are not background: a stack without any background voxel has D2 = cap everywhere (the radius
 *     rule's convention).  With l == 1 only dz = 0 occurs; nothing special-cases it.  A minimum does not depend on order: every tiling,
 *     pass structure and launch cut gives the same bits.
 *   Summary pnr_edt_info (exact): n_vox = N, n_fg, n_capped (foreground voxels with D2 == cap), d2_max (the maximum of D2 over the
 *     foreground), first_max (the smallest linear index x + w * (y + h * z) that attains it; -1 and d2_max = 0 when n_fg == 0), thr_used.
 *   Points: xyz (n x 3 f32, nullable when n == 0) -> d2_at[n] = D2 at the centre voxel of the radius rule, per coordinate
 *     c = (int) fminf(fmaxf(v + 0.5f, 0.f), (float)(extent - 1)); -1.0f for a position with a non-finite coordinate.  Node radii are read
 *     this way without moving 4 N bytes to the host.
 * Arguments (anything else: PNR_E_ARG): thr in -1..255, rmax in 1..PNR_EDT_MAX_R, 0 <= n <= PNR_RADIUS_MAX_N, N at most 2^32 - 2 (as for
 *   the components).  No volume in the context: PNR_E_STATE.  PNR_E_NOMEM: an allocation failed.  info, d2_out (N) and the points are
 *   each optional.
 * The call never writes V (also not a borrowed one), leaves the pipeline state of the context alone, runs on the context's stream
 *   (pnr_set_stream), uses 64-bit voxel indices and frees every device buffer of the call before it returns.  Device memory of a call:
 *   8 N bytes (4 N that hold the u16 row distances and then D2, 4 N that hold the row carries and then the u32 plane distances),
 *   4 (rmax + 1) bytes of the z table, 32 bytes of sums, and 16 n bytes for the points.  Kernel times: pnr_get_kernel_ms group "edt" =
 *   the sum of "edt_threshold" (the byte sum of thr = -1), "edt_x", "edt_y", "edt_z", "edt_stats" and "edt_sample". */
#define PNR_EDT_MAX_R 1024
typedef struct pnr_edt_opts {
    int32_t thr, rmax;
} pnr_edt_opts; /* NULL = {-1, 64} */
typedef struct pnr_edt_info {
    int64_t n_vox, n_fg, n_capped, first_max;
    float d2_max;
    int32_t thr_used;
} pnr_edt_info;
int pnr_distance_transform(pnr_ctx *ctx, const pnr_edt_opts *opts /* NULL = defaults */, pnr_edt_info *info /* nullable */, float *d2_out /* N, nullable */,
                           const float *xyz /* n x 3, nullable when n == 0 */, int64_t n, float *d2_at /* n */);

/* Thinning the foreground of the traced volume to a curve skeleton (beyond the reference, which has no thinning): the step of a
 * Vaa3D-style pipeline that turns a binary object into a one-voxel-wide centre line and reads that as a tree.  Two uses: a second,
 * topological trace of the same stack that shares no code or parameter with the particle tracer (to score against, pnr_tree_distance),
 * and the residual of a trace (pnr_tree_coverage) as SWC fragments that pnr_geodesic_bridges can attach to it.
 * THE RULE (the contract; tests restate it in numpy).  Everything is an exact integer operation.  V is the context's traced u8 volume
 * (w x h x l, owned or borrowed; windowed and filtered as traced), N = w * h * l.  Options {thr, max_rounds}; opts = NULL = {-1, 0}.
 *   Object: V >= t.  t = thr, or for thr == -1: max(1, floor(sum(V) / N)) from the exact u64 sum (the same kernel as the radii, the
 *     coverage, the components and the distance transform).  t is reported as thr_used.  Voxels outside the volume are background.
 *     params.zdist plays no part: thinning is topological.
 *   Neighbourhoods of a voxel p: N6, N18 and N26 are the voxels that differ from p by at most 1 in every coordinate and in exactly 1, at
 *     most 2, at most 3 coordinates; none contains p.  Connectivity is (26, 6): 26 for the object, 6 for the background.
 *   Simple point (Malandain-Bertrand): p is simple when (a) the object voxels of N26(p) are non-empty and form exactly one 26-connected
 *     set within N26(p), and (b) the background voxels of N6(p) are non-empty and all lie in one 6-connected set of the background
 *     voxels of N18(p).  Deleting a simple point changes neither the object's 26-components, nor the background's 6-components, nor the
 *     tunnels.
 *   End point: exactly one voxel of N26(p) is object.
 *   Subfield: s(p) = (x & 1) | (y & 1) << 1 | (z & 1) << 2 of p = (x, y, z).  Two voxels of one subfield are never 26-adjacent.
 *   One round: first the object voxels with a background voxel in N6 are marked as candidates, taken at the round's start.  Then for
 *     s = 0..7 in order one pass: every candidate of subfield s that is still object is deleted if, in the image as it stands at the
 *     start of that pass, it is simple and not an end point; all deletions of a pass happen at once.  Rounds repeat until a round
 *     deletes nothing or max_rounds rounds have run (0: no limit).  rounds counts the rounds run, the last, empty one included.
 *   Why the rule is exact: within a pass no deleted voxel lies in another's N26, so the simultaneous deletion equals a sequential one in
 *     any order; topology is preserved exactly, and the rule fixes every bit whatever the tiling or launch cut.  A pass runs in place: a
 *     thread reads voxels of other subfields, which do not change during the pass, and writes only its own.  The marking runs in place
 *     too: it only switches object voxels between two non-zero states.
 *   Output: skel(p) = 255 for what is left of the object, else 0.  The skeleton voxels in ascending linear index x + w * (y + h * z)
 *     with their degree, the number of skeleton voxels in N26.  Summary pnr_thin_info (exact): n_vox = N, n_fg, n_skel, n_end / n_branch
 *     / n_isolated (the skeleton voxels of degree 1, >= 3 and 0), tiles (the work-group tiles of the volume), tile_visits (the tiles the
 *     passes visited: 8 * tiles in the first round; later a tile is visited only if it or one of its 26 neighbour tiles deleted
 *     something during the previous round or the completed passes of this one -- decided from completed passes only, so the count is
 *     deterministic; it is a property of the implementation, not of the rule), rounds, thr_used.
 * pnr_skeletonize: never writes V (also not a borrowed one) and leaves the pipeline state of the context alone.  info, skel_out (N),
 *   vox_out and deg_out are nullable; the first min(cap, n_skel) entries of vox_out and deg_out are filled, info->n_skel is always the
 *   full count.  Arguments (anything else: PNR_E_ARG): thr in -1..255, max_rounds >= 0, cap >= 0, N at most 2^32 - 2 (as for the
 *   components).  No volume in the context: PNR_E_STATE.  PNR_E_NOMEM: an allocation failed.  It runs on the context's stream
 *   (pnr_set_stream), uses 64-bit voxel indices and frees every device buffer of the call before it returns.  Device memory of a call:
 *   N bytes of state, 8 bytes per tile of 32 x 8 x 8 voxels (stamps and the visit list), N / 1024 bytes of chunk counts, 64 bytes of
 *   counters, and 5 n_skel bytes for the list.  Kernel times: pnr_get_kernel_ms group "thin" = the sum of "thin_threshold" (the byte sum
 *   of thr = -1), "thin_init", "thin_mark", "thin_pass" (with the visit plans between the passes), "thin_list" and "thin_finish".
 * pnr_skeleton_forest: the skeleton as a forest, pure host, no context.  Nodes are the k voxels vox (distinct linear indices of a
 *   w x h x l grid, any order); edges are the 26-adjacent pairs.  The output is the unique minimum spanning forest under the total order
 *   (squared step length 1 / 2 / 3, then lo, then hi) as pnr_bridge {lo, hi, d = sqrtf(len2)} with lo < hi node indices, sorted by
 *   (lo, hi): short links win, so junction triangles open at their diagonal.  *n_edges = k - components, always the full count; the
 *   first min(cap, *n_edges) entries of edges_out (nullable) are filled.  Feeding the edges to pnr_join_reroot with an all-roots parent
 *   gives parents and tree order.  PNR_E_ARG: k < 0 or above 2^31 - 1, a grid extent below 1, an index outside the grid or listed
 *   twice, cap < 0. */
typedef struct pnr_thin_opts {
    int32_t thr, max_rounds;
} pnr_thin_opts; /* NULL = {-1, 0} */
typedef struct pnr_thin_info {
    int64_t n_vox, n_fg, n_skel, n_end, n_branch, n_isolated, tiles, tile_visits;
    int32_t rounds, thr_used;
} pnr_thin_info;
int pnr_skeletonize(pnr_ctx *ctx, const pnr_thin_opts *opts /* NULL = defaults */, pnr_thin_info *info /* nullable */, uint8_t *skel_out /* N, 0 / 255, nullable */,
                    int64_t *vox_out /* linear indices, ascending, nullable */, uint8_t *deg_out /* nullable */, int64_t cap);
int pnr_skeleton_forest(const int64_t *vox /* k */, int64_t k, int64_t w, int64_t h, int64_t l, pnr_bridge *edges_out /* nullable */, int64_t cap, int64_t *n_edges);

/* Gray-weighted geodesic distance through the traced volume (beyond the reference): every voxel gets the cost of the cheapest 26-connected
 * path to the nearest of n source points, where a step costs its length times the darkness of the two voxels it joins, together with the
 * label of that source, and the path itself for a list of targets.  The tree distance, pnr_join_trees, pnr_measure_radii and the distance
 * transform measure straight lines and ignore the image in between; this follows the signal: the cost at a fragment's node says whether the
 * gap to the tree is a dim stretch of one neurite or background between two cells, and the path says along which voxels it attaches.
 * THE RULE (the contract; tests restate it in numpy).  Exact integer arithmetic, but for the 26 step lengths: single IEEE f32 operations on
 * the host.  V is the context's traced u8 volume (w x h x l, owned or borrowed, windowed or filtered as traced), N = w * h * l.
 *   Options {thr, dmax, cost}; opts = NULL = {0, 2^31 - 1, NULL}.
 *   Domain: a voxel is passable when V >= t.  t = thr, or for thr == -1: max(1, floor(sum(V) / N)) (the byte-sum kernel of the other calls);
 *     t is reported as thr_used.  With the default thr = 0 every voxel is passable and the cost does the work.  Voxels outside the volume
 *     do not exist.
 *   Steps: the 26 offsets o = (dx, dy, dz), each component in {-1, 0, 1}, not all zero, enumerated with dz slowest, then dy, then dx, each
 *     ascending (THE OFFSET ORDER).  len[o] = (uint32) rintf(32.0f * sqrtf((float)(dx*dx + dy*dy) + (zd*(float)dz) * (zd*(float)dz))),
 *     zd = params.zdist.  With l == 1 only dz = 0 occurs.  len[o] = len[-o].
 *   Cost: c(v), a table of 256 u16 entries, each >= 1; the default is c(v) = 256 - v; opts->cost (256 entries) replaces it.
 *   Edge: for passable neighbours p, q = p + o: wt(p, q) = len[o] * (c(V(p)) + c(V(q))), symmetric.  PNR_E_ARG if
 *     max(len) * 2 * max(c) > 2^31 - 1.
 *   Sources: n_src points xyz (f32) with labels label[i] >= 0 (int32; src_label = NULL: label i = i).  The centre voxel of a point is that of
 *     the radius / distance-transform rule, per coordinate c = (int) fminf(fmaxf(v + 0.5f, 0.f), (float)(extent - 1)).  A source with a
 *     non-finite coordinate, and a source whose centre voxel is not passable, is DROPPED; dropped sources are counted in n_src_dropped.
 *   Key: every voxel has a u64 key (D << 32) | label; NONE is all ones.  A source voxel has key = (0, the smallest label of the sources on
 *     it).  Every other passable voxel p: key(p) = min over the passable neighbours q with D(q) + wt(q, p) <= dmax of
 *     key(q) + (wt(q, p) << 32); NONE if there is no such neighbour.  Adding wt << 32 keeps the label, so the key is the lexicographic
 *     minimum over all paths of (cost, source label): D is the cheapest path cost from any source, the label the smallest among the sources
 *     that attain it.  Weights are >= 64, so the recursion is well founded and its solution unique; a path of cost <= dmax has only prefixes
 *     of cost <= dmax, so the cap changes no kept value.  Every quantity is a minimum over a fixed set: no tiling, round structure, launch
 *     cut or arrival order changes a bit.
 *   Outputs: D(p) u32, 0xFFFFFFFF when unreached; L(p) int32, -1 when unreached; impassable voxels are unreached.  D / 64 is the path
 *     length in xy voxels at the brightest cost (c = 1).
 *   Path: for a reached voxel p with D > 0, pred(p) is the first q in the offset order with key(q) + (wt(q, p) << 32) == key(p), compared on
 *     the full key.  Such a q exists and D strictly decreases along the walk, which therefore ends on a source voxel of label L(p) after at
 *     most D / 64 steps.  The path of a target is p, pred(p), ..., the source voxel, as linear indices x + w * (y + h * z).
 *   Summary pnr_geo_info (exact): n_vox = N, n_pass, n_reached, n_src (kept), n_src_dropped, d_max (the largest D over the reached voxels),
 *     first_max (the smallest linear index that attains it; -1 and d_max = 0 when nothing is reached), thr_used, rounds (relaxation rounds
 *     of this call: scheduling, not part of the rule).
 *   Targets: at_xyz (m x 3 f32) -> d_at[m], label_at[m] at the centre voxel; a non-finite target gives 0xFFFFFFFF, -1 and path_len 0.
 *     With path_cap > 0, path_len[i] = k > 0: the complete path, k voxels written to path_vox[i * path_cap ...]; 0: the target is unreached
 *     or not finite; -path_cap: the walk was cut after path_cap voxels, and those are written.  With path_cap == 0 path_len and path_vox
 *     are not touched.
 * Arguments (anything else: PNR_E_ARG): thr in -1..255, 1 <= dmax <= 2^31 - 1, cost entries >= 1, labels >= 0, 0 <= n_src, m <=
 *   PNR_RADIUS_MAX_N (with n_src = 0 everything is unreached), src_xyz when n_src > 0, at_xyz and at least one of d_at / label_at /
 *   (path_cap > 0) when m > 0, path_cap in 0..PNR_GEO_MAX_PATH with path_len and path_vox when path_cap > 0 and m > 0, N at most 2^32 - 2.
 *   No volume in the context: PNR_E_STATE.  PNR_E_NOMEM: an allocation failed.  info, d_out, label_out and the targets are each optional.
 * The call never writes V (also not a borrowed one), leaves the pipeline state of the context alone, runs on the context's stream
 *   (pnr_set_stream), uses 64-bit voxel indices and frees every device buffer of the call before it returns.  Device memory of a call: 8 N
 *   bytes of keys, 12 bytes per tile of GEO_TX x GEO_TY x GEO_TZ voxels (two flag arrays and the list), 4 N more for each of d_out and
 *   label_out that is asked for (split on the device), 512 bytes of cost table, 16 n_src bytes of sources, and per target 20 bytes plus
 *   4 + 8 path_cap bytes with paths; 8 bytes of pinned host memory carry the round's tile count.
 * Kernel times: pnr_get_kernel_ms group "geodesic" = the sum of "geodesic_threshold", "geodesic_init", "geodesic_compact",
 *   "geodesic_relax", "geodesic_stats", "geodesic_split", "geodesic_sample" and "geodesic_paths".  pnr_get_option "geo_rounds" /
 *   "geo_visits": the rounds and the tile visits of the last call.  pnr_set_option "geo_iters" (LDS iterations per tile visit; 0 =
 *   automatic, 1 forces a tile to re-queue itself) and "geo_tiles_per_launch" (0 = automatic; small values force launch cuts) change no
 *   bit: tests reach the boundaries on small stacks with them. */
#define PNR_GEO_MAX_PATH (1 << 16)
typedef struct pnr_geo_opts {
    int32_t thr;
    uint32_t dmax;
    const uint16_t *cost;
} pnr_geo_opts; /* NULL = {0, 2^31 - 1, NULL} */
typedef struct pnr_geo_info {
    int64_t n_vox, n_pass, n_reached, n_src, n_src_dropped, first_max;
    uint32_t d_max;
    int32_t thr_used, rounds, pad;
} pnr_geo_info;
int pnr_geodesic_distance(pnr_ctx *ctx, const float *src_xyz, const int32_t *src_label /* nullable */, int64_t n_src,
                          const pnr_geo_opts *opts, pnr_geo_info *info /* nullable */,
                          uint32_t *d_out /* N, nullable */, int32_t *label_out /* N, nullable */,
                          const float *at_xyz /* m x 3, nullable when m == 0 */, int64_t m, uint32_t *d_at, int32_t *label_at /* m, nullable */,
                          int32_t path_cap /* 0..PNR_GEO_MAX_PATH */, int32_t *path_len /* m */, int64_t *path_vox /* m x path_cap */);

/* Joining the traced forest along the signal (beyond the reference): the composition of the geodesic distance and the join.  pnr_join_trees
 * bridges fragments whose closest nodes lie within a straight-line gap and never looks at the image in between; this takes the forest and
 * the stack and returns the unique minimum spanning forest of the fragments under gray-weighted path cost, every bridge as the voxel path
 * it follows.  One geodesic pass suffices (Mehlhorn 1988): a minimum spanning tree of the graph whose edges are the places where the
 * geodesic Voronoi cells of the trees touch, weighted D(p) + wt(p, q) + D(q), is one of the complete graph of pairwise geodesic distances.
 * THE RULE (the contract; tests restate it in numpy).  Exact integer arithmetic on top of the geodesic rule above; every output bit is fixed.
 *   Input.  n nodes xyz (f32, voxel indices as in pnr_node) and parent[i] in [-1, n), any negative value = none: the layout of
 *     pnr_join_trees.  PNR_E_ARG: a cycle, a parent >= n, a coordinate that is not finite.  The context's traced u8 volume V,
 *     zd = params.zdist.  Options {thr, limit, step, cost}; opts = NULL = {0, 0, 1, NULL}; limit == 0: no limit; thr and cost are
 *     those of pnr_geo_opts.
 *   Trees and sources.  The input trees are the components of the parent links; the label of a tree is its smallest node index.  The
 *     sources are the sample points of pnr_tree_sample(xyz, parent, n, zscale = 1, step), in its order, each labelled with the tree of
 *     its owner node (step = 0: the nodes only).  D and L are the outputs of the geodesic rule for these sources with dmax = limit, or
 *     2^31 - 1 when limit is 0 or above 2^31 - 1.  A tree all of whose sources are dropped or share their centre voxel with a source of
 *     a smaller label takes no part, is never bridged and is counted in n_trees_lost.
 *   Meet edges.  For every voxel p and every offset o among the last 13 of THE OFFSET ORDER (indices 13..25: q = p + o has the larger
 *     linear index, every unordered pair of 26-neighbours occurs once): if both voxels are reached and L(p) != L(q),
 *     W(p, o) = D(p) + wt(p, q) + D(q), a u64 (it can exceed 2^32), wt the edge weight of the geodesic rule.  The edge exists iff
 *     limit == 0 or W <= limit (W >= D(p), D(q): capping D at limit drops no edge that the limit keeps).  Its key is the triple
 *     (W, p, o - 13), compared lexicographically; no two edges share a key.
 *   Bridges.  The edges of the UNIQUE minimum spanning forest of the graph whose vertices are the trees and whose edges are the meet
 *     edges, under that key order: what Kruskal's algorithm over the ascending keys gives, and what Boruvka's rounds give in any order
 *     -- independent of tiling, launch cuts, round structure and atomic arrival order.  Reported in ascending key order.
 *   Path and attachment of a bridge (W, p, o).  path(p) and path(q) are the walks along pred() of the geodesic rule; they end on source
 *     voxels s_a, s_b of labels L(p), L(q).  The bridge's voxel chain is reverse(path(p)) followed by path(q): s_a .. p, q .. s_b, at
 *     least 2 voxels.  Node a is the owner of the first sample point, in sample order, of tree L(p) whose centre voxel is s_a; node b
 *     likewise on s_b.
 *   Expansion (pnr_join_expand, pure host).  The k interior voxels of a chain (all but s_a and s_b) become new nodes n, n + 1, ...,
 *     appended bridge after bridge in bridge order, each at its voxel's integer coordinates, each the child of the previous node of the
 *     chain, the first one of a.  The bridge handed to the re-rooting is (the last new node, b), or (a, b) when k = 0, as
 *     pnr_bridge {lo = the smaller index, hi, d = W / 64}.  A negative parent is written as -1.  Re-rooting, numbering and order are
 *     pnr_join_reroot on the n + sum(k) nodes, exactly as for pnr_join_trees.
 *   Summary pnr_geojoin_info (exact): n_trees_in, n_trees_lost, n_trees_out (= n_trees_in - n_bridges), n_bridges, n_inserted (sum(k)),
 *     n_src / n_src_dropped (the geodesic's), w_max (the largest bridge W, 0 without one), thr_used, rounds (Boruvka rounds of this
 *     call: scheduling, not part of the rule).
 * pnr_geodesic_bridges: the geodesic pass, then Boruvka's rounds on the device over the settled keys, which never cross to the host:
 *   per round two sweeps of the key volume give every current component its minimum meet edge under the full key, the host unites; a
 *   component without an edge within the limit leaves the search.  The bridges' p and q voxels then go through the path stage of the
 *   geodesic call.  bridges_out (cap_bridges entries) and path_vox (cap_path entries: the chains one after the other, bridge k at
 *   path_off, path_len voxels) are nullable; *n_bridges > cap_bridges or *n_path > cap_path: call again, as pnr_join_trees.
 *   PNR_E_ARG also for: thr outside -1..255, step < 0 or not finite, a cost entry of 0, n outside 1..PNR_JOIN_MAX_N, more than 2^28
 *   sample points, N above 2^32 - 2, an extent of 2^24 or more (voxel coordinates must be exact in f32), and a bridge whose walk to its
 *   tree has more than PNR_GEO_MAX_PATH voxels (the message says that it was cut).  No volume in the context: PNR_E_STATE.  The call
 *   never writes V (also not a borrowed one), leaves the pipeline state alone, runs on the context's stream, uses 64-bit voxel indices
 *   and frees every device buffer before it returns.  Device memory: that of the geodesic call without d_out / label_out, 20 bytes per
 *   tree during the rounds, then per bridge 2 (24 + 8 * 256) bytes, and 8 path_cap more for every walk of more than 256 voxels,
 *   path_cap = min(PNR_GEO_MAX_PATH, w_max / the smallest edge + 2); 20 bytes per source.
 * pnr_join_expand: the expansion alone, pure host, no context; the grid w x h x l turns a voxel into coordinates.  *n_nodes = n + sum(k);
 *   xyz_out, parent_out (cap_nodes entries), bridge_of (cap_nodes - n entries: for every new node its bridge) are nullable and written
 *   only when *n_nodes <= cap_nodes: else call again.  join_out (nb entries, nullable): the bridges for pnr_join_reroot.  PNR_E_ARG: a
 *   bridge node outside [0, n) or a == b, a path outside [0, n_path) or of fewer than 2 voxels, a voxel outside the grid, more than
 *   PNR_JOIN_MAX_N nodes in all.
 * Kernel times: pnr_get_kernel_ms group "geojoin" = "geojoin_meet_w" + "geojoin_meet_e"; the relaxation counts under "geodesic".
 *   pnr_get_option "geojoin_rounds": the rounds of the last call.  pnr_set_option "geojoin_tiles_per_launch" (0 = automatic) cuts the
 *   launches of a sweep and changes no bit. */
typedef struct pnr_geojoin_opts {
    int32_t thr;
    uint64_t limit;
    float step;
    const uint16_t *cost;
} pnr_geojoin_opts; /* NULL = {0, 0, 1, NULL} */
typedef struct pnr_geo_bridge {
    int32_t a, b;
    int64_t p;
    int32_t o, path_len;
    uint64_t w;
    int64_t path_off;
} pnr_geo_bridge;
typedef struct pnr_geojoin_info {
    int64_t n_trees_in, n_trees_lost, n_trees_out, n_bridges, n_inserted, n_src, n_src_dropped;
    uint64_t w_max;
    int32_t thr_used, rounds;
} pnr_geojoin_info;
int pnr_geodesic_bridges(pnr_ctx *ctx, const float *xyz /* n x 3 */, const int32_t *parent /* n */, int64_t n, const pnr_geojoin_opts *opts /* NULL = defaults */,
                         pnr_geojoin_info *info /* nullable */, pnr_geo_bridge *bridges_out, int64_t cap_bridges, int64_t *n_bridges, int64_t *path_vox,
                         int64_t cap_path, int64_t *n_path);
int pnr_join_expand(const float *xyz /* n x 3 */, const int32_t *parent /* n */, int64_t n, const pnr_geo_bridge *bridges, int64_t nb, const int64_t *path_vox,
                    int64_t n_path, int64_t w, int64_t h, int64_t l, float *xyz_out, int32_t *parent_out, int32_t *bridge_of, int64_t cap_nodes, int64_t *n_nodes,
                    pnr_bridge *join_out /* nb */);

/* Grey-level morphological reconstruction of the traced volume (beyond the reference; Vincent 1993): fill holes, h-maxima, h-domes.  Every
 * other tool decides "foreground" by a threshold on the traced bytes; this repairs the grey image's shape before that decision.  A soma
 * with a dark nucleus is a hollow object whose "curve skeleton" is a closed surface: PNR_MORPH_FILL closes it first.  Shallow grey-level
 * maxima join noise into a sponge at the mean threshold: PNR_MORPH_HMAX removes exactly those, and PNR_MORPH_HDOME keeps bright structure
 * standing at least h above its surroundings whatever its width.
 * THE RULE (the contract; tests restate it in numpy).  Everything is exact u8 / integer arithmetic.  V is the context's traced u8 volume
 * (w x h x l, owned or borrowed, windowed and filtered as traced), N = w * h * l.  params.zdist plays no part.
 *   Neighbourhoods N_C(p), C in {4, 8, 6, 26}: the offsets (dx, dy, dz) in {-1, 0, 1}^3, not all zero.  C = 26: all of them; C = 6: exactly
 *     one non-zero component; C = 8: dz = 0; C = 4: dz = 0 and exactly one non-zero component.  A neighbour outside the volume does not
 *     exist.  C = 4 and C = 8 on a 3-D stack treat every slice independently; with l == 1, 6 equals 4 and 26 equals 8.
 *   Reconstruction by dilation rho_C(M, V): let M' = min(M, V).  R(p) = the maximum, over all C-paths p0, ..., pk = p with k >= 0, of
 *     min(M'(p0), V(p1), ..., V(pk)).  Equivalently R is the least volume with R >= M' and
 *     R(p) = min(V(p), max(R(p), max over q in N_C(p) of R(q))).  M' <= R <= V.
 *   Reconstruction by erosion: rho*_C(M, V) = 255 - rho_C(255 - M, 255 - V).
 *   Exact whatever the schedule: start from M'; every update replaces R(p) by min(V(p), max of itself and its neighbours); every value ever
 *     held is <= the fixed point, so values only rise and a stale neighbour value is still a lower bound; when no voxel can rise the
 *     recursion holds everywhere, and the least fixed point above M' is unique.  No tiling, round structure or launch cut changes a bit.
 *   Operations (opts->op):
 *     1 PNR_MORPH_DILATE  marker required      out = rho_C(marker, V)
 *     2 PNR_MORPH_ERODE   marker required      out = rho*_C(marker, V)
 *     3 PNR_MORPH_FILL    marker must be NULL  out = rho*_C(M, V), M = V on B_C and 255 elsewhere: grey fill-holes; out >= V; every regional
 *                                              minimum that is not connected to the border under C is raised to its pass height
 *     4 PNR_MORPH_HMAX    marker must be NULL  out = rho_C(max(V - h, 0), V), h in 1..255
 *     5 PNR_MORPH_HDOME   marker must be NULL  out = V - (the volume of op 4), h in 1..255; 0 <= out <= h
 *     B_C, the border set of op 3: the voxels with x in {0, w - 1} or y in {0, h - 1}, and for C in {6, 26} and l > 1 also those with z in
 *     {0, l - 1}.  connectivity = 0 is the default of the op: 6 for FILL (the background connectivity of the thinning rule), 26 for the others.
 *   Summary pnr_morph_info (exact unless said otherwise): n_vox = N, n_changed (voxels with out != V), n_nonzero (out > 0), sum_in and
 *     sum_out (the u64 sums of V and of out), max_delta (max |out - V|), connectivity (the one used: the op's default for 0), tiles (of
 *     MORPH_TX x MORPH_TY x MORPH_TZ voxels); tile_visits and rounds: scheduling, not part of the rule, reported and never compared bit for bit.
 * pnr_morph_reconstruct: all five ops.  marker: N host bytes for ops 1 and 2.  info and out (N host bytes) are nullable.  It never writes V
 *   (also not a borrowed one), leaves the pipeline state of the context alone and frees every device buffer of the call before it returns.
 * pnr_morph_volume: ops 3 to 5 only, with the contract of pnr_filter_volume: afterwards the context is what pnr_set_volume of the result's
 *   bytes leaves -- the same dimensions and 2-D mode, an owned volume, and no later pipeline state (soma, Frangi, J8, seeds and the graph are
 *   invalidated); pnr_get_volume returns the result; a second call works on the result of the first; a borrowed device volume
 *   (pnr_set_volume_device) is never written: the result is an owned buffer and the context stops borrowing; the context's volume changes
 *   only once everything has succeeded: on any failure the context still holds the old volume.
 * Arguments (anything else: PNR_E_ARG): opts non-NULL, op in 1..5, connectivity in {0, 4, 8, 6, 26}, h in 1..255 for ops 4 and 5 and 0
 *   otherwise, marker non-NULL exactly for ops 1 and 2, N at most 2^32 - 2.  No volume in the context: PNR_E_STATE.  PNR_E_NOMEM: an
 *   allocation failed.  Voxel indices are 64-bit; the work runs on the context's stream (pnr_set_stream).  Device memory of a call: N bytes
 *   of state (the marker is uploaded into it or built from V; it becomes the result in place, and the context's volume under
 *   pnr_morph_volume), 12 bytes per tile (two flag arrays and the list); 8 bytes of pinned host memory carry the round's tile count.
 * Kernel times: pnr_get_kernel_ms group "morph" = the sum of "morph_init" (the state from the op), "morph_compact" (the listed tiles of a
 *   round), "morph_relax" (the tile relaxation) and "morph_finish" (the result and the statistics).  pnr_get_option "morph_rounds" /
 *   "morph_visits": the rounds and the tile visits of the last call.  pnr_set_option "morph_iters" (LDS iterations per tile visit; 0 =
 *   automatic, 1 forces a tile to re-queue itself) and "morph_tiles_per_launch" (0 = automatic; small values force launch cuts) change no
 *   bit: tests reach the boundaries on small stacks with them. */
#define PNR_MORPH_DILATE 1
#define PNR_MORPH_ERODE 2
#define PNR_MORPH_FILL 3
#define PNR_MORPH_HMAX 4
#define PNR_MORPH_HDOME 5
typedef struct pnr_morph_opts {
    int32_t op, connectivity, h, pad;
} pnr_morph_opts;
typedef struct pnr_morph_info {
    int64_t n_vox, n_changed, n_nonzero;
    uint64_t sum_in, sum_out;
    int64_t tiles, tile_visits;
    int32_t max_delta, connectivity, rounds, pad;
} pnr_morph_info;
int pnr_morph_reconstruct(pnr_ctx *ctx, const pnr_morph_opts *opts, const uint8_t *marker /* N, host; ops 1, 2 only */, pnr_morph_info *info /* nullable */,
                          uint8_t *out /* N, host, nullable */);
int pnr_morph_volume(pnr_ctx *ctx, const pnr_morph_opts *opts, pnr_morph_info *info /* nullable */);

/* Marker-controlled watershed of the traced volume (beyond the reference; Meyer 1991): the last step of "separate what touches".  Two somas
 * that touch are one component for pnr_label_components and one tree for pnr_skeletonize, and no threshold parts them: the neck is as
 * bright as the cells.  pnr_geodesic_distance labels by additive cost, so the nearer source wins even across a dark gap.  The watershed
 * floods a relief from markers and puts the border on the lowest pass between them (the minimax rule): with the relief 255 - V on the
 * darkest gap, with a relief made from pnr_distance_transform on the neck.
 * THE RULE (the contract; tests restate it in numpy).  Everything is exact integer arithmetic.  V is the context's traced u8 volume,
 * N = w * h * l.  params.zdist plays no part.
 *   Mask.  V >= t, t = opts->thr, or for thr == -1 the mean rule of pnr_label_components (max(1, floor(sum / N))); thr = 0: every voxel.
 *   Relief R (u8).  `relief`: N host bytes; NULL: R = 255 - V, bright signal is low ground and floods first.
 *   Neighbourhoods N_C, C in {4, 8, 6, 26}, exactly as the morphological reconstruction above defines them; connectivity = 0 means 26.
 *   Markers, in exactly one of two forms (both, or neither: PNR_E_ARG).  marker_vol: N host int32, a value > 0 is a label, 0 none, a
 *     negative one PNR_E_ARG.  Or n_src > 0 points src_xyz (n x 3 f32, voxel positions) with labels src_label (>= 1; NULL: 1 .. n in
 *     order), each placed on its centre voxel (the radius rule above).  A point that is not finite and a marker (point or voxel) outside the
 *     mask are dropped and counted in n_dropped.  Where several points share a voxel the smallest label wins.
 *   Key.  Every mask voxel carries a key K = (M, D), compared lexicographically.  A marker voxel p has K = (R(p), 0), for good.  Stepping
 *     from s to a mask neighbour t that is no marker: g(K(s), t) = (R(t), 1) if R(t) > M(s), else (M(s), D(s) + 1).  K(t) is the minimum,
 *     over all C-paths inside the mask from any marker to t, of g applied along the path.  M is the lowest pass height to a marker -- the
 *     minimax altitude, the reconstruction by erosion of the marker function under R --, D the steps since the flood last had to rise:
 *     the order in which Meyer's hierarchical queues reach the voxels.  A mask voxel that no marker reaches has no key.
 *   Exact whatever the schedule: g is monotone (K <= K' gives g(K, t) <= g(K', t)) and strictly increasing (g(K, t) > K).  Start with the
 *     markers at their keys and everything else at +inf; every update replaces K(t) by the minimum of itself and g(K(q), t) over its
 *     neighbours q.  Every value ever held is that of a real path, so keys only fall and a stale neighbour key is still an upper bound;
 *     the only fixed point is the path minimum.  No tiling, round structure or launch cut changes a bit.
 *   Label, from the final keys only.  A neighbour s of t is tight when g(K(s), t) == K(t).  L(marker voxel) = its label; L(t) = the
 *     smallest L(s) over the tight neighbours s of t.  Tight edges rise strictly in K: a recursion over a DAG with one solution, relaxed as
 *     a falling minimum in any order.  Every region is C-connected and holds its marker.  Unreached voxels and those outside the mask: 0.
 *   Two passes, necessarily: the triple (M, D, L) carried as one key is NOT monotone -- across a rise both candidates become
 *     (R(t), 1, .), and a label taken from a key that was not yet final can stick.  The labels are relaxed only once the keys have settled.
 *   Representation.  The key is the u32 M << 24 | D; D saturates at 2^24 - 1 (saturating addition keeps g monotone), and a call in which
 *     the D of any voxel ends saturated fails with PNR_E_ARG (the text names the plateau depth and the level).
 *   Outputs.  label_out (N host int32) and level_out (N host bytes: M of the reached voxels -- the height at which a voxel joined its
 *     region --, 0 elsewhere), both nullable.  pnr_watershed_info, exact: n_vox = N, n_mask, n_marker_vox (mask voxels that hold a
 *     marker), n_dropped, n_reached (markers included), n_unreached (= n_mask - n_reached), n_regions (distinct labels in the result),
 *     m_max, d_max (the largest M and D of a reached voxel; 0 without one), thr_used, connectivity (the one used), tiles (of
 *     WS_TX x WS_TY x WS_TZ voxels); flood_visits / flood_rounds (pass 1) and label_visits / label_rounds (pass 2): scheduling, not part
 *     of the rule, reported and never compared bit for bit.
 * Arguments, checked in this order (PNR_E_ARG unless said otherwise): ctx and opts non-NULL; thr in -1..255; connectivity in {0, 4, 8, 6,
 *   26}; n_src in 0..2^31 - 2; exactly one marker form (marker_vol, or n_src > 0; src_label only with points); src_xyz with n_src > 0;
 *   every src_label >= 1; a volume in the context (else PNR_E_STATE) of at most 2^32 - 2 voxels; no negative entry in marker_vol.
 *   PNR_E_NOMEM: an allocation failed.  The call never writes V (also not a borrowed one), leaves the pipeline state of the context alone,
 *   runs on the context's stream (pnr_set_stream), uses 64-bit voxel indices and frees every device buffer before it returns.  Device
 *   memory of a call: 9 bytes per voxel (key, label, relief; the levels replace the relief in place), 12 bytes per tile, 4 bytes per
 *   marker (the labels for n_regions; 16 per point in the point form); 8 bytes of pinned host memory carry a round's tile count.
 * Kernel times: pnr_get_kernel_ms group "watershed" = the sum of "watershed_init" (mean threshold, point scatter, first keys),
 *   "watershed_compact", "watershed_flood" (pass 1), "watershed_label" (pass 2) and "watershed_finish".  pnr_get_option "ws_rounds" /
 *   "ws_visits": rounds and tile visits of the last call, both passes together.  pnr_set_option "ws_iters" (LDS iterations per tile
 *   visit; 0 = automatic, 1 forces a tile to re-queue itself) and "ws_tiles_per_launch" (0 = automatic; small values force launch cuts)
 *   change no bit: tests reach the boundaries on small stacks with them. */
typedef struct pnr_watershed_opts {
    int32_t thr, connectivity;
} pnr_watershed_opts;
typedef struct pnr_watershed_info {
    int64_t n_vox, n_mask, n_marker_vox, n_dropped, n_reached, n_unreached, n_regions;
    int64_t tiles, flood_visits, label_visits;
    int32_t m_max, d_max, thr_used, connectivity, flood_rounds, label_rounds;
} pnr_watershed_info;
int pnr_watershed(pnr_ctx *ctx, const pnr_watershed_opts *opts, const uint8_t *relief /* N, host, nullable */, const int32_t *marker_vol /* N, host, or NULL */,
                  const float *src_xyz /* n_src x 3, or NULL */, const int32_t *src_label /* n_src, nullable */, int64_t n_src,
                  pnr_watershed_info *info /* nullable */, int32_t *label_out /* N, host, nullable */, uint8_t *level_out /* N, host, nullable */);

/* Automatic thresholds from the histogram of the context's u8 volume V (threshold.hip), and a local threshold.
 *
 * The rule (restated in numpy by tests/threshold_ref.py; every value below is exact):
 *   H[v], v = 0..255: the number of voxels with value v, in u64.  lo in 0..255 picks the counted bins [lo, 255] (lo = 1 ignores the
 *   zeros a top-hat, a despeckle or a residual leave).  n = sum H[v], S = sum v H[v] over the counted bins.  Every method yields `raw`;
 *   thr = min(255, max(raw, lo, 1)), so zero is never foreground.  n == 0: thr = 255, n_counted = 0, PNR_OK.
 *   PNR_THR_MEAN: raw = S div n (lo = 0: the rule "thr = -1" of the tools).
 *   PNR_THR_OTSU: for t = lo + 1 .. 255 class 0 is the bins [lo, t), class 1 the bins [t, 255], with counts n0, n1 and sums S0, S1; t is
 *     valid when n0 > 0 and n1 > 0.  In IEEE double, in this order, no contraction: w0 = (double)n0, w1 = (double)n1,
 *     d = (double)S1 / w1 - (double)S0 / w0, score = ((w0 * w1) * d) * d (the conversions are exact: fewer than 2^45 voxels).  raw = the
 *     smallest valid t with the largest score; no valid t (one non-empty bin b): raw = b.
 *   PNR_THR_TRIANGLE (the bright side: bright on dark): p = the smallest counted v with the largest H, e = the largest counted v with
 *     H > 0.  e - p < 2: raw = e.  Else, for b = p + 1 .. e - 1 in signed 64-bit, g(b) = (H[p] - H[e]) (e - b) + (H[e] - H[b]) (e - p)
 *     ((e - p) times the height of the chord from the peak to the end above the histogram at b); raw = b* + 1 for the smallest b* with
 *     the largest g.
 *   PNR_THR_TOP (the brightest share), top_ppm in 1..999999: k = floor(n top_ppm / 10^6); raw = the smallest t in [lo, 255] with
 *     sum_{v >= t} H[v] <= k; none: raw = 255.
 *   PNR_THR_MAXENTROPY: the reference's maxentropy_th (toolbox.cpp:657-737) on H, the function pnr_soma thresholds with; it needs lo == 0
 *     and every bin below 2^31 (the reference's int hist[]), else PNR_E_ARG.  Parity as for the soma path: pinned on the oracle's
 *     restatement.
 *
 * pnr_threshold_from_hist: the rule and nothing else; pure host, no context.  Arguments (anything else: PNR_E_ARG): hist, opts and info
 *   non-NULL, method in 0..4, lo in 0..255, top_ppm in 1..999999 for PNR_THR_TOP and 0 otherwise, fewer than 2^45 voxels in all.
 *   info: thr, method, lo; n_vox (all bins), n_counted = n, sum_counted = S; v_min, v_max (the smallest and largest counted v with
 *   H > 0) and peak (p above), -1 each when n == 0; n_fg = the voxels >= thr over all bins.
 * pnr_auto_threshold: the histogram of the context's volume on its stream (one read of N bytes; kernel time group "threshold"), then the
 *   function above.  hist_out (nullable): the 256 counts.  No volume in the context: PNR_E_STATE.  The context is left as it is; V is
 *   never written; the 2 KiB of device bins are freed before the call returns.
 *
 * The local threshold, pnr_local_opts {r, offset, scale_256, floor, binary}:
 *   the box is the top-hat's: rx = ry = r, rz = (int)((float)r / zd) with one f32 division, zd = params.zdist (only dz = 0 when l == 1).
 *   B(p) = the box around p cut to the volume, n(p) = |B(p)|, S(p) = the sum of V over B(p).  keep(p) iff V(p) >= floor and
 *   256 n(p) V(p) >= scale_256 S(p) + 256 offset n(p) in signed 64-bit; out(p) = keep ? (binary ? 255 : V(p)) : 0.  A box larger than
 *   the stack is legal.  Arguments (anything else: PNR_E_ARG): opts non-NULL, r in 1..PNR_LOCAL_MAX_R, offset in -255..255, scale_256 in
 *   0..4096, floor in 1..255, binary in {0, 1}.  No volume in the context: PNR_E_STATE.
 * pnr_local_threshold: out (N host bytes, nullable) receives the result; the context and its volume stay as they are.
 * pnr_local_threshold_volume: the result becomes the context's volume under the contract of pnr_filter_volume: an owned buffer, a
 *   borrowed device volume is never written (it is released), the later pipeline state is invalidated, and on any failure the context
 *   still holds the old volume.
 *   info (nullable) of both: n_vox = N, n_kept (voxels with keep), sum_in and sum_out (the sums of V and of out), rx, ry, rz.  All
 *   indices are 64-bit.  Device memory of a call beyond the N bytes of the result: (6 s + 10 rz + 8) w h bytes for slabs of
 *   s = max(1, min(l, 2^24 / (w h))) planes (threshold.h), freed before the call returns (PNR_E_NOMEM: an allocation failed).  Kernel
 *   time group "local_threshold".  pnr_set_option "lt_slab_vox" (0 = automatic: 2^24) changes no bit: tests reach slab boundaries on
 *   small stacks with it. */
enum { PNR_THR_MEAN = 0, PNR_THR_OTSU = 1, PNR_THR_TRIANGLE = 2, PNR_THR_TOP = 3, PNR_THR_MAXENTROPY = 4 };
typedef struct pnr_threshold_opts {
    int32_t method, lo, top_ppm, pad;
} pnr_threshold_opts;
typedef struct pnr_threshold_info {
    int64_t n_vox, n_counted;
    uint64_t sum_counted;
    int64_t n_fg;
    int32_t thr, method, lo, v_min, v_max, peak;
} pnr_threshold_info;
int pnr_threshold_from_hist(const uint64_t hist[256], const pnr_threshold_opts *opts, pnr_threshold_info *info);
int pnr_auto_threshold(pnr_ctx *ctx, const pnr_threshold_opts *opts, pnr_threshold_info *info, uint64_t *hist_out /* 256, nullable */);
#define PNR_LOCAL_MAX_R 64
typedef struct pnr_local_opts {
    int32_t r, offset, scale_256, floor, binary, pad;
} pnr_local_opts;
typedef struct pnr_local_info {
    int64_t n_vox, n_kept;
    uint64_t sum_in, sum_out;
    int32_t rx, ry, rz, pad;
} pnr_local_info;
int pnr_local_threshold(pnr_ctx *ctx, const pnr_local_opts *opts, pnr_local_info *info /* nullable */, uint8_t *out /* N, host, nullable */);
int pnr_local_threshold_volume(pnr_ctx *ctx, const pnr_local_opts *opts, pnr_local_info *info /* nullable */);

/* Pruning a tree's short side branches, and the per-node morphometry a tree-order file is followed by (beyond the reference; the step
 * Vaa3D does by rounds of "delete the short terminal branches, recount, delete again").  The rule is decided in ONE pass from one
 * quantity per node, its height, and does not depend on the order of the nodes except through one stated tie rule; the tests restate
 * it in numpy (tests/prune_ref.py).  Every value below is exact.
 *   Input.  A forest: xyz (n x 3 f32), radius (n f32, NULL = all 0), parent[i] in [-1, n), any negative value = root, no cycle: the
 *     layout of pnr_join_trees.  Options {zscale, min_length, radius_factor, min_tree}; opts = NULL = {1, 0, 0, 0}.
 *   Units.  Every length is an integer in units of 1/256 xy voxel: Q(x) = floor(256 x + 0.5), evaluated in double.
 *   1 Edge.  For a non-root i with parent p: q[i] = Q(sqrt(dx*dx + dy*dy + dz*dz)), the differences taken in double from the f32
 *     inputs, dz times (double)zscale, the sum from the left, no contraction, sqrt correctly rounded.  q[root] = 0.
 *   2 Height.  H[i] = 0 for a leaf, else the maximum over the children c of q[c] + H[c].
 *   3 Continuing child.  Of a node with children: the child with the largest q[c] + H[c]; at a tie the smallest index.
 *   4 Segment heads.  Every root is a head, and so is every node that is not its parent's continuing child.  seg[i] = the nearest head on
 *     the path from i to its root, i included.  S[c] = q[c] + H[c] for a non-root head, S = H for a root.
 *   5 Removal.  A non-root head c with parent p is removed iff S[c] < max(Q(min_length), Q((double)radius_factor * radius[p])); a root
 *     is removed iff H[root] < Q(min_tree); a node is removed iff some head on its path to the root, itself included, is removed.  With
 *     all three options 0 nothing is removed: the call is the morphometry alone.
 *   6 Per-node outputs (n entries each, all nullable): keep (u8, 1 = stays), height (u32, H), path (u32, the sum of q from the root),
 *     order (i32, the number of non-root heads on the path from the root, i included: the centrifugal branch order), seg (i32).
 *   7 Range.  If any q[c] + H[c] or any path reaches 2^32 units (2^24 xy voxels of path) the call fails with PNR_E_ARG; nothing wraps.
 *     1 <= n < 2^31.
 *   Consequences: a continuing child is never removed on account of its own segment; the heights of the kept nodes do not change, so
 *     pruning the pruned tree removes nothing; keep is monotone in min_length.
 *   pnr_prune_info: n, n_roots, n_leaves (no child), n_branch (2 or more children), n_segments (heads); n_removed (nodes),
 *     n_removed_segments (heads among them), n_removed_trees (roots among them); length_in, length_out (the sums of q over all and over
 *     the kept nodes); h_max, order_max (over all nodes); rounds_up, rounds_down (the launches of the two jumping loops; 0 on the host).
 *   PNR_E_ARG: n outside the range or xyz / parent missing, zscale <= 0, a negative (or not finite) option, a coordinate or radius that
 *     is not finite, a parent >= n, a cycle, the range of 7.
 * pnr_prune_tree: the rule on ctx's GPU (prune.hip) by pointer jumping: ceil(log2(depth)) + 1 launches up (heights, paths) and as many
 *   down (order, segment, removal), depth = the most edges between a node and its root; no kernel walks a chain.  It needs no volume and
 *   leaves the pipeline state alone; every device buffer (about 100 bytes per node) is freed before it returns (PNR_E_NOMEM: an
 *   allocation failed).  Kernel time group "prune".
 * pnr_prune_tree_host: the same rule as one sequential pass in topological order (prune_rule.cpp); pure host, no context.
 * pnr_prune_apply: pure host.  The kept nodes in input order: new_index_out[i] (n entries, nullable) = the new index of node i or -1,
 *   parent_out (n entries, nullable; the first *m are written) = the remapped parent of every kept node, *m = their number.  A file in
 *   tree order stays in tree order.  PNR_E_ARG: a parent >= n, a kept node whose parent is removed. */
typedef struct pnr_prune_opts {
    float zscale, min_length, radius_factor, min_tree;
} pnr_prune_opts; /* NULL = {1, 0, 0, 0} */
typedef struct pnr_prune_info {
    int64_t n, n_roots, n_leaves, n_branch, n_segments, n_removed, n_removed_segments, n_removed_trees;
    uint64_t length_in, length_out;
    uint32_t h_max;
    int32_t order_max, rounds_up, rounds_down;
} pnr_prune_info;
int pnr_prune_tree(pnr_ctx *ctx, const float *xyz /* n x 3 */, const float *radius /* n, nullable */, const int32_t *parent /* n */, int64_t n,
                   const pnr_prune_opts *opts /* NULL = defaults */, pnr_prune_info *info /* nullable */, uint8_t *keep, uint32_t *height, uint32_t *path,
                   int32_t *order, int32_t *seg);
int pnr_prune_tree_host(const float *xyz /* n x 3 */, const float *radius /* n, nullable */, const int32_t *parent /* n */, int64_t n,
                        const pnr_prune_opts *opts /* NULL = defaults */, pnr_prune_info *info /* nullable */, uint8_t *keep, uint32_t *height, uint32_t *path,
                        int32_t *order, int32_t *seg);
int pnr_prune_apply(const int32_t *parent /* n */, const uint8_t *keep /* n */, int64_t n, int32_t *new_index_out, int32_t *parent_out, int64_t *m);

/* How pnr_trace_batch / pnr_trace_replay schedule the particle filter on the GPU (results are bit-identical):
 * 0 = one launch per SMC phase over all active traces of a batch (default), 1 = one persistent work-group per trace. */
int pnr_set_smc_driver(pnr_ctx *ctx, int driver);

/* Scheduling and host-side knobs of a context; none of them changes a result (the library reads no environment variable).
 *   window (0 = automatic: 1536 on one GPU, 768 sharded or without the tentative replay) trace slots kept busy | look0, look_pct (0 / -1 = automatic) admission lookahead max(look0, frontier*look_pct/100)
 *   target (-1 = automatic: 120 on one GPU, 96 per rank sharded, 0 = off without the tentative replay) seeds are admitted only while fewer traces than this are running |
 *   lag (-1 = automatic: half a poll when no other trace group covers the host's share of a poll, else one step) steps of a poll that run on while the host works on the state in front of them |
 *   overfill (1) the target is the mean over a poll | concentrate (1) with several trace groups new seeds go to one group while few traces survive a poll |
 *   sums_deep (-1 = automatic: launches of at most sums_deep_max (96) traces, or one trace group; 0 / 1) form of the ordered sums (four chunk buffers in turn) |
 *   profile_every (1) with pnr_set_profiling: the streaming tracer times every n-th poll of a trace group and counts it n-fold | poll (0 = automatic: 2 on one or two GPUs, 4 from four ranks on) SMC steps between polls | groups (0 = automatic: 2 on one GPU, 1 sharded; 1..4) trace groups on separate streams | split_x10 (0 = automatic), max_split (96) sampling
 *   work-groups per CU x 10 / per trace | stash_mb (65536) sample-stash budget | host_threads (0 = CPUs of this process /
 *   local_ranks) workers of the seed flood fill and of pnr_reconstruct_ctx | local_ranks (1) processes sharing this host |
 *   trace_timing, seed_timing (0/1) statistics on stderr | recon_timing (0/1) stage times of every pnr_reconstruct on stderr (process-wide: that call takes no context) | trace_log (0/1) keep every trace's end for pnr_get_trace_log | replay_batches (0/1), batch_growth, batch_max: rank batches instead
 *   of the streaming window | no_stash (0/1) persistent driver without the sample stash | exchange_block (0 = 256 KB / world) bytes per rank
 *   and exchange of pnr_trace_replay_sharded | frangi_prune (1) skip the eigen-solver below the first J8 level (pnr_get_frangi) |
 *   hess_chunk (0 = automatic: 2^27 voxels) at most this many planes per z-chunk of the Hessian stage, in whole marches of 32 (only
 *   ever lowers the automatic size; the same bits -- tests reach chunk boundaries with it on small stacks) |
 *   cube_copy (1) phased driver: a trace's cube is fetched from the image once per step and copied by its sampling work-groups (0: each stages it itself) |
 *   share_scales (1) phased driver: a scale whose template grid nests in another's is not sampled, its sums read the host's stash (0: every scale samples on its
 *   own; the same bits) | share_min (0) ... in steps of at least this many traces |
 *   gauss_march (1) the fused x-y Gaussian marches down strips of a slice (0: one 64 x 64 tile per work-group; the same bits) |
 *   dist_split (0 = automatic: enough slices to fill the chip) segments per blockIdx.y slice of a launch of pnr_point_segment_distance |
 *   dist_pairs_per_launch (0 = automatic: 2^34) at most this many (point, segment) pairs per launch (the same bits -- tests reach slice and launch boundaries with them on small inputs) |
 *   join_split (0 = automatic), join_pairs_per_launch (0 = automatic: 2^34): the same for the targets and the (point, target) pairs of pnr_nearest_other / pnr_join_trees (the same bits) |
 *   render_piece (0 = automatic: 16) xy voxels of a segment's axis per work item of pnr_render_tree / pnr_tree_coverage | render_box (0 = automatic: 2^15) voxels per item, larger boxes are cut |
 *   render_items_per_launch (0 = automatic: 2^18) items per launch (the same bits -- tests reach piece, box and launch boundaries with them on small inputs) |
 *   geo_iters, geo_tiles_per_launch (0 = automatic) of pnr_geodesic_distance and geojoin_tiles_per_launch (0 = automatic: 2^20) tiles per launch of a sweep of pnr_geodesic_bridges (the same bits) |
 *   morph_iters, morph_tiles_per_launch (0 = automatic) of pnr_morph_reconstruct / pnr_morph_volume: the same two for its relaxation (the same bits) |
 *   ws_iters, ws_tiles_per_launch (0 = automatic) of pnr_watershed: the same two for both of its passes (the same bits) |
 *   lt_slab_vox (0 = automatic: 2^24) voxels per slab of whole planes of pnr_local_threshold / pnr_local_threshold_volume (the same bits -- tests reach slab boundaries with it on small stacks) |
 *   tentative (1) the streaming scheduler pauses traces that a tentative replay of everything recorded so far cuts, and ends them
 *   itself once that verdict is final (fewer wasted SMC iterations; same graph).
 *   pnr_get_option also knows "join_rounds" (the nearest-other passes of the last pnr_join_trees), "render_items" / "render_pairs" (the last render), "geo_rounds" / "geo_visits", "geojoin_rounds", "morph_rounds" / "morph_visits", "ws_rounds" / "ws_visits" (the last call of that tool), "host_threads_effective" and "frangi_recomputes" (how often pnr_get_frangi / pnr_quantise_j8 had to
 *   re-run Frangi without the frangi_prune shortcut -- one pnr_frangi worth of GPU time each; also printed with trace_timing /
 *   seed_timing).  The kernel timers (pnr_get_kernel_ms) include those re-runs. */
int pnr_set_option(pnr_ctx *ctx, const char *key, int64_t value);
int pnr_get_option(pnr_ctx *ctx, const char *key, int64_t *value);

/* Per-kernel-group device time (HIP events on the ctx stream) accumulated since the last reset:
 * groups: "gauss","hessian_eigen","j8","seed_maxima","soma","zncc","smc" (sampling kernel; the whole trace kernel of the persistent driver),"smc_sums","smc_predict","smc_update","smc_cube" (the traces' cubes fetched once per step),"recon" (pnr_reconstruct_ctx),"volume" (pnr_set_volume_u16: windowing to 8 bits),"radius" (pnr_measure_radii),"filter" (pnr_filter_volume: median and top-hat),"distance" (pnr_point_segment_distance / pnr_tree_distance),"join" (pnr_nearest_other / pnr_join_trees),"render" (pnr_render_tree / pnr_tree_coverage: the sum of "render_scatter" and "render_finish"),"components" (pnr_label_components / pnr_despeckle_volume: the sum of its "components_*" phases),"edt" (pnr_distance_transform: the sum of "edt_threshold", "edt_x", "edt_y", "edt_z", "edt_stats", "edt_sample"),"geodesic" (pnr_geodesic_distance: the sum of its "geodesic_*" phases),"geojoin" (pnr_geodesic_bridges: the sum of "geojoin_meet_w" and "geojoin_meet_e"),"morph" (pnr_morph_reconstruct / pnr_morph_volume: the sum of "morph_init", "morph_compact", "morph_relax" and "morph_finish"),"watershed" (pnr_watershed: the sum of "watershed_init", "watershed_compact", "watershed_flood", "watershed_label" and "watershed_finish"),"threshold" (pnr_auto_threshold: the histogram),"local_threshold" (pnr_local_threshold / pnr_local_threshold_volume: the three passes of every slab),"prune" (pnr_prune_tree: every launch of the call).  Enabled by set_profiling. */
int pnr_set_profiling(pnr_ctx *ctx, int enable);
int pnr_get_kernel_ms(pnr_ctx *ctx, const char *group, double *ms, int64_t *launches);
int pnr_reset_kernel_ms(pnr_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* PNR_HIP_H */
