// advantra_host.h -- C++ host side above the C ABI, mirroring the reference's plugin entry for the
// accelerated path: Advantra::dofunc("advantra_func", ...) -> reconstruction_func
// (/root/reference/pnr-vaa3d/Advantra_plugin.cpp:274-337, 2183-2731).  Same contract: input[0] = list of
// file names, input[1] = the 11 positional parameters as strings; returns false on a usage error
// (missing image / wrong parameter count, after printing the help), true otherwise (range errors print
// the reference's v3d_msg text and stop, as `return 0` does there).
// The Vaa3D/Qt shell itself (V3DPluginInterface2_1, QObject) cannot be built without the Vaa3D SDK;
// this is the same logic behind a plain C++ signature, driven by advantra_cli.
#pragma once
#include "../../include/pnr_hip.h"
#include <string>
#include <vector>

namespace advantra {

struct Stack {
    std::vector<unsigned char> data; // 8-bit: x fastest: i = z*w*h + y*w + x (TIFF: the kept channel copied out of the file)
    std::vector<uint16_t> data16;    // 16-bit: the same, in the host's byte order
    long long w = 0, h = 0, l = 0;
    int bits = 8;                    // bits per sample: 8 or 16
    int channels = 1, channel = 0;   // channels of the file (samples per pixel, or an ImageJ hyperstack's channels); the one kept (0-based)
    // a raw stack is mapped, not copied: 1 GiB through a zero-filled vector cost a quarter of a second that the upload pays anyway
    const unsigned char *view = nullptr;
    size_t map_len = 0;
    const unsigned char *bytes() const { return view ? view : data.data(); }
    const uint16_t *samples16() const { return view ? (const uint16_t *)view : data16.data(); }
    Stack() = default;
    Stack(const Stack &) = delete;
    Stack &operator=(const Stack &) = delete;
    ~Stack();
};

struct Result {
    float Jmin = 0, Jmax = 0;
    long long n_seeds_init = 0, n_seeds = 0, n_traces = 0, n_iterations = 0;
    std::vector<pnr_node> nodes;   // nodes[0] = dummy
    std::vector<int32_t> links;    // pairs
    std::vector<pnr_node> tree;    // reconstruct() output: tree list, tree[0] = dummy
    std::vector<int32_t> parent;   // parent index per tree node, -1 = root
    std::vector<int32_t> radius_k; // --measure-radius: k* of pnr_measure_radii per tree node (index 0 dummy: -1), else empty
    int32_t radius_thr = 0;        // ... the threshold it used (0: the relative mode)
    long long join_bridges = 0, join_trees_in = 0, join_trees_out = 0; // --join: what pnr_join_trees reported
    long long join_inserted = 0;   // --join-geodesic: the nodes pnr_join_expand inserted
    int join_thr_used = 0;         // ... and the threshold pnr_geodesic_bridges used
    double t_join = 0;
    bool have_prune = false;       // --prune: what pnr_prune_tree reported
    pnr_prune_info prune = {};
    bool have_coverage = false;    // --mask / --residual / --coverage: the final tree rendered on the traced volume (pnr_tree_coverage)
    pnr_coverage coverage = {};
    double t_render = 0;
    long long despeckle_removed = 0, despeckle_voxels = 0; // --despeckle: the components and voxels pnr_despeckle_volume cleared
    int despeckle_thr = 0;                                 // ... and the threshold it used
    double t_despeckle = 0;                                // (part of t_setup)
    std::string swc_path;
    double t_frangi = 0, t_seeds = 0, t_select = 0, t_trace = 0, t_recon = 0;
    double t_filter = 0;           // --median / --subtract-background: the pre-filter (part of t_setup)
    long long local_kept = 0;      // --local-threshold: the voxels pnr_local_threshold_volume kept
    double t_local = 0;            // ... and its time (part of t_setup)
    double t_morph = 0;            // --fill-holes / --hmax / --hdome: the morphological reconstructions (part of t_setup)
    double t_radius = 0;           // --measure-radius: the measurement (kernels, transfers, the first call's shell table)
    double t_load = 0, t_setup = 0, t_write = 0, t_total = 0; // stack file -> memory; context + upload (+ soma); SWC file; advantra_func as a whole
};

// a threshold given as a word where a flag takes "T or -1": mean|otsu|triangle|maxentropy|topP, each with an optional :LO (P: the
// brightest P per cent, up to 4 decimals; LO: the counted bins are [LO, 255]).  The word is resolved by pnr_auto_threshold on the bytes
// on which the -1 rule would have taken its mean and passed on as a number; the tool's JSON line or SWC comment then names it (thr_method).
struct ThrWord {
    bool given = false;
    pnr_threshold_opts opts = {0, 0, 0, 0};
    std::string text;
};
bool parse_threshold_word(const char *txt, ThrWord &out); // false: no such word (out is left as it was)

// switches of the head-less driver (advantra_cli flags; the plugin's compile-time TRACING_VERBOSE / saveMidres taps)
struct Settings {
    bool verbose = false;     // -v: per-trace progress and stop reasons in the reference's words (tracker.cpp:866,879,908,916; Advantra_plugin.cpp:2677)
    bool timing = false;      // --timing: the library's stage statistics on stderr (options trace_timing, seed_timing, recon_timing)
    bool save_midres = false; // --save-midres: also write the plugin's saveMidres node lists (:2098-2141): <inimg>_n0_.swc (the node graph before
                              // reconstruct()), _n0res_, _n1_, _n2_, _n2tree_
    bool single_tree = false; // --single-tree: the plugin's ENFORCE_SINGLE_TREE branch (:81, :2142-2152): only the largest tree, written to <inimg>_Advantra1.swc
    uint32_t rng_seed = 42;   // --rng-seed: replaces srand(time(NULL)) of tracker.cpp:1003,1098
    // --ranks N: this process is rank `rank` of `world` processes of one host, one GPU each, that reconstruct ONE stack together
    // (z-slabs of Frangi / seeds, sorted seeds dealt round-robin, finished traces exchanged through shared memory: INTEGRATION.md);
    // rank 0 writes the SWC.  The reference has no counterpart.
    int rank = 0, world = 1;
    pnr_shm_exchange *exchange = nullptr; // the ranks of one host: bootstrap and default transport (shared memory)
    // --exchange rccl: the collectives of the sharded path -- ncclAllReduce of (Jmin, Jmax), ncclAllGather of the scored seeds and of the
    // finished trace records at every poll -- over RCCL / xGMI instead (one rank per GPU; the shared-memory segment only carries the
    // 128-byte ncclUniqueId).  force_shard: the sharded code path also for a world of one (the only RCCL world a one-GPU box can form).
    pnr_rccl_exchange *rccl = nullptr;
    bool force_shard = false;
    // the input: --channel C (1-based; the reference's channel), --raw-type u16, and for a 16-bit stack --window LO,HI or --saturate LO,HI
    // (windowed: either was given; window as pnr_set_volume_u16 takes it)
    int channel = 1;
    bool raw_u16 = false;
    bool windowed = false;
    pnr_window window = {-1, -1, 0, 0};
    // --measure-radius: the radius column of the SWC is measured from the image at the final tree's nodes (pnr_measure_radii) instead
    // of SIG2RADIUS * the winning Frangi scale; --radius-threshold T (absolute mode, -1: the mean; sets rel_pct = 0), --radius-rel PCT
    // (relative mode, the default), --radius-max K, --radius-bg PERMILLE.  The reference has no counterpart.
    bool measure_radius = false;
    pnr_radius_opts radius = {-1, 50, 32, 1};
    // --median 2d|3d, --subtract-background R: the traced volume is pre-filtered on the GPU (pnr_filter_volume: median first, then the
    // top-hat with the flat box of half-width R) right after it is set -- for 16-bit input after windowing -- and before the soma
    // path; on every rank of --ranks N.  The SWC comment then has a #filter= line.  The reference has no counterpart.
    pnr_filter_opts filter = {0, 0};
    // --join GAP: the reconstructed forest is joined on the GPU (pnr_join_trees, zscale = zdist) right after reconstruct() and before
    // --measure-radius: fragments whose closest nodes lie within GAP xy voxels (0: any distance) are bridged, the result is re-rooted
    // and the SWC written in tree order (every parent before its children) with a #join= comment line.  --join-root soma (the default:
    // the first soma node, type 1, if there is one) or ID (a node id of the file without --join); --join-keep-largest: only component
    // 0 is written.  The reference has no counterpart (ENFORCE_SINGLE_TREE throws the other trees away).
    // --join-geodesic D [--join-threshold T] in the place of --join GAP: the fragments are joined along the signal of the traced volume
    // (pnr_geodesic_bridges; D: the largest bridge weight, 0: no limit; T as --geodesic's --threshold), the bridges' voxels become nodes
    // (the type of the bridge's node a, the smaller radius of its two nodes) and the comment line is
    // #join=geodesic:D,thr:T,bridges:K,trees:T0->T1,inserted:M.
    bool join = false, join_keep_largest = false, join_geodesic = false;
    float join_gap = 0.f;
    unsigned long long join_limit = 0;
    int join_thr = 0;
    long long join_root_id = 0; // 0: the first soma node, if any
    // --prune L[,K[,M]]: the forest -- after --join / --join-geodesic, before --measure-radius -- loses its side branches shorter than
    // max(L, K x the radius of the node they leave) and its trees lower than M xy voxels on the GPU (pnr_prune_tree, zscale = zdist, the
    // radii the file would be written with); the kept nodes stay in their order and the comment block gains
    // #prune=length:L,radius:K,min_tree:M,removed:N,segments:S behind #join.  Without --join soma nodes are roots and go only under M.
    // With --skeleton --swc the same is applied to the skeleton before the file is written (radius = the distance transform).
    bool prune = false;
    pnr_prune_opts prune_opts = {1.f, 0.f, 0.f, 0.f}; // (zscale is filled in where it runs)
    // --mask OUT, --residual OUT, --coverage: the final tree -- after --join and --measure-radius, with the f32 radius each SWC line is
    // written from and zscale = zdist -- is rendered on the traced volume (pnr_tree_coverage): OUT receives the mask (255 under the
    // tree) / the residual (the volume where the tree is not) as a stack (save_stack_u8), and the comment block gains a #coverage= line.
    // The reference has no counterpart.
    std::string mask_out, residual_out;
    bool coverage = false;
    // --despeckle MIN[,THR[,CONN]]: foreground components ({V >= THR}, -1: the mean; CONN 6 or 26) of fewer than MIN voxels are cleared on
    // the GPU (pnr_despeckle_volume) after the pre-filters -- for 16-bit input after windowing -- and before the soma path; on every rank
    // of --ranks N.  The SWC comment then has a #despeckle= line behind #filter.  The reference has no counterpart.
    bool despeckle = false;
    pnr_components_opts despeckle_opts = {-1, 26, 1};
    // --fill-holes 2d|3d, --hmax H | --hdome H (1..255): the grey image's shape is repaired on the GPU (pnr_morph_volume) after the
    // pre-filters -- for 16-bit input after windowing -- and before --despeckle; the fill (PNR_MORPH_FILL with C = 4 in every slice, or
    // C = 6) runs first, then the h transform (C = 26); on every rank of --ranks N, and in every tool mode that takes the volume set-up.
    // The SWC comment then has a #morph= line behind #filter.  The reference has no counterpart.
    int fill_holes = 0; // 0: off, 4: 2d, 6: 3d (the connectivity)
    int hmax = 0, hdome = 0;
    bool morph() const { return fill_holes || hmax || hdome; }
    // --local-threshold R[,OFFSET[,SCALE_256]] [--local-binary]: the local threshold (pnr_local_threshold_volume, floor 1) is the next step of
    // the volume set-up, after --fill-holes / --hmax / --hdome and before --despeckle, on every rank and in every tool mode that takes the
    // set-up.  The SWC comment then has a #local= line behind #morph.  The reference has no counterpart.
    pnr_local_opts local = {0, 0, 256, 1, 0, 0}; // r = 0: off
    // the words given to --threshold (the tool modes), --coverage-threshold, --radius-threshold, --join-threshold and the THR of --despeckle
    ThrWord thr_word, coverage_word, radius_word, join_word, despeckle_word;
};
Settings &settings();

void print_help();
void print_flags(); // advantra_cli --help: print_help() and the driver's own flags
// simple_loadimage_wrapper's role (Advantra_plugin.cpp:2241): a multi-page uncompressed TIFF of 8- or 16-bit unsigned samples
// (either byte order; several samples per pixel, chunky or planar, or an ImageJ hyperstack's channels), or ".raw" (u8, or u16
// little-endian with raw_u16; dims from `raw_dims` = "w,h,l").  Keeps channel `channel` (0-based) only.  Returns false with a
// message in `err`.
bool load_stack(const std::string &path, const std::string &raw_dims, Stack &out, std::string &err, int channel = 0, bool raw_u16 = false);
// advantra_cli --info: loads the stack and prints one JSON line {"w","h","l","bits","channels","channel","min","max","sum"} of the
// kept channel (channel printed 1-based); no GPU is touched
bool print_info(const std::string &path, const std::string &raw_dims, int channel, bool raw_u16);
// An SWC file as the tree distance takes it: lines `n type x y z r parent`; `#` comments and blank lines are skipped; ids may be
// written as 3.0 and come in any order; a parent id that is not in the file means "none" (as -1 does).  Numbers are read as
// doubles and rounded to f32.  A duplicate id, a line of fewer than 7 fields or a field that is no number fails with
// "<file>:<line>: ..." in err.  parent[i] = the index of the parent's node in file order, -1 = none.
struct SwcTree {
    std::vector<float> xyz, radius; // n x 3; n
    std::vector<int32_t> parent, type;
    std::vector<long long> id;
    long long n() const { return (long long)id.size(); }
};
bool load_swc(const std::string &path, SwcTree &out, std::string &err);
// advantra_cli --swc-info: one JSON line {"nodes", "roots", "segments", "length", "bbox": [x0, y0, z0, x1, y1, z1]} (segments = nodes
// with a parent; length = the f64 sum of their lengths in file order; bbox null for an empty file); no GPU is touched
bool print_swc_info(const std::string &path);
// advantra_cli --distance A.swc B.swc: pnr_tree_distance of the two files on `device` (a context of pnr_default_params) as one JSON
// line; per_node (not empty): <per_node>_ab.csv / _ba.csv with one row `id,d` per sample point of A / of B (id = the SWC id of the
// point's node) under a header line
bool print_tree_distance(const std::string &a, const std::string &b, const pnr_distance_opts &opts, int device, const std::string &per_node);
// advantra_cli --join-swc IN.swc OUT.swc: pnr_join_trees of the file on `device`; OUT.swc has the nodes in tree order with ids 1..n, the
// type and radius columns carried over and a #join= comment line; root_id: an SWC id of IN (0: none); keep_largest: component 0 only.
// Prints one JSON line {"nodes", "trees_in", "trees_out", "bridges", "longest_bridge", "rounds"}.
bool join_swc_file(const std::string &in, const std::string &out, float gap, float zscale, long long root_id, bool keep_largest, int device);
// advantra_cli --join-swc IN.swc OUT.swc --join-geodesic D -i stack: the fragments of the file joined along the signal of the stack
// (pnr_geodesic_bridges on `device`; the volume setup of --geodesic, zscale >= 1 is the context's zdist; opts.limit = D, 0: no limit),
// the bridges' voxels inserted as nodes (pnr_join_expand: the type of the bridge's node a, the smaller radius of its two nodes) and the
// result re-rooted (pnr_join_reroot); OUT.swc as --join-swc writes it, with #join=geodesic:D,thr:T,bridges:K,trees:T0->T1,inserted:M.
// Prints one JSON line {"nodes", "n_trees_in", "n_trees_lost", "n_trees_out", "n_bridges", "n_inserted", "w_max", "thr_used", "n_src",
// "n_src_dropped", "limit", "zdist", "rounds"}.
bool join_swc_geodesic_file(const std::string &in, const std::string &out, const pnr_geojoin_opts &opts, const std::vector<char *> &infiles, const std::string &raw_dims,
                            float zscale, long long root_id, bool keep_largest, int device);
// advantra_cli --render-swc IN.swc: the file rendered into a stack (pnr_tree_coverage on `device`).  With a stack (infiles[0]; the same
// volume setup as tracing: channel, window, pre-filters of settings()) the tree is measured on what would be traced: `mask` / `residual`
// (not empty) are written with save_stack_u8, `per_node` is a CSV `id,vox,fg,sum` per node under a header line, and one JSON line has
// the fields of pnr_coverage, then "nodes" and "items".  Without a stack, raw_dims = "w,h,l" gives the grid and only the mask is
// written (pnr_render_tree); the JSON line is {"n_vox", "n_tree", "nodes", "items"}.
// advantra_cli --prune-swc IN.swc [OUT.swc]: pnr_prune_tree of the file on `device` (opts: zscale and the three thresholds in xy voxels).
// OUT.swc (not empty): the kept nodes in the input's order with ids 1..m, type and radius carried over, under a comment block that ends in
// #prune=length:L,radius:K,min_tree:M,removed:N,segments:S.  per_node (not empty): a CSV `id,keep,height,path,order,seg_id` per input node
// under a header line, the lengths in xy voxels (units / 256, exact in %.17g).  Prints one JSON line with the fields of pnr_prune_info, the
// lengths in voxels.
bool prune_swc_file(const std::string &in, const std::string &out, const pnr_prune_opts &opts, const std::string &per_node, int device);
// the #prune= line of an SWC comment block (no newline)
std::string prune_comment(const pnr_prune_opts &opts, const pnr_prune_info &info);
struct RenderJob {
    std::string swc, mask, residual, per_node;
    pnr_render_opts opts = {1.f, 1.f, 0.f, -1};
};
bool render_swc_file(const RenderJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, int device);
// advantra_cli --components -i stack: the connected components of the stack's foreground (pnr_label_components on `device`; the same
// volume setup as --render-swc: channel, window, pre-filters of settings(); zscale >= 1 is the zdist of --subtract-background).  One JSON
// line with the fields of pnr_components_info; `labels` (not empty): the label volume as bare little-endian int32; `per_component` (not
// empty): a CSV `id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax` per kept component under a header line, the centroid as %.3f of the f64
// quotient.  Run on a file written by --residual, this lists what the trace missed.
struct ComponentsJob {
    pnr_components_opts opts = {-1, 26, 1};
    std::string labels, per_component;
};
bool components_file(const ComponentsJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device);
// advantra_cli --edt -i stack: the exact distance transform of the stack's foreground (pnr_distance_transform on `device`; the same volume
// setup as --components; zscale >= 1 is the context's zdist).  One JSON line {"n_vox", "n_fg", "n_capped", "thr_used", "rmax", "zdist",
// "d_max", "max_at": [x, y, z]} (d_max = sqrtf(d2_max); max_at null without foreground); `out` (not empty): d = sqrtf(D2) of every voxel as
// bare little-endian f32; `at` and `per_node` (both or neither): a CSV `id,d` per node of the SWC file `at` under a header line, d as %.9g
// (-1: a position that is not finite).
struct EdtJob {
    pnr_edt_opts opts = {-1, 64};
    std::string out, at, per_node;
};
bool edt_file(const EdtJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device);
// advantra_cli --geodesic -i stack --from tree.swc: the gray-weighted geodesic distance of every voxel of the stack to the tree
// (pnr_geodesic_distance on `device`; the same volume setup as --edt; zscale >= 1 is the context's zdist).  Sources: the sample points of
// `from` (pnr_tree_sample at step 1, zscale 1), each labelled with the SWC id of its owner node.  One JSON line {"n_vox", "n_pass",
// "n_reached", "n_src", "n_src_dropped", "thr_used", "dmax", "zdist", "d_max", "len_max" (d_max / 64: xy voxels at the brightest cost),
// "max_at": [x, y, z] (null when nothing is reached), "rounds"}.  `to` and `per_node` (both or neither): a CSV `id,d,label` per node of the
// SWC file `to` under a header line (-1,-1: unreached or not finite); `paths` (needs `to`): every complete path as a chain of SWC nodes
// from the target's voxel to the source voxel (the root of the chain), each chain under a comment line
// `# path <target id> -> <label>: <k> voxels, cost <d>` (walked in the same call with a cap of min(PNR_GEO_MAX_PATH, N, max(64, 2^26 / nodes))
// voxels; a longer path is left out, and a line on stderr says how many were); `out` (not empty): <out>_d.raw (u32) and <out>_label.raw (i32), little-endian.
struct GeodesicJob {
    pnr_geo_opts opts = {0, 0x7fffffffu, nullptr};
    std::string from, to, per_node, paths, out;
};
bool geodesic_file(const GeodesicJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device);
// advantra_cli --skeleton -i stack: the stack's foreground thinned to a one-voxel-wide curve skeleton (pnr_skeletonize on `device`; the same
// volume setup as --components; zscale >= 1 is the context's zdist, which only the radii see).  One JSON line with the fields of
// pnr_thin_info, then "trees": the 26-components of the skeleton.  `out` (not empty): the 0 / 255 volume as a TIFF, or bare bytes for a .raw
// name.  `swc` (not empty): the skeleton as a tree -- pnr_skeleton_forest, then pnr_join_reroot at the voxel with the largest D2 (the
// smallest index on ties); coordinates = the voxel's x, y, z, radius = sqrtf(D2) of pnr_distance_transform at those points (thr = thr_used,
// rmax = 64), type 2, ids 1..n in tree order with every parent before its children; the comment block ends in
// #skeleton=thr:T,rounds:R,voxels:K,trees:C, followed by #prune= (as --prune-swc writes it) when the job prunes.
struct SkeletonJob {
    pnr_thin_opts opts = {-1, 0};
    std::string out, swc;
    bool prune = false; // --prune L[,K[,M]]: the tree of `swc` is pruned before it is written (pnr_prune_tree, zscale = the context's zdist)
    pnr_prune_opts prune_opts = {1.f, 0.f, 0.f, 0.f};
};
bool skeleton_file(const SkeletonJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device);
// advantra_cli --morph -i stack [--fill-holes 2d|3d] [--hmax H | --hdome H] --morph-out OUT: the stack after the volume set-up of tracing,
// whose last steps are these flags (pnr_morph_volume on `device`), written as a TIFF, or as bare bytes for a .raw name.  One JSON line
// {"w", "h", "l", "stages": [{"op": "fill" | "hmax" | "hdome", "h", then the fields of pnr_morph_info}, ...]}, a stage per flag in the order run.
bool morph_file(const std::string &out, const std::vector<char *> &infiles, const std::string &raw_dims, int device);
// advantra_cli --watershed -i stack (--markers-swc tree.swc [--markers-by tree|node] | --markers FILE.raw) [--relief FILE.raw] --labels OUT.raw
// [--levels OUT.raw]: the marker-controlled watershed of the stack after the volume set-up of tracing (pnr_watershed on `device`).  The
// markers are the nodes of the SWC file, each labelled with 1 + the number of its tree in the order of pnr_join_reroot (by_node: with its
// SWC id, 1 .. 2^31 - 1) -- the voxels per neuron --, or a file of w h l little-endian int32.  relief: w h l bytes (empty: 255 - the
// volume).  labels: every voxel's label as bare little-endian int32; levels (not empty): the pass heights as bare bytes.  One JSON line
// {"w", "h", "l", "markers_by": "tree" | "node" | "volume", "n_markers", then the fields of pnr_watershed_info}.
struct WatershedJob {
    pnr_watershed_opts opts = {-1, 26};
    std::string markers_swc, markers_raw, relief, labels, levels;
    bool by_node = false;
};
bool watershed_file(const WatershedJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, int device);
// advantra_cli --auto-threshold -i stack [--threshold-lo LO] [--histogram FILE.csv]: every threshold rule on the stack after the volume
// set-up of tracing, from one histogram pass (pnr_auto_threshold on `device`, then pnr_threshold_from_hist on its counts).  One JSON line
// {"w", "h", "l", "n_vox", "lo", "mean": {"thr", "n_fg"}, "otsu": ..., "triangle": ..., "maxentropy": ..., "top1": ...} (maxentropy with
// lo = 0 whatever LO is; null where the reference's int histogram cannot hold a bin); histogram (not empty): a CSV `v,count` under a header line.
bool auto_threshold_file(int lo, const std::string &histogram, const std::vector<char *> &infiles, const std::string &raw_dims, int device);
// save_nodelist (Advantra_plugin.cpp:480-523).  radius (optional, one entry per node): a node whose entry is >= 0 writes it as its
// radius instead of sig2r * sig
bool save_nodelist(const std::vector<pnr_node> &nodes, const std::vector<int32_t> &links, const std::string &swcname,
                   int type = -1, float sig2r = 1.f, const std::string &name = "", const std::string &comment = "",
                   const std::vector<float> *radius = nullptr);
// the same writer for a tree list (each node has 0 or 1 link: its parent)
bool save_treelist(const std::vector<pnr_node> &tree, const std::vector<int32_t> &parent, const std::string &swcname, int type = -1,
                   float sig2r = 1.f, const std::string &name = "", const std::string &comment = "",
                   const std::vector<float> *radius = nullptr);
// the radius column of measured nodes: k* >= 1 -> k*, 0 -> 0.5; nodes that were not measured (k = -1) and soma nodes (type 1) keep
// sig2r * sig (entry -1)
std::vector<float> measured_radius_column(const std::vector<pnr_node> &tree, const std::vector<int32_t> &k);
// 0 = ok, -1 = usage error (dofunc returns false), -2 = range error (dofunc "return 0"), -3 = runtime failure
int parse_params(const std::vector<std::string> &paras, pnr_params &p, std::string &err);
// reconstruction_func (Advantra_plugin.cpp:2183-2731) from the point where the stack is in memory (:2255): the caller keeps
// ownership of `data1d` (u8, x fastest).  Writes <inimg_file>_Advantra.swc; false = a library call failed (message printed).
// data16 != nullptr: a 16-bit stack instead (data1d unused), windowed to 8 bits on the GPU with `win` (pnr_set_volume_u16; nullptr
// = [min, max]); the SWC comment then ends in #bits=16 and #window=lo,hi.
bool reconstruction_func(const unsigned char *data1d, long long w, long long h, long long l, const std::string &inimg_file,
                         const std::vector<std::string> &paras, pnr_params p, int device = 0, Result *result = nullptr,
                         const uint16_t *data16 = nullptr, const pnr_window *win = nullptr);
bool advantra_func(const std::vector<char *> &infiles, const std::vector<char *> &paras, int device = 0,
                   const std::string &raw_dims = "", Result *result = nullptr);

} // namespace advantra
