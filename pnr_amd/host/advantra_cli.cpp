// advantra_cli -- head-less driver with the reference's command-line contract:
//   vaa3d -x Advantra -f advantra_func -i <inimg_file> -p <11 parameters>      (README.md:15-18)
// becomes
//   advantra_cli [-v] [--save-midres] [--rng-seed N] [-g device] [-d w,h,l for .raw] -f advantra_func -i <inimg_file> -p <11 parameters>
// (-p takes the rest of the line, as in vaa3d: put the driver's own flags before it)
//   --ranks N [--share-gpu]: N processes of this host, one GPU each (device = -g + rank; --share-gpu: all on -g, for rehearsals),
//   reconstruct the ONE stack together; the processes are forked before anything touches a GPU and joined through shared memory.
//   --channel C: the channel to trace (1-based, default 1: the reference's `channel`); --raw-type u8|u16 (u16: little-endian);
//   a 16-bit stack is windowed to 8 bits on the GPU: [min, max] by default, --window LO,HI, or --saturate LO,HI (percent of the voxels
//   clipped to 0 / to 255, up to 4 decimals);  --info: print {"w","h","l","bits","channels","channel","min","max","sum"} of the
//   stack's channel as one JSON line and exit (no GPU).
//   --measure-radius: the SWC's radius column is measured from the image at the final tree's nodes (pnr_measure_radii) -- k* voxels, 0.5
//   for a node thinner than one voxel; soma nodes keep theirs -- and the comment block ends in #radius=measured,thr=<t or rel:PCT>,rmax=K,
//   bg=PERMILLE.  --radius-rel PCT (1..100; the default mode, 50) or --radius-threshold T (0..255, -1: the stack's mean), --radius-max K
//   (1..64, default 32), --radius-bg PERMILLE (0..999, default 1): out-of-range values are usage errors.  --help lists all flags.
//   --median 2d|3d, --subtract-background R (1..64): the stack is pre-filtered on the GPU before it is traced (pnr_filter_volume: a 3 x 3
//   median in every slice or a 3 x 3 x 3 one, then a top-hat with a flat box of half-width R); the comment block then has the line
//   #filter=median:<2d|3d|off>,tophat:<R|off> behind #bits / #window and in front of #radius.  Any other value is a usage error.
//   --swc-info FILE.swc: {"nodes","roots","segments","length","bbox"} of an SWC file as one JSON line (no GPU; the sibling of --info).
//   --distance A.swc B.swc [--distance-step S] [--distance-threshold T] [--zscale Z] [--per-node PREFIX]: the tree distance of the two
//   files (pnr_tree_distance on device -g, a context of pnr_default_params) as one JSON line; --per-node also writes PREFIX_ab.csv and
//   PREFIX_ba.csv, one row `id,d` per sample point.  Any failure (an unreadable or malformed file, a bad value) exits non-zero.
//   --join GAP [--join-root soma|ID] [--join-keep-largest]: while tracing, the reconstructed forest is joined into one tree on the GPU
//   (pnr_join_trees with zscale = zdist; GAP in xy voxels, 0 = any distance), re-rooted (default: at the first soma node, if any; ID = a
//   node id of the file without --join) and written in tree order; the comment block gains #join=gap:G,bridges:K,trees:T0->T1.
//   --join-geodesic D [--join-threshold T] [--join-root soma|ID] [--join-keep-largest] in the place of --join GAP: the forest is joined along
//   the signal (pnr_geodesic_bridges: the minimum spanning forest of the fragments under gray-weighted path cost, no bridge heavier than D,
//   0 = no limit), the bridges' voxels become nodes; the comment block gains #join=geodesic:D,thr:T,bridges:K,trees:T0->T1,inserted:M.
//   --join-swc IN.swc OUT.swc --join-geodesic D -i stack [--zscale Z] [--join-threshold T]: the same on a file and a stack; one JSON line.
//   --join-swc IN.swc OUT.swc [--join GAP] [--zscale Z] [--join-root ID] [--join-keep-largest]: the same on a file (device -g); one JSON
//   line {"nodes","trees_in","trees_out","bridges","longest_bridge","rounds"}.
//   --prune-swc IN.swc [OUT.swc] [--prune-length L] [--prune-radius K] [--prune-min-tree M] [--zscale Z] [--per-node FILE.csv]: the file's side
//   branches shorter than max(L, K x the radius of the node they leave) and its trees lower than M (xy voxels) removed on the GPU
//   (pnr_prune_tree on device -g); OUT.swc has the kept nodes in the input's order with ids 1..m under a comment block that ends in
//   #prune=length:L,radius:K,min_tree:M,removed:N,segments:S; one JSON line with the fields of pnr_prune_info, lengths in voxels; the CSV is
//   `id,keep,height,path,order,seg_id` per input node.  --prune L[,K[,M]]: the same while tracing (after --join / --join-geodesic, before
//   --measure-radius, zscale = zdist; #prune= behind #join) and with --skeleton --swc (before the file is written; #prune= behind #skeleton=).
//   --render-swc IN.swc -i stack [--mask OUT] [--residual OUT] [--per-node FILE.csv] [--zscale Z] [--radius-scale S] [--radius-add A]
//   [--coverage-threshold T]: the file rendered into the stack on the GPU (pnr_tree_coverage on device -g; the stack goes through the
//   same volume setup as tracing: --channel, --window / --saturate, --median, --subtract-background); one JSON line with the fields of
//   pnr_coverage, then "nodes" and "items"; the CSV is `id,vox,fg,sum` per node.  Without -i, -d w,h,l gives the grid and only --mask is
//   allowed.  While tracing, --mask OUT, --residual OUT and --coverage render the final tree (after --join and --measure-radius, zscale =
//   zdist) and add #coverage=thr:T,covered:..,on_signal:..,intensity:..,tree_voxels:N to the comment block.
//   --despeckle MIN[,THR[,CONN]]: while tracing, the foreground components (voxels >= THR, default -1: the stack's mean; CONN 6 or 26,
//   default 26) of fewer than MIN voxels are cleared on the GPU (pnr_despeckle_volume) after --median / --subtract-background and on every
//   rank; the comment block gains #despeckle=min:M,thr:T,conn:C,removed:K,voxels:V (T: the threshold used) behind #filter.
//   --components -i stack [--threshold T] [--connectivity 6|26] [--min-size M] [--labels OUT.raw] [--per-component FILE.csv]: the
//   connected components of the stack (pnr_label_components on device -g; the same volume setup as --render-swc) as one JSON line with
//   the fields of pnr_components_info; --labels writes bare little-endian int32, --per-component one line
//   `id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax` per kept component.  On a --residual file (.raw with -d w,h,l): what the trace missed.
//   --edt -i stack [--threshold T] [--edt-max R] [--zscale Z] [--edt-out OUT.raw] [--at tree.swc --per-node FILE.csv]: the exact Euclidean
//   distance transform of the stack's foreground (pnr_distance_transform on device -g; the same volume setup as --components; Z >= 1,
//   default 1, is the context's zdist) as one JSON line n_vox, n_fg, n_capped, thr_used, rmax, zdist, d_max, max_at; --edt-out writes
//   d = sqrtf(D2) as bare little-endian f32, --at / --per-node one line `id,d` per node of the SWC file.
//   --geodesic -i stack --from tree.swc [--to other.swc --per-node FILE.csv [--paths OUT.swc]] [--threshold T] [--geo-max D] [--zscale Z]
//   [--geo-out PREFIX]: the gray-weighted geodesic distance of every voxel to the tree (pnr_geodesic_distance on device -g; the volume setup
//   of --edt; sources: the tree's sample points labelled with their node ids) as one JSON line; --per-node writes `id,d,label` per node of
//   other.swc, --paths every complete path as a chain of SWC nodes, --geo-out PREFIX_d.raw (u32) and PREFIX_label.raw (i32).
//   --skeleton -i stack [--threshold T] [--skeleton-rounds R] [--zscale Z] [--skeleton-out OUT.tif|.raw] [--swc OUT.swc]: the stack's foreground
//   thinned to a one-voxel-wide curve skeleton (pnr_skeletonize on device -g; the volume setup of --components) as one JSON line with the
//   fields of pnr_thin_info and "trees"; --skeleton-out writes the 0 / 255 volume, --swc the skeleton as a tree (pnr_skeleton_forest, then
//   pnr_join_reroot at the thickest voxel; radius = the distance transform at the voxel with zdist = Z; the comment block ends in
//   #skeleton=thr:T,rounds:R,voxels:K,trees:C): an independent baseline for --distance, and fragments for --join-swc --join-geodesic.
//   --fill-holes 2d|3d, --hmax H | --hdome H (1..255): the last steps of the volume set-up, after --median / --subtract-background and before
//   --despeckle, on every rank: grey-level fill-holes (pnr_morph_volume PNR_MORPH_FILL, 4-connected in every slice or 6-connected), then the
//   h-maxima or the h-domes (26-connected).  Every mode that takes the set-up gets them: a tracing run -- the comment block gains
//   #morph=fill:<2d|3d|off>,hmax:<H|off>,hdome:<H|off> behind #filter --, --skeleton, --components, --edt, --geodesic, --render-swc and
//   --join-swc --join-geodesic.  --morph -i stack [those flags] --morph-out OUT.tif|.raw: the resulting stack and one JSON line with the
//   fields of pnr_morph_info of each stage run.
//   --local-threshold R[,OFFSET[,SCALE_256]] [--local-binary]: the next step of the volume set-up, after --fill-holes / --hmax / --hdome and before
//   --despeckle, on every rank and in every tool mode that takes the set-up: the local threshold of pnr_local_threshold_volume (floor 1); the
//   comment block gains #local=r:R,offset:C,scale:K,kept:N behind #morph.
//   --auto-threshold -i stack [--threshold-lo LO] [--histogram FILE.csv]: one JSON line with thr and n_fg of mean, otsu, triangle, maxentropy
//   and top1 from one histogram pass on the GPU (pnr_auto_threshold); --histogram writes `v,count`.
//   Every flag that takes "T or -1" (--threshold, --coverage-threshold, --radius-threshold, --join-threshold, the THR of --despeckle) also
//   takes mean|otsu|triangle|maxentropy|topP[:LO]; the tool's JSON line or SWC comment then gains thr_method.
//   --watershed -i stack (--markers-swc tree.swc [--markers-by tree|node] | --markers FILE.raw) [--relief FILE.raw] [--threshold T]
//   [--connectivity 4|8|6|26] --labels OUT.raw [--levels OUT.raw]: the marker-controlled watershed of the stack after the same volume set-up
//   (pnr_watershed): the label volume, with --markers-by tree the voxels per traced neuron, and one JSON line with the fields of
//   pnr_watershed_info.
// Exit code: 0 = dofunc returned true, 1 = dofunc returned false (usage error).
#include "advantra_host.h"
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

// "a,b" of two non-negative decimals with at most `decimals` digits after the point -> a and b times 10^decimals
static bool parse_pair(const char *txt, int decimals, long long &a, long long &b)
{
    long long v[2] = {0, 0};
    const char *q = txt;
    for (int k = 0; k < 2; k++) {
        if (!isdigit((unsigned char)*q)) return false;
        long long x = 0;
        int nd = 0;
        for (; isdigit((unsigned char)*q); q++) {
            if (++nd > 9) return false;
            x = 10 * x + (*q - '0');
        }
        int frac = 0;
        if (*q == '.' && decimals > 0) {
            q++;
            for (; isdigit((unsigned char)*q); q++) {
                if (++frac > decimals) return false;
                x = 10 * x + (*q - '0');
            }
        }
        for (; frac < decimals; frac++) x *= 10;
        v[k] = x;
        if (k == 0 && *q++ != ',') return false;
    }
    if (*q) return false;
    a = v[0];
    b = v[1];
    return true;
}

// the whole of txt as a finite decimal number
static bool parse_float(const char *txt, float &out)
{
    char *end = nullptr;
    const double v = strtod(txt, &end);
    if (!*txt || *end || !(v == v) || v > 3e38 || v < -3e38) return false;
    out = (float)v;
    return true;
}

// the whole of txt as a decimal integer in [lo, hi]
static bool parse_int(const char *txt, long lo, long hi, long &out)
{
    char *end = nullptr;
    const long v = strtol(txt, &end, 10);
    if (!*txt || *end || v < lo || v > hi) return false;
    out = v;
    return true;
}

// "T or -1", or a threshold word (advantra_host.h ThrWord): the word leaves -1 in `out` until it is resolved on the volume
static bool parse_thr(const char *txt, long &out, advantra::ThrWord &word)
{
    if (parse_int(txt, -1, 255, out)) return true;
    if (!advantra::parse_threshold_word(txt, word)) return false;
    out = -1;
    return true;
}

int main(int argc, char **argv)
{
    std::vector<char *> infiles, paras;
    std::string func = "advantra_func", raw_dims;
    int device = 0, ranks = 1;
    bool share_gpu = false;
    std::string transport = "shm";
    bool info = false, window = false, saturate = false, help = false;
    bool radius_abs = false, radius_rel = false, radius_flag = false;
    bool distance = false, dist_flag = false;
    std::string swc_info, dist_a, dist_b, per_node;
    pnr_distance_opts dist_opts = {1.f, 1.f, 2.f};
    // --join and its companions are parsed into locals: they reach the tracing Settings only where the run traces (not under --join-swc)
    bool zscale_flag = false, join_flag = false, join_root_soma = false, join_given = false, join_keep_largest = false;
    float join_gap = 0.f;
    long join_root_id = 0;
    bool join_geodesic = false, join_thr_flag = false;
    unsigned long long join_limit = 0;
    int join_thr = 0;
    std::string join_in, join_out;
    std::string prune_in, prune_out;
    bool prune_flag = false, prune_given = false;
    pnr_prune_opts prune_opts = {1.f, 0.f, 0.f, 0.f};
    advantra::RenderJob render;
    std::string mask_out, residual_out;
    bool coverage = false, render_flag = false, per_node_flag = false;
    advantra::ComponentsJob comp;
    bool components = false, comp_flag = false, thr_flag = false;
    advantra::EdtJob edt_job;
    bool edt = false, edt_flag = false;
    advantra::GeodesicJob geo_job;
    bool geo = false, geo_flag = false;
    advantra::SkeletonJob skel_job;
    bool skeleton = false, skel_flag = false;
    bool morph = false;
    std::string morph_out;
    bool auto_thr = false, auto_flag = false;
    int auto_lo = 0;
    std::string auto_hist;
    advantra::WatershedJob ws_job;
    bool ws = false, ws_flag = false, ws_by_flag = false, conn_planar = false, comp_only_flag = false; // (--min-size, --per-component: of --components alone)
    advantra::Settings &S0 = advantra::settings();
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--geodesic")) { geo = true; continue; }
        if (!strcmp(argv[i], "--geo-max")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 1, 0x7fffffffL, v)) { fprintf(stderr, "--geo-max D: the largest path cost kept, an integer from 1 to 2147483647\n"); return 1; }
            geo_job.opts.dmax = (uint32_t)v;
            geo_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--from") || !strcmp(argv[i], "--to") || !strcmp(argv[i], "--paths") || !strcmp(argv[i], "--geo-out")) {
            const std::string flag = argv[i];
            const std::string name = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (name.empty()) {
                fprintf(stderr, "%s\n", flag == "--from" ? "--from tree.swc" : flag == "--to" ? "--to other.swc" : flag == "--paths" ? "--paths OUT.swc" : "--geo-out PREFIX");
                return 1;
            }
            (flag == "--from" ? geo_job.from : flag == "--to" ? geo_job.to : flag == "--paths" ? geo_job.paths : geo_job.out) = name;
            geo_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--watershed")) { ws = true; continue; }
        if (!strcmp(argv[i], "--markers-swc") || !strcmp(argv[i], "--markers") || !strcmp(argv[i], "--relief") || !strcmp(argv[i], "--levels")) {
            const std::string flag = argv[i];
            const std::string name = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (name.empty() || (flag != "--markers-swc" && (name.size() <= 4 || name.substr(name.size() - 4) != ".raw"))) {
                fprintf(stderr, "%s\n", flag == "--markers-swc" ? "--markers-swc FILE.swc" : flag == "--markers" ? "--markers FILE.raw: a .raw file name (bare little-endian int32)"
                                        : flag == "--relief"    ? "--relief FILE.raw: a .raw file name (bare bytes)"
                                                                : "--levels OUT.raw: a .raw file name (bare bytes)");
                return 1;
            }
            (flag == "--markers-swc" ? ws_job.markers_swc : flag == "--markers" ? ws_job.markers_raw : flag == "--relief" ? ws_job.relief : ws_job.levels) = name;
            ws_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--markers-by")) {
            const std::string by = i + 1 < argc ? argv[++i] : "";
            if (by != "tree" && by != "node") { fprintf(stderr, "--markers-by tree|node\n"); return 1; }
            ws_job.by_node = by == "node";
            ws_flag = ws_by_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--skeleton")) { skeleton = true; continue; }
        if (!strcmp(argv[i], "--skeleton-rounds")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 0, 0x7fffffffL, v)) { fprintf(stderr, "--skeleton-rounds R: the thinning rounds run at the most, an integer, 0 (until nothing is deleted) or more\n"); return 1; }
            skel_job.opts.max_rounds = (int32_t)v;
            skel_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--skeleton-out") || !strcmp(argv[i], "--swc")) {
            const bool out = !strcmp(argv[i], "--skeleton-out");
            const std::string name = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (name.empty()) { fprintf(stderr, "%s\n", out ? "--skeleton-out OUT: a .tif or .raw file name" : "--swc OUT.swc"); return 1; }
            (out ? skel_job.out : skel_job.swc) = name;
            skel_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--components")) { components = true; continue; }
        if (!strcmp(argv[i], "--edt")) { edt = true; continue; }
        if (!strcmp(argv[i], "--edt-max")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 1, PNR_EDT_MAX_R, v)) { fprintf(stderr, "--edt-max R: the largest distance looked for, an integer from 1 to %d\n", PNR_EDT_MAX_R); return 1; }
            edt_job.opts.rmax = (int32_t)v;
            edt_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--edt-out") || !strcmp(argv[i], "--at")) {
            const bool out = !strcmp(argv[i], "--edt-out");
            const std::string name = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (name.empty() || (out && (name.size() <= 4 || name.substr(name.size() - 4) != ".raw"))) {
                fprintf(stderr, "%s\n", out ? "--edt-out OUT.raw: a .raw file name (bare little-endian float32)" : "--at tree.swc");
                return 1;
            }
            (out ? edt_job.out : edt_job.at) = name;
            edt_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--threshold")) {
            long v = 0;
            if (!parse_thr(i + 1 < argc ? argv[++i] : "", v, S0.thr_word)) { fprintf(stderr, "--threshold T: an integer from 0 to 255, or -1 for the stack's mean\n"); return 1; }
            comp.opts.thr = edt_job.opts.thr = geo_job.opts.thr = skel_job.opts.thr = ws_job.opts.thr = (int32_t)v;
            thr_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--connectivity")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 4, 26, v) || (v != 4 && v != 8 && v != 6 && v != 26)) { fprintf(stderr, "--connectivity 6|26 (--watershed: 4|8|6|26)\n"); return 1; }
            comp.opts.connectivity = ws_job.opts.connectivity = (int32_t)v;
            conn_planar = v == 4 || v == 8;
            comp_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--min-size")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 1, 0x7fffffffffffffffL, v)) { fprintf(stderr, "--min-size M: an integer from 1\n"); return 1; }
            comp.opts.min_size = v;
            comp_flag = comp_only_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--labels") || !strcmp(argv[i], "--per-component")) {
            const bool lab = !strcmp(argv[i], "--labels");
            const std::string name = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (name.empty() || (lab && (name.size() <= 4 || name.substr(name.size() - 4) != ".raw"))) {
                fprintf(stderr, "%s\n", lab ? "--labels OUT.raw: a .raw file name (bare little-endian int32)" : "--per-component FILE.csv");
                return 1;
            }
            (lab ? comp.labels : comp.per_component) = name;
            comp_flag = true;
            if (!lab) comp_only_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--despeckle")) {
            const std::string txt = i + 1 < argc ? argv[++i] : "";
            std::vector<std::string> part(1);
            for (char ch : txt) {
                if (ch == ',') part.emplace_back();
                else part.back() += ch;
            }
            long m = 0, t = -1, cn = 26;
            if (part.size() > 3 || !parse_int(part[0].c_str(), 1, 0x7fffffffffffffffL, m) || (part.size() > 1 && !parse_thr(part[1].c_str(), t, S0.despeckle_word)) ||
                (part.size() > 2 && (!parse_int(part[2].c_str(), 6, 26, cn) || (cn != 6 && cn != 26)))) {
                fprintf(stderr, "--despeckle MIN[,THR[,CONN]]: MIN an integer from 1, THR 0..255 or -1 for the stack's mean, CONN 6 or 26\n");
                return 1;
            }
            S0.despeckle = true;
            S0.despeckle_opts = pnr_components_opts{(int32_t)t, (int32_t)cn, m};
            continue;
        }
        if (!strcmp(argv[i], "--info")) { info = true; continue; }
        if (!strcmp(argv[i], "--channel") && i + 1 < argc) {
            char *end = nullptr;
            const long c = strtol(argv[++i], &end, 10);
            if (!*argv[i] || *end || c < 1 || c > 65536) { fprintf(stderr, "--channel C: a channel number from 1\n"); return 1; }
            S0.channel = (int)c;
            continue;
        }
        if (!strcmp(argv[i], "--raw-type") && i + 1 < argc) {
            const std::string t = argv[++i];
            if (t != "u8" && t != "u16") { fprintf(stderr, "--raw-type: u8 or u16\n"); return 1; }
            S0.raw_u16 = t == "u16";
            continue;
        }
        if (!strcmp(argv[i], "--window") && i + 1 < argc) {
            long long lo = 0, hi = 0;
            if (!parse_pair(argv[++i], 0, lo, hi) || lo >= hi || hi > 65535) { fprintf(stderr, "--window LO,HI: integers with 0 <= LO < HI <= 65535\n"); return 1; }
            S0.window = pnr_window{(int32_t)lo, (int32_t)hi, 0, 0};
            S0.windowed = window = true;
            continue;
        }
        if (!strcmp(argv[i], "--saturate") && i + 1 < argc) {
            long long lo = 0, hi = 0; // parts per million
            if (!parse_pair(argv[++i], 4, lo, hi) || lo + hi >= 1000000) {
                fprintf(stderr, "--saturate LO,HI: percentages of the voxels clipped to 0 / to 255, up to 4 decimals, LO + HI below 100\n");
                return 1;
            }
            S0.window = pnr_window{-1, -1, (int32_t)lo, (int32_t)hi};
            S0.windowed = saturate = true;
            continue;
        }
        if (!strcmp(argv[i], "--help")) { help = true; continue; }
        if (!strcmp(argv[i], "--swc-info")) {
            if (i + 1 >= argc) { fprintf(stderr, "--swc-info FILE.swc\n"); return 1; }
            swc_info = argv[++i];
            continue;
        }
        if (!strcmp(argv[i], "--distance")) {
            if (i + 2 >= argc) { fprintf(stderr, "--distance A.swc B.swc\n"); return 1; }
            dist_a = argv[++i];
            dist_b = argv[++i];
            distance = true;
            continue;
        }
        if (!strcmp(argv[i], "--distance-step") || !strcmp(argv[i], "--distance-threshold") || !strcmp(argv[i], "--zscale")) {
            const std::string flag = argv[i];
            float v = 0;
            if (!parse_float(i + 1 < argc ? argv[++i] : "", v) || v < 0 || (flag == "--zscale" && !(v > 0))) {
                fprintf(stderr, "%s: a number, %s\n", flag.c_str(), flag == "--zscale" ? "above 0" : "0 or more");
                return 1;
            }
            (flag == "--zscale" ? dist_opts.zscale : flag == "--distance-step" ? dist_opts.step : dist_opts.thr) = v;
            (flag == "--zscale" ? zscale_flag : dist_flag) = true;
            continue;
        }
        if (!strcmp(argv[i], "--join")) {
            float v = 0;
            if (!parse_float(i + 1 < argc ? argv[++i] : "", v) || v < 0) { fprintf(stderr, "--join GAP: the largest bridge in xy voxels, a number, 0 (any distance) or more\n"); return 1; }
            join_given = true;
            join_gap = v;
            continue;
        }
        if (!strcmp(argv[i], "--join-geodesic")) {
            const char *txt = i + 1 < argc ? argv[++i] : "";
            char *end = nullptr;
            errno = 0;
            join_limit = strtoull(txt, &end, 10);
            if (!*txt || *txt == '-' || *end || errno) { fprintf(stderr, "--join-geodesic D: the largest bridge weight, an integer, 0 (no limit) or more\n"); return 1; }
            join_geodesic = true;
            continue;
        }
        if (!strcmp(argv[i], "--join-threshold")) {
            long v = 0;
            if (!parse_thr(i + 1 < argc ? argv[++i] : "", v, S0.join_word)) { fprintf(stderr, "--join-threshold T: an integer from 0 to 255, or -1 for the stack's mean\n"); return 1; }
            join_thr = (int)v;
            join_thr_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--join-root")) {
            const char *txt = i + 1 < argc ? argv[++i] : "";
            long v = 0;
            join_root_soma = !strcmp(txt, "soma");
            if (!join_root_soma && !parse_int(txt, 1, PNR_JOIN_MAX_N, v)) { fprintf(stderr, "--join-root soma|ID: `soma` or a node id from 1\n"); return 1; }
            join_root_id = v;
            join_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--join-keep-largest")) { join_keep_largest = join_flag = true; continue; }
        if (!strcmp(argv[i], "--join-swc")) {
            if (i + 2 >= argc || argv[i + 1][0] == '-' || argv[i + 2][0] == '-') { fprintf(stderr, "--join-swc IN.swc OUT.swc\n"); return 1; }
            join_in = argv[++i];
            join_out = argv[++i];
            continue;
        }
        if (!strcmp(argv[i], "--prune-swc")) {
            if (i + 1 >= argc || argv[i + 1][0] == '-') { fprintf(stderr, "--prune-swc IN.swc [OUT.swc]\n"); return 1; }
            prune_in = argv[++i];
            if (i + 1 < argc && argv[i + 1][0] != '-') prune_out = argv[++i];
            continue;
        }
        if (!strcmp(argv[i], "--prune-length") || !strcmp(argv[i], "--prune-radius") || !strcmp(argv[i], "--prune-min-tree")) {
            const std::string flag = argv[i];
            float v = 0;
            if (!parse_float(i + 1 < argc ? argv[++i] : "", v) || v < 0) {
                fprintf(stderr, "%s\n", flag == "--prune-length" ? "--prune-length L: the shortest side branch kept, in xy voxels, a number, 0 or more"
                                        : flag == "--prune-radius" ? "--prune-radius K: a side branch is kept from K times its parent's radius on, a number, 0 or more"
                                                                   : "--prune-min-tree M: the lowest tree kept, in xy voxels, a number, 0 or more");
                return 1;
            }
            (flag == "--prune-length" ? prune_opts.min_length : flag == "--prune-radius" ? prune_opts.radius_factor : prune_opts.min_tree) = v;
            prune_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--prune")) {
            const std::string txt = i + 1 < argc ? argv[++i] : "";
            std::vector<std::string> part(1);
            for (char ch : txt) {
                if (ch == ',') part.emplace_back();
                else part.back() += ch;
            }
            float v[3] = {0.f, 0.f, 0.f};
            bool ok = part.size() <= 3;
            for (size_t k = 0; ok && k < part.size(); k++) ok = parse_float(part[k].c_str(), v[k]) && v[k] >= 0;
            if (!ok) { fprintf(stderr, "--prune L[,K[,M]]: numbers, 0 or more: the shortest side branch kept, times its parent's radius, the lowest tree kept (xy voxels)\n"); return 1; }
            S0.prune = prune_given = true;
            S0.prune_opts = pnr_prune_opts{1.f, v[0], v[1], v[2]};
            continue;
        }
        if (!strcmp(argv[i], "--per-node")) {
            if (i + 1 >= argc) { fprintf(stderr, "--per-node PREFIX (--distance) or FILE.csv (--render-swc)\n"); return 1; }
            per_node = argv[++i];
            per_node_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--render-swc")) {
            if (i + 1 >= argc || argv[i + 1][0] == '-') { fprintf(stderr, "--render-swc IN.swc\n"); return 1; }
            render.swc = argv[++i];
            continue;
        }
        if (!strcmp(argv[i], "--mask") || !strcmp(argv[i], "--residual")) {
            const bool m = !strcmp(argv[i], "--mask");
            if (i + 1 >= argc || argv[i + 1][0] == '-') { fprintf(stderr, "%s OUT: a .tif or .raw file name\n", argv[i]); return 1; }
            (m ? mask_out : residual_out) = argv[++i];
            continue;
        }
        if (!strcmp(argv[i], "--coverage")) { coverage = true; continue; }
        if (!strcmp(argv[i], "--radius-scale") || !strcmp(argv[i], "--radius-add")) {
            const bool sc = !strcmp(argv[i], "--radius-scale");
            float v = 0;
            if (!parse_float(i + 1 < argc ? argv[++i] : "", v) || (sc && v < 0)) { fprintf(stderr, "%s\n", sc ? "--radius-scale S: a number, 0 or more" : "--radius-add A: a number"); return 1; }
            (sc ? render.opts.rscale : render.opts.radd) = v;
            render_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--coverage-threshold")) {
            long v = 0;
            if (!parse_thr(i + 1 < argc ? argv[++i] : "", v, S0.coverage_word)) { fprintf(stderr, "--coverage-threshold T: an integer from 0 to 255, or -1 for the stack's mean\n"); return 1; }
            render.opts.thr = (int32_t)v;
            render_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--median")) {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m != "2d" && m != "3d") { fprintf(stderr, "--median 2d|3d: a 3 x 3 median in every slice, or a 3 x 3 x 3 one\n"); return 1; }
            S0.filter.median = m == "3d" ? 3 : 2;
            continue;
        }
        if (!strcmp(argv[i], "--subtract-background")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 1, PNR_TOPHAT_MAX_R, v)) { fprintf(stderr, "--subtract-background R: the half-width of the top-hat's box, an integer from 1 to %d\n", PNR_TOPHAT_MAX_R); return 1; }
            S0.filter.tophat_r = (int32_t)v;
            continue;
        }
        if (!strcmp(argv[i], "--fill-holes")) {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m != "2d" && m != "3d") { fprintf(stderr, "--fill-holes 2d|3d: grey-level fill-holes in every slice (4-connected), or in 3-D (6-connected)\n"); return 1; }
            S0.fill_holes = m == "3d" ? 6 : 4;
            continue;
        }
        if (!strcmp(argv[i], "--hmax") || !strcmp(argv[i], "--hdome")) {
            const bool dome = !strcmp(argv[i], "--hdome");
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 1, 255, v)) {
                fprintf(stderr, "%s\n", dome ? "--hdome H: the height kept of what stands above its surroundings, an integer from 1 to 255"
                                             : "--hmax H: the height every grey-level maximum is cut down by, an integer from 1 to 255");
                return 1;
            }
            (dome ? S0.hdome : S0.hmax) = (int)v;
            continue;
        }
        if (!strcmp(argv[i], "--local-threshold")) {
            const std::string txt = i + 1 < argc ? argv[++i] : "";
            std::vector<std::string> part(1);
            for (char ch : txt) {
                if (ch == ',') part.emplace_back();
                else part.back() += ch;
            }
            long r = 0, off = 0, sc = 256;
            if (part.size() > 3 || !parse_int(part[0].c_str(), 1, PNR_LOCAL_MAX_R, r) || (part.size() > 1 && !parse_int(part[1].c_str(), -255, 255, off)) ||
                (part.size() > 2 && !parse_int(part[2].c_str(), 0, 4096, sc))) {
                fprintf(stderr, "--local-threshold R[,OFFSET[,SCALE_256]]: R an integer from 1 to %d, OFFSET -255..255, SCALE_256 0..4096\n", PNR_LOCAL_MAX_R);
                return 1;
            }
            S0.local.r = (int32_t)r, S0.local.offset = (int32_t)off, S0.local.scale_256 = (int32_t)sc;
            continue;
        }
        if (!strcmp(argv[i], "--local-binary")) { S0.local.binary = 1; continue; }
        if (!strcmp(argv[i], "--auto-threshold")) { auto_thr = true; continue; }
        if (!strcmp(argv[i], "--threshold-lo")) {
            long v = 0;
            if (!parse_int(i + 1 < argc ? argv[++i] : "", 0, 255, v)) { fprintf(stderr, "--threshold-lo LO: an integer from 0 to 255\n"); return 1; }
            auto_lo = (int)v;
            auto_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--histogram")) {
            auto_hist = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (auto_hist.empty()) { fprintf(stderr, "--histogram FILE.csv\n"); return 1; }
            auto_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--morph")) { morph = true; continue; }
        if (!strcmp(argv[i], "--morph-out")) {
            morph_out = i + 1 < argc && argv[i + 1][0] != '-' ? argv[++i] : "";
            if (morph_out.empty()) { fprintf(stderr, "--morph-out OUT: a .tif or .raw file name\n"); return 1; }
            continue;
        }
        if (!strcmp(argv[i], "--measure-radius")) { S0.measure_radius = true; continue; }
        if (!strncmp(argv[i], "--radius-", 9)) {
            const std::string flag = argv[i];
            long v = 0;
            const char *txt = i + 1 < argc ? argv[++i] : "";
            if (flag == "--radius-threshold") {
                if (!parse_thr(txt, v, S0.radius_word)) { fprintf(stderr, "--radius-threshold T: an integer from 0 to 255, or -1 for the stack's mean\n"); return 1; }
                S0.radius.thr = (int32_t)v;
                S0.radius.rel_pct = 0;
                radius_abs = true;
            } else if (flag == "--radius-rel") {
                if (!parse_int(txt, 1, 100, v)) { fprintf(stderr, "--radius-rel PCT: an integer from 1 to 100\n"); return 1; }
                S0.radius.rel_pct = (int32_t)v;
                radius_rel = true;
            } else if (flag == "--radius-max") {
                if (!parse_int(txt, 1, PNR_RADIUS_MAX, v)) { fprintf(stderr, "--radius-max K: an integer from 1 to %d\n", PNR_RADIUS_MAX); return 1; }
                S0.radius.rmax = (int32_t)v;
            } else if (flag == "--radius-bg") {
                if (!parse_int(txt, 0, 999, v)) { fprintf(stderr, "--radius-bg PERMILLE: an integer from 0 to 999\n"); return 1; }
                S0.radius.bg_permille = (int32_t)v;
            } else {
                fprintf(stderr, "%s: unknown flag (--radius-threshold, --radius-rel, --radius-max, --radius-bg)\n", flag.c_str());
                return 1;
            }
            radius_flag = true;
            continue;
        }
        if (!strcmp(argv[i], "--ranks") && i + 1 < argc) { ranks = atoi(argv[++i]); continue; }
        if (!strcmp(argv[i], "--share-gpu")) { share_gpu = true; continue; }
        if (!strcmp(argv[i], "--exchange") && i + 1 < argc) { transport = argv[++i]; continue; }
        if (!strcmp(argv[i], "-x") && i + 1 < argc) { i++; continue; } // plugin name: ignored
        if (!strcmp(argv[i], "-f") && i + 1 < argc) { func = argv[++i]; continue; }
        if (!strcmp(argv[i], "-g") && i + 1 < argc) { device = atoi(argv[++i]); continue; }
        if (!strcmp(argv[i], "-v")) { advantra::settings().verbose = true; continue; }
        if (!strcmp(argv[i], "--timing")) { advantra::settings().timing = true; continue; }
        if (!strcmp(argv[i], "--save-midres")) { advantra::settings().save_midres = true; continue; }
        if (!strcmp(argv[i], "--single-tree")) { advantra::settings().single_tree = true; continue; }
        if (!strcmp(argv[i], "--rng-seed") && i + 1 < argc) { advantra::settings().rng_seed = (uint32_t)strtoul(argv[++i], nullptr, 10); continue; }
        if (!strcmp(argv[i], "-d") && i + 1 < argc) { raw_dims = argv[++i]; continue; }
        if (!strcmp(argv[i], "-i")) { while (i + 1 < argc && argv[i + 1][0] != '-') infiles.push_back(argv[++i]); continue; }
        if (!strcmp(argv[i], "-p")) { while (i + 1 < argc) paras.push_back(argv[++i]); continue; }
    }
    if (window && saturate) { fprintf(stderr, "--window and --saturate: one of them\n"); return 1; }
    if (radius_abs && radius_rel) { fprintf(stderr, "--radius-threshold and --radius-rel: one of them\n"); return 1; }
    if (radius_flag && !S0.measure_radius) { fprintf(stderr, "--radius-threshold / --radius-rel / --radius-max / --radius-bg need --measure-radius\n"); return 1; }
    if (help) {
        advantra::print_help();
        advantra::print_flags();
        return 0;
    }
    const bool rendering = !render.swc.empty();
    if ((dist_flag && !distance) || (per_node_flag && !distance && !rendering && !edt && !geo && prune_in.empty()) || (zscale_flag && !distance && join_in.empty() && prune_in.empty() && !rendering && !components && !edt && !geo && !skeleton)) {
        fprintf(stderr, "--distance-step / --distance-threshold / --zscale / --per-node need --distance A.swc B.swc (--zscale: or --join-swc or --skeleton; --zscale, --per-node: or --render-swc, --edt or --geodesic)\n");
        return 1;
    }
    if (render_flag && !rendering) { fprintf(stderr, "--radius-scale / --radius-add / --coverage-threshold need --render-swc IN.swc\n"); return 1; }
    if (join_geodesic && join_given) { fprintf(stderr, "--join GAP and --join-geodesic D: one or the other\n"); return 1; }
    if (join_thr_flag && !join_geodesic) { fprintf(stderr, "--join-threshold needs --join-geodesic D\n"); return 1; }
    if (join_flag && !join_given && !join_geodesic && join_in.empty()) { fprintf(stderr, "--join-root / --join-keep-largest need --join GAP, --join-geodesic D or --join-swc IN.swc OUT.swc\n"); return 1; }
    if (!join_in.empty() && join_root_soma) { fprintf(stderr, "--join-swc: --join-root takes a node id of IN.swc\n"); return 1; }
    if (conn_planar && !ws) { fprintf(stderr, "--connectivity 6|26 (--watershed: 4|8|6|26)\n"); return 1; }
    if (ws_flag && !ws) { fprintf(stderr, "--markers-swc / --markers / --markers-by / --relief / --levels need --watershed -i stack\n"); return 1; }
    if ((comp_flag && !components && !ws) || (thr_flag && !components && !edt && !geo && !skeleton && !ws)) { fprintf(stderr, "--threshold / --connectivity / --min-size / --labels / --per-component need --components -i stack (--threshold: or --edt, --geodesic or --skeleton)\n"); return 1; }
    if (skel_flag && !skeleton) { fprintf(stderr, "--skeleton-rounds / --skeleton-out / --swc need --skeleton -i stack\n"); return 1; }
    if (edt_flag && !edt) { fprintf(stderr, "--edt-max / --edt-out / --at need --edt -i stack\n"); return 1; }
    if (geo_flag && !geo) { fprintf(stderr, "--from / --to / --paths / --geo-max / --geo-out need --geodesic -i stack\n"); return 1; }
    if (S0.hmax && S0.hdome) { fprintf(stderr, "--hmax and --hdome: one of them\n"); return 1; }
    if (!morph_out.empty() && !morph) { fprintf(stderr, "--morph-out needs --morph -i stack\n"); return 1; }
    if (S0.local.binary && !S0.local.r) { fprintf(stderr, "--local-binary needs --local-threshold R\n"); return 1; }
    if (auto_flag && !auto_thr) { fprintf(stderr, "--threshold-lo / --histogram need --auto-threshold -i stack\n"); return 1; }
    if (prune_flag && prune_in.empty()) { fprintf(stderr, "--prune-length / --prune-radius / --prune-min-tree need --prune-swc IN.swc [OUT.swc]\n"); return 1; }
    if (prune_given && !prune_in.empty()) { fprintf(stderr, "--prune L[,K[,M]] and --prune-swc: one or the other (--prune-swc takes --prune-length, --prune-radius, --prune-min-tree)\n"); return 1; }
    if (prune_given && (geo || edt || components || rendering || distance || !join_in.empty() || info || morph || ws || auto_thr || !swc_info.empty() || (skeleton && skel_job.swc.empty()))) {
        fprintf(stderr, "--prune L[,K[,M]] needs a tracing run or --skeleton --swc OUT.swc\n");
        return 1;
    }
    if (!prune_in.empty()) {
        if (skeleton || skel_flag || geo || geo_flag || edt || edt_flag || components || comp_flag || thr_flag || rendering || distance || !join_in.empty() || info || S0.despeckle ||
            S0.measure_radius || join_given || join_geodesic || join_flag || !paras.empty() || morph || ws || ws_flag || auto_thr || !swc_info.empty()) {
            fprintf(stderr, "--prune-swc: not with a tracing run (-p), another tool mode, --threshold, --despeckle, --measure-radius or --join\n");
            return 1;
        }
        prune_opts.zscale = dist_opts.zscale;
        return advantra::prune_swc_file(prune_in, prune_out, prune_opts, per_node, device) ? 0 : 1;
    }
    if (!swc_info.empty()) return advantra::print_swc_info(swc_info) ? 0 : 1;
    if (auto_thr) {
        if (skeleton || skel_flag || geo || geo_flag || edt || edt_flag || components || comp_flag || thr_flag || rendering || distance || !join_in.empty() || info || S0.despeckle ||
            S0.measure_radius || join_given || join_geodesic || per_node_flag || zscale_flag || !paras.empty() || morph || ws || ws_flag) {
            fprintf(stderr, "--auto-threshold: not with a tracing run (-p), another tool mode, --threshold, --despeckle, --measure-radius, --join, --per-node or --zscale\n");
            return 1;
        }
        if (infiles.empty()) { fprintf(stderr, "--auto-threshold needs -i <stack>\n"); return 1; }
        return advantra::auto_threshold_file(auto_lo, auto_hist, infiles, raw_dims, device) ? 0 : 1;
    }
    if (skeleton) {
        if (geo || geo_flag || edt || edt_flag || components || comp_flag || rendering || distance || !join_in.empty() || info || S0.despeckle || S0.measure_radius || join_given || join_geodesic ||
            per_node_flag || !paras.empty() || morph || ws || ws_flag) {
            fprintf(stderr, "--skeleton: not with a tracing run (-p), --geodesic, --edt, --components, --render-swc, --distance, --join-swc, --join, --info, --despeckle, --measure-radius, --per-node, --morph or --watershed\n");
            return 1;
        }
        if (infiles.empty()) { fprintf(stderr, "--skeleton needs -i <stack>\n"); return 1; }
        if (zscale_flag && dist_opts.zscale < 1.f) { fprintf(stderr, "--skeleton: --zscale Z: a number, 1 or more\n"); return 1; }
        skel_job.prune = prune_given, skel_job.prune_opts = S0.prune_opts;
        return advantra::skeleton_file(skel_job, infiles, raw_dims, zscale_flag ? dist_opts.zscale : 1.f, device) ? 0 : 1;
    }
    if (morph) {
        if (geo || geo_flag || edt || edt_flag || components || comp_flag || rendering || distance || !join_in.empty() || info || S0.despeckle || S0.measure_radius || join_given || join_geodesic ||
            per_node_flag || thr_flag || zscale_flag || !paras.empty() || ws || ws_flag) {
            fprintf(stderr, "--morph: not with a tracing run (-p), --skeleton, --geodesic, --edt, --components, --render-swc, --distance, --join-swc, --join, --info, --despeckle, --measure-radius, --per-node, --threshold, --zscale or --watershed\n");
            return 1;
        }
        if (infiles.empty()) { fprintf(stderr, "--morph needs -i <stack>\n"); return 1; }
        if (morph_out.empty()) { fprintf(stderr, "--morph needs --morph-out OUT\n"); return 1; }
        if (!S0.morph()) { fprintf(stderr, "--morph needs one of --fill-holes, --hmax and --hdome\n"); return 1; }
        return advantra::morph_file(morph_out, infiles, raw_dims, device) ? 0 : 1;
    }
    if (ws) {
        if (geo || geo_flag || edt || edt_flag || components || comp_only_flag || rendering || distance || !join_in.empty() || info || S0.despeckle ||
            S0.measure_radius || join_given || join_geodesic || per_node_flag || zscale_flag || !paras.empty()) {
            fprintf(stderr, "--watershed: not with a tracing run (-p), --skeleton, --morph, --geodesic, --edt, --components, --min-size, --per-component, --render-swc, --distance, --join-swc, --join, --info, --despeckle, --measure-radius, --per-node or --zscale\n");
            return 1;
        }
        if (infiles.empty()) { fprintf(stderr, "--watershed needs -i <stack>\n"); return 1; }
        if (!ws_job.markers_swc.empty() && !ws_job.markers_raw.empty()) { fprintf(stderr, "--markers-swc and --markers: one of them\n"); return 1; }
        if (ws_job.markers_swc.empty() && ws_job.markers_raw.empty()) { fprintf(stderr, "--watershed needs one of --markers-swc and --markers\n"); return 1; }
        if (ws_by_flag && ws_job.markers_swc.empty()) { fprintf(stderr, "--markers-by needs --markers-swc\n"); return 1; }
        if (comp.labels.empty()) { fprintf(stderr, "--watershed needs --labels OUT.raw\n"); return 1; }
        ws_job.labels = comp.labels;
        return advantra::watershed_file(ws_job, infiles, raw_dims, device) ? 0 : 1;
    }
    if (geo) {
        if (edt || edt_flag || components || comp_flag || rendering || distance || !join_in.empty() || info || S0.despeckle || S0.measure_radius || join_given || join_geodesic || !paras.empty()) {
            fprintf(stderr, "--geodesic: not with a tracing run (-p), --edt, --components, --render-swc, --distance, --join-swc, --join, --info, --despeckle or --measure-radius\n");
            return 1;
        }
        if (infiles.empty()) { fprintf(stderr, "--geodesic needs -i <stack>\n"); return 1; }
        if (geo_job.from.empty()) { fprintf(stderr, "--geodesic needs --from tree.swc\n"); return 1; }
        if (geo_job.to.empty() != per_node.empty()) { fprintf(stderr, "--geodesic: --to other.swc and --per-node FILE.csv go together\n"); return 1; }
        if (!geo_job.paths.empty() && geo_job.to.empty()) { fprintf(stderr, "--geodesic: --paths OUT.swc needs --to other.swc\n"); return 1; }
        if (zscale_flag && dist_opts.zscale < 1.f) { fprintf(stderr, "--geodesic: --zscale Z: a number, 1 or more\n"); return 1; }
        geo_job.per_node = per_node;
        return advantra::geodesic_file(geo_job, infiles, raw_dims, zscale_flag ? dist_opts.zscale : 1.f, device) ? 0 : 1;
    }
    if (edt) {
        if (components || comp_flag || rendering || distance || !join_in.empty() || info || S0.despeckle || S0.measure_radius || join_given || join_geodesic || !paras.empty()) {
            fprintf(stderr, "--edt: not with a tracing run (-p), --components, --render-swc, --distance, --join-swc, --join, --info, --despeckle or --measure-radius\n");
            return 1;
        }
        if (infiles.empty()) { fprintf(stderr, "--edt needs -i <stack>\n"); return 1; }
        if (edt_job.at.empty() != per_node.empty()) { fprintf(stderr, "--edt: --at tree.swc and --per-node FILE.csv go together\n"); return 1; }
        if (zscale_flag && dist_opts.zscale < 1.f) { fprintf(stderr, "--edt: --zscale Z: a number, 1 or more\n"); return 1; }
        edt_job.per_node = per_node;
        return advantra::edt_file(edt_job, infiles, raw_dims, zscale_flag ? dist_opts.zscale : 1.f, device) ? 0 : 1;
    }
    if (components) {
        if (rendering || distance || !join_in.empty() || info || S0.despeckle) { fprintf(stderr, "--components: not with --render-swc, --distance, --join-swc, --info or --despeckle (--min-size drops the small components)\n"); return 1; }
        if (infiles.empty()) { fprintf(stderr, "--components needs -i <stack>\n"); return 1; }
        return advantra::components_file(comp, infiles, raw_dims, zscale_flag ? dist_opts.zscale : 0.f, device) ? 0 : 1;
    }
    if (S0.despeckle && (rendering || distance || !join_in.empty() || info)) { fprintf(stderr, "--despeckle needs a tracing run\n"); return 1; }
    if (rendering) {
        if (distance || !join_in.empty() || coverage) { fprintf(stderr, "--render-swc: not with --distance, --join-swc or --coverage (the JSON line has the coverage)\n"); return 1; }
        if (infiles.empty() && (mask_out.empty() || !residual_out.empty() || !per_node.empty() || render.opts.thr != -1 || S0.coverage_word.given)) {
            fprintf(stderr, "--render-swc without -i: -d w,h,l gives the grid and only --mask OUT is allowed (and needed)\n");
            return 1;
        }
        render.mask = mask_out, render.residual = residual_out, render.per_node = per_node, render.opts.zscale = dist_opts.zscale;
        return advantra::render_swc_file(render, infiles, raw_dims, device) ? 0 : 1;
    }
    if ((!mask_out.empty() || !residual_out.empty() || coverage) && (distance || !join_in.empty() || info)) { fprintf(stderr, "--mask / --residual / --coverage need a tracing run or --render-swc IN.swc\n"); return 1; }
    S0.mask_out = mask_out, S0.residual_out = residual_out, S0.coverage = coverage;
    if (!join_in.empty() && join_geodesic) {
        if (infiles.empty()) { fprintf(stderr, "--join-swc --join-geodesic needs -i <stack>\n"); return 1; }
        if (zscale_flag && dist_opts.zscale < 1.f) { fprintf(stderr, "--join-geodesic: --zscale Z: a number, 1 or more\n"); return 1; }
        const pnr_geojoin_opts go = {join_thr, join_limit, 1.f, nullptr};
        return advantra::join_swc_geodesic_file(join_in, join_out, go, infiles, raw_dims, zscale_flag ? dist_opts.zscale : 1.f, join_root_id, join_keep_largest, device) ? 0 : 1;
    }
    if (!join_in.empty()) return advantra::join_swc_file(join_in, join_out, join_gap, dist_opts.zscale, join_root_id, join_keep_largest, device) ? 0 : 1;
    if (join_given) S0.join = true, S0.join_gap = join_gap, S0.join_root_id = join_root_id, S0.join_keep_largest = join_keep_largest;
    if (join_geodesic) S0.join = S0.join_geodesic = true, S0.join_limit = join_limit, S0.join_thr = join_thr, S0.join_root_id = join_root_id, S0.join_keep_largest = join_keep_largest;
    if (distance) return advantra::print_tree_distance(dist_a, dist_b, dist_opts, device, per_node) ? 0 : 1;
    if (info) {
        if (infiles.empty()) { fprintf(stderr, "--info needs -i <inimg_file>\n"); return 1; }
        return advantra::print_info(infiles[0], raw_dims, S0.channel - 1, S0.raw_u16) ? 0 : 1;
    }
    if (func == "help") { // funclist(): advantra_func, help (Advantra_plugin.cpp:157-162)
        advantra::print_help();
        return 0;
    }
    if (func != "advantra_func") return 1; // dofunc: unknown function -> false
    if (transport != "shm" && transport != "rccl") { fprintf(stderr, "--exchange: shm or rccl\n"); return 1; }
    const bool rccl = transport == "rccl";
    if (rccl && share_gpu && ranks > 1) { fprintf(stderr, "--exchange rccl needs one GPU per rank (RCCL refuses two ranks on one device)\n"); return 1; }
    // (--ranks 1 --exchange rccl: the sharded code path with its RCCL collectives on a world of one -- what a one-GPU box can rehearse)
    if (ranks <= 1 && !rccl) return advantra::advantra_func(infiles, paras, device, raw_dims) ? 0 : 1;
    if (ranks < 1) ranks = 1;
    if (ranks > 64) { fprintf(stderr, "--ranks: at most 64\n"); return 1; }
    // one process per GPU, forked here -- nothing has touched a GPU yet -- and joined through a shared-memory segment
    // unique to this job, not only to this pid (a recycled pid must never meet the segment of a crashed earlier job)
    struct timespec now;
    clock_gettime(CLOCK_REALTIME, &now);
    const std::string name = "pnr_cli_" + std::to_string((long long)getpid()) + "_" + std::to_string((long long)now.tv_sec) + "_" + std::to_string((long long)now.tv_nsec);
    std::vector<pid_t> kids;
    for (int r = 0; r < ranks; r++) {
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); return 1; }
        if (pid == 0) {
            advantra::Settings &S = advantra::settings();
            S.rank = r; S.world = ranks;
            if (pnr_shm_exchange_open(name.c_str(), r, ranks, 1 << 18, &S.exchange) != PNR_OK) {
                fprintf(stderr, "rank %d: %s\n", r, pnr_last_error());
                _exit(1);
            }
            const int dev = share_gpu ? device : device + r;
            if (rccl) { // the ncclUniqueId of rank 0 reaches the others through the shared-memory segment; then every rank joins with its GPU
                unsigned char id[128] = {0};
                std::vector<unsigned char> all((size_t)128 * ranks);
                int okid = (r != 0 || pnr_rccl_unique_id(id) == PNR_OK) ? 1 : 0;
                if (!okid) fprintf(stderr, "rank 0: %s\n", pnr_last_error());
                if (pnr_shm_allgather(S.exchange, id, all.data(), 128) != PNR_OK) { fprintf(stderr, "rank %d: %s\n", r, pnr_last_error()); _exit(1); }
                bool zero = true; // (rank 0 failed to make an id: everybody leaves)
                for (int b = 0; b < 128; b++) zero = zero && all[(size_t)b] == 0;
                if (zero || pnr_rccl_exchange_open(all.data(), r, ranks, dev, 1 << 18, &S.rccl) != PNR_OK) {
                    if (!zero) fprintf(stderr, "rank %d: %s\n", r, pnr_last_error());
                    _exit(1);
                }
                S.force_shard = true;
            }
            const bool okr = advantra::advantra_func(infiles, paras, dev, raw_dims);
            pnr_rccl_exchange_close(S.rccl);
            pnr_shm_exchange_close(S.exchange);
            fflush(stdout); fflush(stderr);
            _exit(okr ? 0 : 1);
        }
        kids.push_back(pid);
    }
    int worst = 0;
    for (pid_t k : kids) {
        int st = 0;
        if (waitpid(k, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) worst = 1;
    }
    return worst;
}
