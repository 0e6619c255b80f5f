// advantra_host.cpp -- see advantra_host.h.  Host orchestration only: every compute stage is a call
// through the C ABI into libpnr_hip.so.  Here: the settings, the help, the parameters, the SWC comment block and the tracing run;
// stack_reader.cpp reads stacks, swc_io.cpp reads and writes SWC files, tools.cpp has the tool modes.
#include "host_internal.h"
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <sstream>

namespace advantra {

static const int nrInputParams = 11; // Advantra_plugin.cpp:60

Settings &settings()
{
    static Settings s;
    return s;
}

void print_help()
{
    // wording of the reference's print_help (Advantra_plugin.cpp:125-148), shortened to the call contract
    printf("**** usage of Advantra tracing ****\n");
    printf("vaa3d -x Advantra -f advantra_func -i <inimg_file> -p <neuritesigmas> <somaradius> <tolerance> <znccth> <kappa> "
           "<step> <ni> <np> <zdist> <nodepervol> <vol>\n");
    printf("inimg_file     The input image (8- or 16-bit multi-page TIFF; 16-bit stacks are windowed to 8 bits)\n");
    printf("neuritesigmas  Comma delimited list of gaussian cross-section sigmas, e.g. 2,4,6\n");
    printf("somaradius     Soma radius (0: no soma)\n");
    printf("tolerance      Seed extraction (find maxima) tolerance\n");
    printf("znccth         Correlation threshold [0,1]\n");
    printf("kappa          Von Mises kappa [0,5]\n");
    printf("step           Prediction step\n");
    printf("ni             Number of iterations\n");
    printf("np             Number of particles\n");
    printf("zdist          Distance between layers in pixels\n");
    printf("nodepervol     Node density limit (2,20]\n");
    printf("vol            Volume pattern: 1,5,9,11,19,27\n");
    printf("outswc_file    <inimg_file>_Advantra.swc\n");
}

void print_flags()
{
    printf("\nadvantra_cli [flags] -f advantra_func -i <inimg_file> -p <the 11 parameters>   (flags go before -p)\n");
    printf("-v | --timing | --save-midres | --single-tree | --rng-seed N | -g DEVICE | -d w,h,l (.raw) | --info\n");
    printf("--ranks N [--share-gpu] [--exchange shm|rccl]   one stack on N GPUs of this host\n");
    printf("--swc-info FILE.swc       one JSON line about an SWC file: nodes, roots, segments, total length, bounding box (no GPU)\n");
    printf("--distance A.swc B.swc    the tree distance of two SWC files on the GPU (SD, SSD, %%SSD per direction and combined) as one JSON line\n");
    printf("  --distance-step S         resampling step of both trees (default 1; 0: the nodes only)\n");
    printf("  --distance-threshold T    a point counts as far away from T on (default 2)\n");
    printf("  --zscale Z                z is multiplied by Z first (default 1; the stack's zdist gives distances in xy voxels)\n");
    printf("  --per-node PREFIX         also write PREFIX_ab.csv / PREFIX_ba.csv: `id,d` of every sample point of A / of B\n");
    printf("--join GAP                join the traced forest into one tree on the GPU: fragments whose closest nodes lie within GAP xy voxels\n");
    printf("                          (0: any distance) are bridged, the tree is re-rooted and written with every parent before its children\n");
    printf("  --join-root soma|ID       the root: the first soma node if there is one (default), or the node with this id in the file without --join\n");
    printf("  --join-keep-largest       write only the largest component (the root's, if a root is given)\n");
    printf("--join-swc IN.swc OUT.swc the same on an SWC file ([--join GAP] [--zscale Z] [--join-root ID] [--join-keep-largest]); one JSON line\n");
    printf("--join-geodesic D         in the place of --join GAP: join the traced forest along the signal on the GPU -- the minimum spanning forest of the\n");
    printf("                          fragments under gray-weighted path cost; no bridge that weighs more than D is made (0: no limit; 64 is one xy voxel\n");
    printf("                          at cost 1); the bridges' voxels become nodes ([--join-threshold T] [--join-root soma|ID] [--join-keep-largest])\n");
    printf("  --join-threshold T        voxels below T are impassable, 0..255, -1: the stack's mean (default 0: every voxel is passable)\n");
    printf("--join-swc IN.swc OUT.swc --join-geodesic D -i stack   the same on an SWC file and a stack (the volume setup of --geodesic; [--zscale Z]\n");
    printf("                          [--join-threshold T] [--join-root ID] [--join-keep-largest]); one JSON line with the summary\n");
    printf("--prune L[,K[,M]]         while tracing (after --join / --join-geodesic, before --measure-radius), and with --skeleton --swc: side branches shorter than\n");
    printf("                          max(L, K x the radius of the node they leave) and trees lower than M, in xy voxels, are removed on the GPU in one pass (a\n");
    printf("                          branch = what hangs on a node beside its longest continuation); the comment block gains\n");
    printf("                          #prune=length:L,radius:K,min_tree:M,removed:N,segments:S\n");
    printf("--prune-swc IN.swc [OUT.swc]   the same on an SWC file: OUT.swc has the kept nodes in the input's order with ids 1..m; one JSON line with the counts,\n");
    printf("                          lengths in xy voxels; without a threshold it is the morphometry of the file\n");
    printf("  --prune-length L | --prune-radius K | --prune-min-tree M   the three thresholds, numbers, 0 or more (default 0: off)\n");
    printf("  --zscale Z                z counts Z-fold (default 1)\n");
    printf("  --per-node FILE.csv       `id,keep,height,path,order,seg_id` per input node: its longest way down, its way from the root (xy voxels), its\n");
    printf("                            branch order and the first node of its segment\n");
    printf("--render-swc IN.swc       render an SWC file into the stack given with -i (the same volume setup as tracing) on the GPU; one JSON line with\n");
    printf("                          the coverage counts: how much of the foreground the tree covers, how much of the tree lies on signal\n");
    printf("  --mask OUT                write the mask (255 under the tree) as a multi-page 8-bit TIFF, or bare bytes for a .raw name\n");
    printf("  --residual OUT            write the stack with the tree's voxels set to 0: the signal the trace does not explain\n");
    printf("  --per-node FILE.csv       `id,vox,fg,sum` per node: its voxels, the foreground among them, their summed intensity\n");
    printf("  --zscale Z | --radius-scale S | --radius-add A   z and the radii as rendered: z * Z, max(radius * S + A, 0)\n");
    printf("  --coverage-threshold T    foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("                          without -i: -d w,h,l gives the grid and only --mask is allowed\n");
    printf("--mask OUT | --residual OUT | --coverage   while tracing: the final tree rendered on the traced stack (zscale = zdist); the comment block\n");
    printf("                          gains #coverage=thr:T,covered:..,on_signal:..,intensity:..,tree_voxels:N\n");
    printf("--channel C | --raw-type u8|u16 | --window LO,HI | --saturate LO,HI   the input; 16-bit stacks are windowed to 8 bits\n");
    printf("--median 2d|3d            pre-filter: 3 x 3 median in every slice, or 3 x 3 x 3 (on the GPU, before tracing; default: off)\n");
    printf("--subtract-background R   pre-filter: top-hat with a flat box of half-width R in xy and R / zdist in z, 1..%d (after the median)\n", PNR_TOPHAT_MAX_R);
    printf("--fill-holes 2d|3d        pre-filter: grey-level fill-holes on the GPU (after the median and the top-hat): every dark region that the brighter\n");
    printf("                          voxels around it cut off from the stack's border is raised to their level -- in every slice (2d, 4-connected) or in 3-D\n");
    printf("                          (3d, 6-connected); a hollow soma is closed before it is thinned or measured\n");
    printf("--hmax H | --hdome H      pre-filter (after --fill-holes): h-maxima -- every grey-level maximum is cut down by H, 1..255, so maxima standing less\n");
    printf("                          than H above their surroundings vanish --, or h-domes: what that removes, the structure standing above its surroundings\n");
    printf("--morph -i stack          the stack after the volume set-up of tracing with [--fill-holes 2d|3d] [--hmax H | --hdome H] as one JSON line: per stage\n");
    printf("                          op, h, n_vox, n_changed, n_nonzero, sum_in, sum_out, max_delta, connectivity, tiles, tile_visits, rounds\n");
    printf("  --morph-out OUT           write the resulting stack as a multi-page 8-bit TIFF, or bare bytes for a .raw name (needed)\n");
    printf("--watershed -i stack      the marker-controlled watershed of the stack (after the volume set-up of tracing) on the GPU: every voxel from --threshold T\n");
    printf("                          on (default -1: the stack's mean) gets the label of the marker whose flood over the relief reaches it first; the borders\n");
    printf("                          lie on the lowest passes.  One JSON line: w, h, l, markers_by, n_markers, then the fields of pnr_watershed_info\n");
    printf("  --markers-swc FILE.swc    the markers are the nodes of the tree file ...\n");
    printf("  --markers-by tree|node    ... each labelled with the number of its tree, 1.. by descending node count (default: the voxels per neuron), or with its id\n");
    printf("  --markers FILE.raw        ... or a marker volume: little-endian int32, > 0 = a label, 0 = none\n");
    printf("  --relief FILE.raw         the relief to flood as bare bytes (default: 255 - the stack, bright signal floods first)\n");
    printf("  --connectivity 4|8|6|26   the neighbourhood (default 26; 4 and 8: every slice on its own)\n");
    printf("  --labels OUT.raw          write the label volume: little-endian int32, 0 = not reached or below the threshold (needed)\n");
    printf("  --levels OUT.raw          write the pass height at which each voxel joined its region, as bare bytes\n");
    printf("--local-threshold R[,OFFSET[,SCALE_256]]   pre-filter (after --fill-holes / --hmax / --hdome, before --despeckle): a voxel is kept where it is at least\n");
    printf("                          SCALE_256 / 256 times the mean of the box of half-width R in xy and R / zdist in z around it, plus OFFSET; the others are set\n");
    printf("                          to 0 (R 1..%d, OFFSET -255..255, default 0, SCALE_256 0..4096, default 256); the comment block gains #local=r:R,offset:C,scale:K,kept:N\n", PNR_LOCAL_MAX_R);
    printf("  --local-binary            kept voxels become 255\n");
    printf("--auto-threshold -i stack every threshold rule on the stack (after the volume set-up of tracing) from one histogram pass on the GPU, as one JSON line:\n");
    printf("                          w, h, l, n_vox, lo, and thr and n_fg (the voxels from thr on) of mean, otsu, triangle, maxentropy and top1 (the brightest 1 %%)\n");
    printf("  --threshold-lo LO         only the values from LO on are counted, 0..255 (default 0; 1 ignores the zeros a top-hat leaves)\n");
    printf("  --histogram FILE.csv      write the 256 counts as `v,count`\n");
    printf("threshold words           --threshold, --coverage-threshold, --radius-threshold, --join-threshold and the THR of --despeckle also take, in the place of\n");
    printf("                          T or -1, mean|otsu|triangle|maxentropy|topP, each with an optional :LO (topP: the brightest P per cent; LO as --threshold-lo);\n");
    printf("                          the tool's JSON line or SWC comment then names the word as thr_method\n");
    printf("--despeckle MIN[,THR[,CONN]]  pre-filter: foreground components (voxels >= THR, default -1: the stack's mean; CONN 6 or 26, default 26) of\n");
    printf("                          fewer than MIN voxels are set to 0 on the GPU (after the median and the top-hat, before tracing)\n");
    printf("--components -i stack     the connected components of the stack's foreground on the GPU (the same volume setup as tracing) as one JSON\n");
    printf("                          line: n_vox, n_fg, n_comp, n_small, vox_small, largest, thr_used; on a --residual file: what the trace missed\n");
    printf("  --threshold T             foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("  --connectivity 6|26       face neighbours only, or faces, edges and corners (default 26)\n");
    printf("  --min-size M              components of fewer than M voxels are not counted, numbered or listed (default 1)\n");
    printf("  --labels OUT.raw          write the label volume: little-endian int32, 0 = background, 1.. by first voxel in raster order\n");
    printf("  --per-component FILE.csv  `id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax` per component\n");
    printf("--edt -i stack            the exact Euclidean distance transform of the stack's foreground on the GPU (the same volume setup as tracing):\n");
    printf("                          every voxel's distance d to the nearest background voxel, in xy voxels; one JSON line: n_vox, n_fg, n_capped,\n");
    printf("                          thr_used, rmax, zdist, d_max, max_at (the thickest point: where a soma is, and how large somaradius has to be)\n");
    printf("  --threshold T             foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("  --edt-max R               distances are capped at R xy voxels, 1..%d (default 64)\n", PNR_EDT_MAX_R);
    printf("  --zscale Z                z counts Z-fold, 1 or more (default 1)\n");
    printf("  --edt-out OUT.raw         write d of every voxel: little-endian float32\n");
    printf("  --at tree.swc --per-node FILE.csv   `id,d` per node of the SWC file: its sub-voxel radius (-1: a position that is not finite)\n");
    printf("--geodesic -i stack --from tree.swc   the gray-weighted geodesic distance of every voxel to the tree on the GPU (the same volume setup as\n");
    printf("                          tracing): the cheapest 26-connected path, a step costs its length times the darkness 256 - v of its two voxels;\n");
    printf("                          one JSON line: n_vox, n_pass, n_reached, n_src, n_src_dropped, thr_used, dmax, zdist, d_max, len_max, max_at, rounds\n");
    printf("  --threshold T             voxels below T are impassable, 0..255, -1: the stack's mean (default 0: every voxel is passable)\n");
    printf("  --geo-max D               no path that costs more than D is kept, 1..2147483647 (default: no limit; 64 is one xy voxel at cost 1)\n");
    printf("  --zscale Z                z counts Z-fold, 1 or more (default 1)\n");
    printf("  --to other.swc --per-node FILE.csv   `id,d,label` per node of the SWC file: its cost and the id of the tree node it attaches to\n");
    printf("  --paths OUT.swc           with --to: every complete path as a chain of SWC nodes that ends on the tree (paths of more than\n");
    printf("                            min(%d, 2^26 / nodes) voxels are left out and counted on stderr)\n", PNR_GEO_MAX_PATH);
    printf("  --geo-out PREFIX          write PREFIX_d.raw (little-endian uint32, 4294967295: unreached) and PREFIX_label.raw (int32, -1: unreached)\n");
    printf("--skeleton -i stack       the stack's foreground thinned to a one-voxel-wide curve skeleton on the GPU (the same volume setup as tracing;\n");
    printf("                          topology-preserving: simple points that are no end points go, subfield by subfield); one JSON line: n_vox, n_fg,\n");
    printf("                          n_skel, n_end, n_branch, n_isolated, tiles, tile_visits, rounds, thr_used, trees\n");
    printf("  --threshold T             foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("  --skeleton-rounds R       at most R thinning rounds (default 0: until nothing is deleted)\n");
    printf("  --zscale Z                z counts Z-fold in the radii of --swc, 1 or more (default 1)\n");
    printf("  --skeleton-out OUT        write the skeleton (255) as a multi-page 8-bit TIFF, or bare bytes for a .raw name\n");
    printf("  --swc OUT.swc             write the skeleton as a tree rooted at its thickest voxel: radius = the distance to the background, type 2,\n");
    printf("                            every parent before its children; the comment block ends in #skeleton=thr:T,rounds:R,voxels:K,trees:C\n");
    printf("--measure-radius          SWC radii measured from the image at the final nodes (default: SIG2RADIUS * the winning scale)\n");
    printf("--radius-rel PCT          relative mode (default, 50): background below PCT %% of the node's brightest centre voxel, 1..100\n");
    printf("--radius-threshold T      absolute mode: background below T, 0..255; -1: below the stack's mean\n");
    printf("--radius-max K            largest radius looked for, in xy voxels, 1..%d (default 32)\n", PNR_RADIUS_MAX);
    printf("--radius-bg PERMILLE      background voxels a ball may hold, per thousand, 0..999 (default 1)\n");
}

std::vector<float> measured_radius_column(const std::vector<pnr_node> &tree, const std::vector<int32_t> &k)
{
    std::vector<float> r(tree.size(), -1.f);
    for (size_t i = 1; i < tree.size() && i < k.size(); i++)
        if (k[i] >= 0 && tree[i].type != 1) r[i] = k[i] >= 1 ? (float)k[i] : 0.5f;
    return r;
}

int parse_params(const std::vector<std::string> &paras, pnr_params &p, std::string &err)
{
    if ((int)paras.size() != nrInputParams) { // Advantra_plugin.cpp:295-299
        err = "Needs 11 input parameters.";
        return -1;
    }
    pnr_default_params(&p);
    { // parse_csv_string (:1885-1897): comma separated floats, sorted ascending
        std::vector<float> sig;
        std::stringstream ss(paras[0]);
        float v;
        while (ss >> v) {
            sig.push_back(v);
            if (ss.peek() == ',') ss.ignore();
        }
        std::sort(sig.begin(), sig.end());
        if (sig.empty() || sig.size() > PNR_MAX_SIGMAS) { err = "neuritesigmas out of range"; return -2; }
        p.nsig = (int)sig.size();
        for (int i = 0; i < p.nsig; i++) p.sig[i] = sig[i];
    }
    p.somaradius = atoi(paras[1].c_str());
    p.tolerance = (float)atof(paras[2].c_str());
    p.znccth = (float)atof(paras[3].c_str());
    p.kappa = (float)atof(paras[4].c_str());
    p.step = atoi(paras[5].c_str());
    p.ni = atoi(paras[6].c_str());
    p.np = atoi(paras[7].c_str());
    p.zdist = (float)atof(paras[8].c_str());
    p.nodepervol = atoi(paras[9].c_str());
    p.vol = atoi(paras[10].c_str());
    // range checks and messages of Advantra_plugin.cpp:317-326
    if (p.somaradius < 0) { err = "somaradius out of range"; return -2; }
    if (p.tolerance < 0) { err = "tolerance out of range"; return -2; }
    if (p.znccth < 0 || p.znccth > 1) { err = "znccth out of range"; return -2; }
    if (p.kappa < 0 || p.kappa > 5) { err = "kappa out of range"; return -2; }
    if (p.step < 1) { err = "step out of range"; return -2; }
    if (p.ni <= 0) { err = "ni out of range"; return -2; }
    if (p.np <= 0) { err = "np out of range"; return -2; }
    if (p.zdist < 1) { err = "zdist out of range"; return -2; }
    if (p.nodepervol <= 2 || p.nodepervol > 20) { err = "nodepervol out of range"; return -2; }
    if (!(p.vol == 1 || p.vol == 5 || p.vol == 9 || p.vol == 11 || p.vol == 19 || p.vol == 27)) { err = "vol can be 1,5,9,11,19,27"; return -2; }
    return 0;
}

// window: the (lo, hi) a 16-bit stack was windowed with (nullptr: 8-bit input); radius_thr: the threshold the radii were measured
// with (nullptr: not measured; 0: the relative mode)
// join: the result of a --join run (nullptr: not joined); cover: the result of a --mask / --residual / --coverage run (nullptr: none)
static std::string swc_comment(const std::vector<std::string> &paras, const pnr_params &p, const int32_t *window, const int32_t *radius_thr = nullptr,
                               const Result *join = nullptr, const Result *cover = nullptr)
{
    static const char *keys[] = {"neuritesigmas", "somaradius", "tolerance", "znccth", "kappa", "step", "ni", "np", "zdist", "nodepervol", "vol"};
    std::stringstream c;
    c << "email: miro@braincadet.com\n#params:\n#channel=" << settings().channel; // Advantra_plugin.cpp:2276-2306
    for (int i = 0; i < nrInputParams; i++) c << "\n#" << keys[i] << "=" << paras[i];
    c << "\n#------------------------\n#Kc=" << p.Kc << "\n#neff_ratio=" << p.neff_ratio << "\n#frangi_alfa=" << p.alpha
      << "\n#frangi_beta=" << p.beta << "\n#frangi_C=" << p.C << "\n#MAX_TRACE_COUNT=" << p.max_trace_count
      << "\n#EPSILON2=0.0001\n#REFINE_ITER=4\n#SIG2RADIUS=1.5\n#TRACE_RSMPL=1\n#GROUP_RADIUS=2\n#ENFORCE_SINGLE_TREE=0\n#TREE_SIZE_MIN=10\n#TAIL_SIZE_MIN=2";
    if (window) c << "\n#bits=16\n#window=" << window[0] << "," << window[1];
    const pnr_filter_opts &fo = settings().filter;
    if (fo.median || fo.tophat_r) {
        c << "\n#filter=median:" << (fo.median == 3 ? "3d" : fo.median == 2 ? "2d" : "off") << ",tophat:";
        if (fo.tophat_r) c << fo.tophat_r;
        else c << "off";
    }
    if (settings().morph()) {
        const Settings &s = settings();
        auto level = [&](int v) { return v ? std::to_string(v) : std::string("off"); };
        c << "\n#morph=fill:" << (s.fill_holes == 6 ? "3d" : s.fill_holes == 4 ? "2d" : "off") << ",hmax:" << level(s.hmax) << ",hdome:" << level(s.hdome);
    }
    if (settings().local.r && cover)
        c << "\n#local=r:" << settings().local.r << ",offset:" << settings().local.offset << ",scale:" << settings().local.scale_256 << ",kept:" << cover->local_kept;
    if (settings().despeckle && cover)
        c << "\n#despeckle=min:" << settings().despeckle_opts.min_size << ",thr:" << cover->despeckle_thr << ",conn:" << settings().despeckle_opts.connectivity
          << ",removed:" << cover->despeckle_removed << ",voxels:" << cover->despeckle_voxels << thr_method_swc(settings().despeckle_word);
    if (join && settings().join_geodesic)
        c << "\n#join=geodesic:" << settings().join_limit << ",thr:" << join->join_thr_used << ",bridges:" << join->join_bridges << ",trees:" << join->join_trees_in << "->"
          << join->join_trees_out << ",inserted:" << join->join_inserted << thr_method_swc(settings().join_word);
    else if (join) c << "\n#join=gap:" << f32_text(settings().join_gap) <<",bridges:" << join->join_bridges << ",trees:" << join->join_trees_in << "->" << join->join_trees_out;
    if (cover && cover->have_prune) c << "\n" << prune_comment(settings().prune_opts, cover->prune);
    if (radius_thr) {
        const pnr_radius_opts &ro = settings().radius;
        c << "\n#radius=measured,thr=";
        if (ro.rel_pct > 0) c << "rel:" << ro.rel_pct;
        else c << *radius_thr;
        c << ",rmax=" << ro.rmax << ",bg=" << ro.bg_permille;
        if (ro.rel_pct == 0) c << thr_method_swc(settings().radius_word);
    }
    if (cover && cover->have_coverage) {
        char buf[200];
        snprintf(buf, sizeof buf, "\n#coverage=thr:%d,covered:%.6f,on_signal:%.6f,intensity:%.6f,tree_voxels:%lld", (int)cover->coverage.thr_used, cover->coverage.covered,
                 cover->coverage.on_signal, cover->coverage.covered_intensity, (long long)cover->coverage.n_tree);
        c << buf;
    }
    return c.str();
}

bool advantra_func(const std::vector<char *> &infiles, const std::vector<char *> &paras_c, int device, const std::string &raw_dims,
                   Result *result)
{
    if (infiles.empty()) {
        fprintf(stderr, "Need input image. \n"); // :286-289
        return false;
    }
    std::vector<std::string> paras(paras_c.begin(), paras_c.end());
    pnr_params p;
    std::string err;
    const int pr = parse_params(paras, p, err);
    if (pr == -1) {
        fprintf(stderr, "\nNeeds %d input parameters.\n\n", nrInputParams);
        print_help();
        return false;
    }
    if (pr == -2) {
        fprintf(stderr, "%s\n", err.c_str()); // v3d_msg(...); return 0
        return true;
    }
    Stack st;
    const auto tl0 = std::chrono::steady_clock::now();
    const Settings &S = settings();
    const Loaded loaded = load_input_stack(infiles[0], raw_dims, st);
    if (loaded != Loaded::ok) return loaded == Loaded::unreadable; // (an unreadable stack stops as a range error does: v3d_msg(...); return 0)
    Result local;
    Result *R = result ? result : &local;
    const double t_load = std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
    // a failure of the device library (no GPU, out of memory, a failed exchange) has no counterpart in the reference's contract:
    // it is reported on stderr by reconstruction_func and makes the function -- and the CLI's exit status -- fail
    const uint16_t *deep = st.bits == 16 ? st.samples16() : nullptr;
    if (!reconstruction_func(deep ? nullptr : st.bytes(), st.w, st.h, st.l, infiles[0], paras, p, device, R, deep, S.windowed ? &S.window : nullptr))
        return false;
    if (settings().rank == 0) {
        // what a user of advantra_func waits for (Advantra_plugin.cpp:2241 load, :2183-2731 reconstruction_func, :2164 the SWC)
        R->t_load = t_load;
        R->t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
        printf("wall: load %.3f s, context + upload %.3f s, frangi %.3f s, seeds %.3f s, selection %.3f s, tracing %.3f s, reconstruct %.3f s, "
               "write %.3f s | total %.3f s for %lld voxels\n",
               R->t_load, R->t_setup, R->t_frangi, R->t_seeds, R->t_select, R->t_trace, R->t_recon, R->t_write, R->t_total, (long long)(st.w * st.h * st.l));
    }
    return true;
}

// ---- the few collectives of the sharded path, over the transport the ranks were joined with: the shared-memory all-gather of the
// ranks of this host (default) or RCCL (--exchange rccl) -----------------------------------------------------------------------------
namespace {
constexpr size_t XCHUNK = 1 << 18; // bytes per rank and call (both transports are opened with this capacity)
bool allgather_bytes(pnr_allgather_fn fn, void *user, int world, const void *send, size_t n, std::vector<unsigned char> &out)
{
    out.assign(n * (size_t)world, 0);
    std::vector<unsigned char> sb(XCHUNK), rb(XCHUNK * (size_t)world);
    for (size_t off = 0; off < n || off == 0; off += XCHUNK) {
        const size_t m = std::min(XCHUNK, n - off);
        if (m) std::memcpy(sb.data(), (const unsigned char *)send + off, m);
        if (fn(user, sb.data(), rb.data(), (int64_t)m) != PNR_OK) return false;
        for (int r = 0; r < world; r++)
            if (m) std::memcpy(out.data() + (size_t)r * n + off, rb.data() + (size_t)r * m, m);
        if (n == 0) break;
    }
    return true;
}

// ---- the tracing run: reconstruction_func as a sequence of stages ----------------------------------------------------------------------
using clk = std::chrono::steady_clock;
double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// the kernel timers while one stage runs: switched on if `on`; end() reads the stage's timer group into (ms, launches) and switches them
// off, as leaving the stage does
struct Profile {
    pnr_ctx *const ctx;
    const char *const group;
    bool on;
    double ms = 0;
    int64_t launches = 0;
    Profile(pnr_ctx *c, const char *g, bool o) : ctx(c), group(g), on(o) { if (on) pnr_set_profiling(ctx, 1); }
    void end()
    {
        if (!on) return;
        pnr_get_kernel_ms(ctx, group, &ms, &launches);
        pnr_set_profiling(ctx, 0);
        on = false;
    }
    ~Profile() { if (on) pnr_set_profiling(ctx, 0); }
};

// the tree list as the library's tree calls take it.  Entry i belongs to tree[i], the dummy included: the nodes alone start at entry 1.
// par: the parent's index among the nodes alone, -1 = none; rad: what save_treelist writes (radius: the measured column, or nullptr)
struct TreeArrays {
    std::vector<float> xyz, rad;
    std::vector<int32_t> par;
};
TreeArrays tree_arrays(const std::vector<pnr_node> &tree, const std::vector<int32_t> &parent, const std::vector<float> *radius)
{
    const size_t nt = std::max<size_t>(tree.size(), 1); // (an empty list still has the dummy's entries)
    TreeArrays T{std::vector<float>(3 * nt, 0.f), std::vector<float>(nt, 0.f), std::vector<int32_t>(nt, -1)};
    for (size_t i = 0; i < tree.size(); i++) {
        const pnr_node &nd = tree[i];
        T.xyz[3 * i] = nd.x, T.xyz[3 * i + 1] = nd.y, T.xyz[3 * i + 2] = nd.z;
        T.par[i] = parent[i] > 0 ? parent[i] - 1 : -1;
        T.rad[i] = (radius && (*radius)[i] >= 0.f) ? (*radius)[i] : 1.f * nd.sig;
    }
    return T;
}

// one tracing run: the arguments of reconstruction_func, what its stages hand on to one another, and the stages in the order they run
struct Pipeline {
    const unsigned char *data1d;
    const long long w, h, l;
    const std::string &inimg_file;
    const std::vector<std::string> &paras;
    pnr_params p;
    const uint16_t *const data16;
    const pnr_window *const win;
    const Settings &S = settings();
    const int rank = S.rank, world = S.world;
    // the transport of the sharded path's collectives
    pnr_rccl_exchange *const RX = S.rccl;
    const pnr_allgather_fn xfn = RX ? pnr_rccl_allgather : pnr_shm_allgather;
    void *const X = RX ? (void *)RX : (void *)S.exchange;
    const bool sharded = world > 1 || S.force_shard;
    const pnr_filter_opts &fo = S.filter;
    const bool filtered = fo.median || fo.tophat_r || S.morph() || S.local.r || S.despeckle;
    Ctx ctx;
    Result R;
    bool ok = true;
    clk::time_point t_begin, t_created, t0, t1, t2, t3, t4, t5;
    std::vector<pnr_seed> seeds;
    int64_t nfound = 0, nseeds = 0, nn = 0, nl = 0, used = 0, iters = 0;
    int32_t window[2] = {-1, -1}; // 16-bit input: the window it was mapped with
    std::vector<unsigned char> mapped;
    std::vector<float> radius; // --measure-radius: the radius column, measured on the volume this context traced

    void soma() // SOMA EXTR. (:2426-2486): erosion, xy blur, max-entropy threshold, regions -> soma nodes
    {
        if (p.somaradius <= 0) { printf("no soma detection\n"); return; }
        auto ts = clk::now();
        int32_t th = 0;
        int64_t nsoma = 0;
        ok = ok && pnr_soma(ctx, nullptr, &th, &nsoma) == PNR_OK;
        printf("imerode(%d) imgaussian(%d) maxentropy_th() %d  %lld soma regions  %.3f sec.\n", p.somaradius, p.somaradius, (int)th, (long long)nsoma, secs(ts, clk::now()));
    }

    void despeckle() // --despeckle: the small foreground components of the (filtered) volume are cleared
    {
        if (!S.despeckle || !ok) return;
        const auto tf = clk::now();
        pnr_components_info ci = {};
        pnr_components_opts co = S.despeckle_opts;
        ok = resolve_threshold(ctx, S.despeckle_word, co.thr) && pnr_despeckle_volume(ctx, &co, &ci) == PNR_OK;
        R.t_despeckle = secs(tf, clk::now());
        R.despeckle_removed = ci.n_small, R.despeckle_voxels = ci.vox_small, R.despeckle_thr = ci.thr_used;
        printf("despeckle... %lld components of fewer than %lld voxels (%lld voxels) removed, threshold %d, %g sec.\n", (long long)ci.n_small,
               (long long)S.despeckle_opts.min_size, (long long)ci.vox_small, (int)ci.thr_used, R.t_despeckle);
        if (S.timing) fprintf(stderr, "[pnr host] despeckle: %.3f s\n", R.t_despeckle);
    }

    void local_threshold() // --local-threshold: the volume is replaced by its local threshold
    {
        if (!S.local.r || !ok) return;
        const auto tf = clk::now();
        Profile prof(ctx, "local_threshold", S.timing || S.verbose);
        pnr_local_info li = {};
        ok = local_stage(ctx, &li);
        R.t_local = secs(tf, clk::now());
        prof.end();
        R.local_kept = li.n_kept;
        printf("local threshold... box %d x %d x %d, offset %d, scale %d/256, %lld of %lld voxels kept, %g sec.\n", (int)li.rx, (int)li.ry, (int)li.rz, (int)S.local.offset,
               (int)S.local.scale_256, (long long)li.n_kept, (long long)li.n_vox, R.t_local);
        if (S.verbose) printf("local threshold kernels %.3f ms in %lld launches\n", prof.ms, (long long)prof.launches);
        if (S.timing) fprintf(stderr, "[pnr host] local threshold: %.3f s, kernels %.3f ms in %lld launches\n", R.t_local, prof.ms, (long long)prof.launches);
    }

    void morph() // --fill-holes / --hmax / --hdome: the (filtered) volume is replaced by its reconstruction, then thresholded locally and despeckled
    {
        if (S.morph() && ok) {
            const auto tf = clk::now();
            Profile prof(ctx, "morph", S.timing || S.verbose);
            std::vector<MorphStage> stages;
            ok = morph_stages(ctx, &stages);
            R.t_morph = secs(tf, clk::now());
            prof.end();
            auto level = [](int v) { return v ? std::to_string(v) : std::string("off"); };
            long long changed = 0;
            for (const MorphStage &st : stages) changed += st.info.n_changed;
            printf("morphology... fill holes %s, h-maxima %s, h-dome %s, %lld voxels changed, %g sec.\n", S.fill_holes == 6 ? "3d" : S.fill_holes == 4 ? "2d" : "off",
                   level(S.hmax).c_str(), level(S.hdome).c_str(), changed, R.t_morph);
            if (S.verbose) printf("morphology kernels %.3f ms in %lld launches\n", prof.ms, (long long)prof.launches);
            if (S.timing) fprintf(stderr, "[pnr host] morph: %.3f s, kernels %.3f ms in %lld launches\n", R.t_morph, prof.ms, (long long)prof.launches);
        }
        local_threshold();
        despeckle();
    }

    void filter() // --median / --subtract-background (/ --fill-holes / --hmax / --hdome / --despeckle): the context's volume is replaced by its filtered bytes
    {
        if (!filtered || !ok) return;
        if (!fo.median && !fo.tophat_r) return morph();
        const auto tf = clk::now();
        Profile prof(ctx, "filter", S.timing || S.verbose);
        ok = pnr_filter_volume(ctx, &fo) == PNR_OK;
        R.t_filter = secs(tf, clk::now());
        prof.end();
        printf("pre-filter... median %s, top-hat %d, %g sec.\n", fo.median == 3 ? "3d" : fo.median == 2 ? "2d" : "off", (int)fo.tophat_r, R.t_filter);
        if (S.verbose) printf("pre-filter kernels %.3f ms in %lld launches\n", prof.ms, (long long)prof.launches);
        if (S.timing) fprintf(stderr, "[pnr host] filter: %.3f s, kernels %.3f ms in %lld launches\n", R.t_filter, prof.ms, (long long)prof.launches);
        morph();
    }

    void seeds_one_gpu() // volume, pre-filter, soma, Frangi, and the scored and sorted seeds
    {
        ok = (data16 ? pnr_set_volume_u16(ctx, data16, w, h, l, 1, 0, win, &window[0], &window[1]) : pnr_set_volume(ctx, data1d, w, h, l)) == PNR_OK;
        if (S.timing) fprintf(stderr, "[pnr host] context %.3f s, upload of %.2f GB %.3f s\n", secs(t_begin, t_created), (double)(w * h * l) / 1e9, secs(t_created, clk::now()));
        filter();
        if (ok) soma();
        t0 = clk::now();
        ok = ok && pnr_frangi(ctx, &R.Jmin, &R.Jmax) == PNR_OK; // :2496-2512
        t1 = clk::now();
        const pnr_seed *found = nullptr;
        ok = ok && pnr_extract_seeds(ctx, &found, &nfound) == PNR_OK; // :2549
        t2 = clk::now();
        if (!ok) return;
        seeds.assign(found, found + nfound);
        printf("seed extraction... %gk seeds,  %g sec.\n", nfound / 1000.0, secs(t1, t2));
        ok = pnr_score_filter_sort_seeds(ctx, seeds.data(), nfound, &nseeds) == PNR_OK; // :2561-2586
        seeds.resize((size_t)nseeds);
    }

    void whole_stack_on_every_rank() // sharded: data1d becomes the 8-bit stack as it is traced
    {
        if (data16) { // every rank maps the whole stack once and runs the 8-bit path on it: slabs and stack share one window
            mapped.resize((size_t)(w * h * l));
            ok = pnr_set_volume_u16(ctx, data16, w, h, l, 1, 0, win, &window[0], &window[1]) == PNR_OK && pnr_get_volume(ctx, mapped.data()) == PNR_OK;
            data1d = mapped.data();
        }
        if (filtered) { // every rank filters its own copy of the whole stack (the filter is deterministic: all ranks hold the same bytes)
            if (!data16) ok = pnr_set_volume(ctx, data1d, w, h, l) == PNR_OK;
            filter();
            mapped.resize((size_t)(w * h * l));
            ok = ok && pnr_get_volume(ctx, mapped.data()) == PNR_OK;
            data1d = mapped.data();
        }
    }

    // sharded: this rank's z-slab with its halo (the z pass of the widest Gaussian + the radius-2 Hessian stencil): exact Frangi / seeds
    // of the planes it owns, no halo exchange -- every rank has the whole stack
    void slab_frangi_and_seeds(std::vector<pnr_seed> &mine)
    {
        float smax = 0;
        for (int i = 0; i < p.nsig; i++) smax = std::max(smax, p.sig[i]);
        const long long halo = (long long)std::ceil(3 * (smax / p.zdist)) + 2;
        const long long z0 = l * rank / world, z1 = l * (rank + 1) / world, zlo = std::max(0LL, z0 - halo), zhi = std::min(l, z1 + halo);
        float mm[2] = {FLT_MAX, -FLT_MAX}; // (min, max) of J over the owned planes
        if (z1 > z0) {
            ok = ok && pnr_set_volume(ctx, data1d + zlo * w * h, w, h, zhi - zlo) == PNR_OK;
            ok = ok && pnr_frangi_slab(ctx, z0 - zlo, z1 - zlo, &mm[0], &mm[1]) == PNR_OK;
        }
        // the 2-float all-reduce: one ncclAllReduce over RCCL, an all-gather + local reduction through shared memory
        R.Jmin = FLT_MAX; R.Jmax = -FLT_MAX;
        if (RX) {
            R.Jmin = mm[0]; R.Jmax = mm[1];
            if (pnr_rccl_allreduce_minmax(RX, &R.Jmin, &R.Jmax) != PNR_OK) ok = false;
        } else {
            std::vector<unsigned char> all;
            if (!allgather_bytes(xfn, X, world, mm, sizeof(mm), all)) ok = false;
            for (int r = 0; r < world && ok; r++) {
                float q[2];
                std::memcpy(q, all.data() + (size_t)r * sizeof(q), sizeof(q));
                R.Jmin = std::min(R.Jmin, q[0]); R.Jmax = std::max(R.Jmax, q[1]);
            }
        }
        t1 = clk::now();
        const pnr_seed *found = nullptr;
        int64_t nmine = 0;
        if (ok && z1 > z0) {
            ok = pnr_quantise_j8(ctx, R.Jmin, R.Jmax) == PNR_OK && pnr_extract_seeds_range(ctx, z0 - zlo, z1 - zlo, &found, &nmine) == PNR_OK;
            if (ok) {
                mine.assign(found, found + nmine);
                for (auto &sd : mine) sd.z += (float)zlo;
            }
        }
        t2 = clk::now();
    }

    void gather_seeds(std::vector<pnr_seed> &mine) // sharded: this slab's seeds scored, every rank's gathered and sorted
    {
        const int64_t nmine = (int64_t)mine.size();
        int64_t cnt[2] = {nmine, 0};
        if (ok && nmine) ok = pnr_score_filter_seeds(ctx, mine.data(), nmine, &cnt[1]) == PNR_OK; // this slab's seeds: znccBBB + threshold
        if (!ok) cnt[0] = -1; // a rank that failed says so: every collective up to here was entered by everybody, none after is
        std::vector<unsigned char> counts;
        if (!allgather_bytes(xfn, X, world, cnt, sizeof(cnt), counts)) ok = false;
        int64_t mx = 0;
        std::vector<int64_t> kept((size_t)world);
        for (int r = 0; r < world; r++) {
            int64_t q[2] = {-1, 0};
            if (counts.size() >= (size_t)(r + 1) * sizeof(q)) std::memcpy(q, counts.data() + (size_t)r * sizeof(q), sizeof(q));
            if (q[0] < 0) { if (ok) fprintf(stderr, "rank %d failed\n", r); ok = false; continue; }
            nfound += q[0]; kept[(size_t)r] = q[1]; mx = std::max(mx, q[1]);
        }
        mine.resize((size_t)mx); // padded payloads
        std::vector<unsigned char> pay;
        if (ok && !allgather_bytes(xfn, X, world, mine.data(), (size_t)mx * sizeof(pnr_seed), pay)) ok = false;
        for (int r = 0; r < world && ok; r++) { // rank order = the z-major order of the unsharded extraction
            const pnr_seed *q = (const pnr_seed *)(pay.data() + (size_t)r * (size_t)mx * sizeof(pnr_seed));
            seeds.insert(seeds.end(), q, q + kept[(size_t)r]);
        }
        if (!ok) return;
        printf("seed extraction... %gk seeds,  %g sec.\n", nfound / 1000.0, secs(t1, t2));
        nseeds = (int64_t)seeds.size();
        if (nseeds) ok = pnr_sort_seeds(ctx, seeds.data(), nseeds, &nseeds) == PNR_OK; // the list one GPU would have
        seeds.resize((size_t)nseeds);
    }

    void seeds_sharded()
    {
        whole_stack_on_every_rank();
        std::vector<pnr_seed> mine;
        slab_frangi_and_seeds(mine);
        ok = ok && pnr_set_volume(ctx, data1d, w, h, l) == PNR_OK; // scoring and tracing see the whole stack
        if (ok) soma();
        gather_seeds(mine);
    }

    // :2658-2710: the particle filters on the GPU (a window of traces refilled as they stop), the bookkeeping replayed on the
    // host in seed order; the graph stays in the context and is fetched once its size is known
    void trace()
    {
        printf("seed selection & sorting... %gk seeds, %g sec.\ntracing...\n", nseeds / 1000.0, secs(t2, t3));
        if (S.verbose) pnr_set_option(ctx, "trace_log", 1);
        if (S.timing) { pnr_set_option(ctx, "trace_timing", 1); pnr_set_option(ctx, "recon_timing", 1); }
        if (!sharded)
            ok = pnr_trace_replay(ctx, seeds.data(), nseeds, 0, nullptr, 0, &nn, nullptr, 0, &nl, &used, &iters) == PNR_OK;
        else // every rank traces seeds rank, rank + world, ...; finished traces are exchanged and replayed in seed order on every rank
            ok = pnr_trace_replay_sharded(ctx, seeds.data(), nseeds, rank, world, xfn, X, nullptr, 0, &nn, nullptr, 0, &nl, &used, &iters) == PNR_OK;
        if (ok) {
            R.nodes.resize((size_t)nn);
            R.links.resize((size_t)(2 * nl));
            ok = pnr_get_graph(ctx, R.nodes.data(), nn, &nn, R.links.data(), nl, &nl) == PNR_OK;
        }
        if (ok && S.verbose) print_trace_log();
    }

    void print_trace_log() // what the reference prints while it traces (TRACING_VERBOSE :2677; tracker.cpp:866,879,908,916)
    {
        int64_t nlog = 0;
        pnr_get_trace_log(ctx, nullptr, 0, &nlog);
        std::vector<int32_t> lg((size_t)nlog * 5);
        pnr_get_trace_log(ctx, lg.data(), nlog, &nlog);
        int trace_count = 0;
        for (int64_t k = 0; k < nlog; k++) {
            const int32_t *e = &lg[(size_t)k * 5];
            const pnr_seed &sd = seeds[(size_t)e[0]];
            if (e[1] == 0)
                printf("\nTrace: %6d\t [%4.1f, %4.1f, %4.1f]\t sc=%6.2f\t corr=%3.2f\t progress %3.2f%%\t", ++trace_count, sd.x, sd.y, sd.z, sd.score, sd.corr,
                       (100.0 * e[0]) / (double)nseeds);
            float cv;
            std::memcpy(&cv, &e[4], 4);
            switch (e[3]) {
            case 3: printf("\n--%d[%d], SOMA, idx=%d", e[2], p.ni, e[4]); break;
            case 2: printf("\n--%d[%d], DENSITY, nodespervol=%d", e[2], p.ni, e[4]); break;
            case 1: printf("\n--%d[%d], success=0, corr=%1.2f", e[2], p.ni, cv); break;
            default: printf("\n--%d[%d], TRACK LIMIT, niter=%d", e[2], p.ni, p.ni); break;
            }
        }
        printf("\n");
    }

    // reconstruct(n0, ...) :2729 -> :2096-2181: refinement and grouping queries on this rank's GPU, trees and resampling on the host
    bool reconstruct()
    {
        int64_t cap = std::max<int64_t>(16, 4 * nn), nt = 0;
        for (;;) {
            R.tree.resize((size_t)cap);
            R.parent.resize((size_t)cap);
            if (pnr_reconstruct_ctx(ctx, R.nodes.data(), nn, R.links.data(), nl, 0, 0, 0, 0, 0, S.single_tree ? -1 : 0, R.tree.data(), R.parent.data(), cap, &nt) != PNR_OK) return lib_fail(nullptr);
            if (nt <= cap) break;
            cap = nt;
        }
        R.tree.resize((size_t)nt);
        R.parent.resize((size_t)nt);
        return true;
    }

    bool join() // --join: the forest becomes one tree (pnr_join_trees), the tree list is rewritten in tree order
    {
        if (!S.join || R.tree.size() <= 1) return true;
        const auto tj = clk::now();
        const int64_t n = (int64_t)R.tree.size() - 1; // without the dummy
        const TreeArrays T = tree_arrays(R.tree, R.parent, nullptr);
        int64_t root = -1;
        for (int64_t i = 0; i < n && S.join_root_id == 0 && root < 0; i++)
            if (R.tree[(size_t)i + 1].type == 1) root = i; // the first soma node
        if (S.join_root_id > 0) root = S.join_root_id - 1;
        if (root >= n) {
            fprintf(stderr, "--join-root %lld: the tree has %lld nodes\n", S.join_root_id, (long long)n);
            return false;
        }
        if (S.join_geodesic) return join_geodesic(tj, T, n, root);
        const pnr_join_opts jo = {p.zdist, S.join_gap, (int32_t)root};
        std::vector<int32_t> par_out((size_t)n), order((size_t)n), comp((size_t)n);
        int64_t nb = 0, t_in = 0, t_out = 0;
        Profile prof(ctx, "join", S.timing);
        if (pnr_join_trees(ctx, T.xyz.data() + 3, T.par.data() + 1, n, &jo, par_out.data(), order.data(), comp.data(), nullptr, 0, &nb, &t_in, &t_out) != PNR_OK) return lib_fail(nullptr);
        R.join_bridges = nb, R.join_trees_in = t_in, R.join_trees_out = t_out;
        std::vector<int32_t> pos((size_t)n, -1); // node -> its line; component 0 comes first in the order
        std::vector<pnr_node> tree(1, R.tree[0]);
        std::vector<int32_t> parent(1, R.parent[0]);
        for (int64_t k = 0; k < n; k++) {
            const int32_t v = order[(size_t)k];
            if (S.join_keep_largest && comp[(size_t)v] != 0) break;
            pos[(size_t)v] = (int32_t)tree.size();
            tree.push_back(R.tree[(size_t)v + 1]);
            parent.push_back(par_out[(size_t)v] < 0 ? -1 : pos[(size_t)par_out[(size_t)v]]); // (the parent was written before)
        }
        R.tree.swap(tree);
        R.parent.swap(parent);
        R.t_join = secs(tj, clk::now());
        printf("join... gap %g, %lld bridges, %lld -> %lld trees, %zu nodes written, %g sec.\n", (double)S.join_gap, (long long)nb, (long long)t_in, (long long)t_out,
               R.tree.size() - 1, R.t_join);
        if (S.timing) {
            int64_t rounds = 0;
            prof.end();
            pnr_get_option(ctx, "join_rounds", &rounds);
            fprintf(stderr, "[pnr host] join: %.3f s, %lld rounds, kernels %.3f ms in %lld launches\n", R.t_join, (long long)rounds, prof.ms, (long long)prof.launches);
        }
        return true;
    }

    // --join-geodesic: the fragments are joined along the signal (pnr_geodesic_bridges), the bridges' voxels become nodes, and the tree
    // list is rewritten in tree order
    bool join_geodesic(clk::time_point tj, const TreeArrays &T, int64_t n, int64_t root)
    {
        pnr_geojoin_opts go = {S.join_thr, S.join_limit, 1.f, nullptr};
        if (!resolve_threshold(ctx, S.join_word, go.thr)) return false;
        GeoJoined J;
        Profile prof(ctx, "geojoin", S.timing);
        if (!geodesic_join(ctx, T.xyz.data() + 3, T.par.data() + 1, n, go, root, w, h, l, J)) return false;
        const pnr_geojoin_info &gi = J.info;
        R.join_bridges = gi.n_bridges, R.join_trees_in = gi.n_trees_in, R.join_trees_out = gi.n_trees_out, R.join_inserted = gi.n_inserted, R.join_thr_used = gi.thr_used;
        std::vector<int32_t> pos((size_t)J.n2(), -1); // node -> its line; component 0 comes first in the order
        std::vector<pnr_node> tree(1, R.tree[0]);
        std::vector<int32_t> parent(1, R.parent[0]);
        for (int64_t k = 0; k < J.n2(); k++) {
            const int32_t v = J.order[(size_t)k];
            if (S.join_keep_largest && J.comp[(size_t)v] != 0) break;
            pos[(size_t)v] = (int32_t)tree.size();
            if (v < n) tree.push_back(R.tree[(size_t)v + 1]);
            else { // an inserted node: node a of its bridge moved onto the voxel, with the smaller radius of a and b
                const pnr_geo_bridge &b = J.bridges[(size_t)J.bridge_of[(size_t)(v - n)]];
                pnr_node nd = R.tree[(size_t)b.a + 1];
                nd.x = J.xyz[3 * (size_t)v], nd.y = J.xyz[3 * (size_t)v + 1], nd.z = J.xyz[3 * (size_t)v + 2];
                nd.sig = std::min(nd.sig, R.tree[(size_t)b.b + 1].sig);
                tree.push_back(nd);
            }
            parent.push_back(J.par_out[(size_t)v] < 0 ? -1 : pos[(size_t)J.par_out[(size_t)v]]); // (the parent was written before)
        }
        R.tree.swap(tree);
        R.parent.swap(parent);
        R.t_join = secs(tj, clk::now());
        printf("join... geodesic %llu, %lld bridges, %lld -> %lld trees, %lld nodes inserted, %zu nodes written, %g sec.\n", S.join_limit, (long long)gi.n_bridges,
               (long long)gi.n_trees_in, (long long)gi.n_trees_out, (long long)gi.n_inserted, R.tree.size() - 1, R.t_join);
        if (S.timing) {
            prof.end();
            fprintf(stderr, "[pnr host] join: %.3f s, %d rounds, meet kernels %.3f ms in %lld launches\n", R.t_join, (int)gi.rounds, prof.ms, (long long)prof.launches);
        }
        return true;
    }

    bool prune() // --prune: short side branches and low trees go (pnr_prune_tree); the kept nodes stay in their order
    {
        if (!S.prune || R.tree.size() <= 1) return true;
        const int64_t n = (int64_t)R.tree.size() - 1; // without the dummy
        const TreeArrays T = tree_arrays(R.tree, R.parent, nullptr);
        pnr_prune_opts po = S.prune_opts;
        po.zscale = p.zdist;
        std::vector<uint8_t> keep((size_t)n);
        std::vector<int32_t> idx((size_t)n), par((size_t)n);
        int64_t m = 0;
        Profile prof(ctx, "prune", S.timing);
        if (pnr_prune_tree(ctx, T.xyz.data() + 3, T.rad.data() + 1, T.par.data() + 1, n, &po, &R.prune, keep.data(), nullptr, nullptr, nullptr, nullptr) != PNR_OK ||
            pnr_prune_apply(T.par.data() + 1, keep.data(), n, idx.data(), par.data(), &m) != PNR_OK)
            return lib_fail(nullptr);
        R.have_prune = true;
        std::vector<pnr_node> tree(1, R.tree[0]);
        std::vector<int32_t> parent(1, R.parent[0]);
        for (int64_t v = 0; v < n; v++) {
            if (!keep[(size_t)v]) continue;
            tree.push_back(R.tree[(size_t)v + 1]);
            parent.push_back(par[(size_t)idx[(size_t)v]] < 0 ? -1 : par[(size_t)idx[(size_t)v]] + 1);
        }
        R.tree.swap(tree);
        R.parent.swap(parent);
        printf("prune... %lld of %lld nodes in %lld segments removed, %zu nodes written\n", (long long)R.prune.n_removed, (long long)n, (long long)R.prune.n_removed_segments,
               R.tree.size() - 1);
        prof.end();
        if (S.timing) fprintf(stderr, "[pnr host] prune: %d + %d rounds, kernels %.3f ms in %lld launches\n", (int)R.prune.rounds_up, (int)R.prune.rounds_down, prof.ms, (long long)prof.launches);
        return true;
    }

    bool measure_radius() // --measure-radius: the radius column, measured on the volume this context traced
    {
        if (!S.measure_radius) return true;
        const size_t nt = R.tree.size();
        const TreeArrays T = tree_arrays(R.tree, R.parent, nullptr);
        R.radius_k.assign(nt, -1);
        Profile prof(ctx, "radius", S.timing);
        pnr_radius_opts ro = S.radius;
        if (ro.rel_pct == 0 && !resolve_threshold(ctx, S.radius_word, ro.thr)) return false;
        if (pnr_measure_radii(ctx, T.xyz.data(), (int64_t)nt, &ro, R.radius_k.data(), &R.radius_thr) != PNR_OK) return lib_fail(nullptr);
        if (nt) R.radius_k[0] = -1; // the dummy
        radius = measured_radius_column(R.tree, R.radius_k);
        t5 = clk::now();
        R.t_radius = secs(t4, t5) - R.t_recon;
        printf("radius measurement... %zu nodes, %g sec.\n", nt ? nt - 1 : 0, R.t_radius);
        prof.end();
        if (S.timing) fprintf(stderr, "[pnr host] radius: %.3f s, kernels %.3f ms in %lld launches\n", R.t_radius, prof.ms, (long long)prof.launches);
        return true;
    }

    bool render() // --mask / --residual / --coverage: the final tree rendered on the traced volume
    {
        if (S.mask_out.empty() && S.residual_out.empty() && !S.coverage) return true;
        const auto tr = clk::now();
        const int64_t n = std::max<int64_t>((int64_t)R.tree.size() - 1, 0); // without the dummy
        const TreeArrays T = tree_arrays(R.tree, R.parent, radius.empty() ? nullptr : &radius);
        const size_t N = (size_t)(w * h * l);
        std::vector<unsigned char> mask(S.mask_out.empty() ? 0 : N), residual(S.residual_out.empty() ? 0 : N);
        const pnr_render_opts ro = {p.zdist, 1.f, 0.f, -1};
        Profile prof(ctx, "render", S.timing);
        if (pnr_tree_coverage(ctx, T.xyz.data() + 3, T.rad.data() + 1, T.par.data() + 1, n, &ro, &R.coverage, nullptr, nullptr, nullptr,
                              S.mask_out.empty() ? nullptr : mask.data(), S.residual_out.empty() ? nullptr : residual.data()) != PNR_OK)
            return lib_fail(nullptr);
        if (!S.mask_out.empty() && !write_stack(S.mask_out, mask.data(), w, h, l)) return false;
        if (!S.residual_out.empty() && !write_stack(S.residual_out, residual.data(), w, h, l)) return false;
        R.have_coverage = true;
        R.t_render = secs(tr, clk::now());
        printf("render... %lld tree voxels, covered %.4f, on signal %.4f, intensity %.4f (threshold %d), %g sec.\n", (long long)R.coverage.n_tree, R.coverage.covered,
               R.coverage.on_signal, R.coverage.covered_intensity, (int)R.coverage.thr_used, R.t_render);
        prof.end();
        if (S.timing) fprintf(stderr, "[pnr host] render: %.3f s, kernels %.3f ms in %lld launches\n", R.t_render, prof.ms, (long long)prof.launches);
        t5 = clk::now();
        return true;
    }

    void write_midres() // the saveMidres taps of reconstruct() (:2098-2141)
    {
        save_nodelist(R.nodes, R.links, inimg_file + "_n0_.swc");
        static const char *const names[] = {"", "_n0res_.swc", "_n1_.swc", "_n2_.swc", "_n2tree_.swc"};
        for (int stage = 1; stage <= 4; stage++) {
            int64_t sn = 0, sl = 0;
            if (pnr_reconstruct_stage(R.nodes.data(), nn, R.links.data(), nl, 0, 0, 0, 0, 0, stage, nullptr, 0, &sn, nullptr, 0, &sl) != PNR_OK) break;
            std::vector<pnr_node> tn((size_t)sn);
            std::vector<int32_t> tl((size_t)(2 * sl));
            if (pnr_reconstruct_stage(R.nodes.data(), nn, R.links.data(), nl, 0, 0, 0, 0, 0, stage, tn.data(), sn, &sn, tl.data(), sl, &sl) != PNR_OK) break;
            if (stage < 4) save_nodelist(tn, tl, inimg_file + names[stage]);
            else { // a tree list: every node carries its parent (or none)
                std::vector<int32_t> par((size_t)sn, -1);
                for (int64_t k = 0; k < sl; k++) par[(size_t)tl[(size_t)(2 * k)]] = tl[(size_t)(2 * k + 1)];
                save_treelist(tn, par, inimg_file + names[stage], -1, 1.f, "", "");
            }
        }
    }

    void write() // the SWC file, the --save-midres files and the closing line
    {
        R.swc_path = inimg_file + (S.single_tree ? "_Advantra1.swc" : "_Advantra.swc"); // :2152 / :2164
        save_treelist(R.tree, R.parent, R.swc_path, -1, 1.f, "Advantra",
                      swc_comment(paras, p, data16 ? window : nullptr, S.measure_radius ? &R.radius_thr : nullptr, S.join ? &R : nullptr, &R),
                      radius.empty() ? nullptr : &radius);
        if (S.save_midres) write_midres();
        R.t_write = secs(t5, clk::now());
        printf("%s\n%lld trace nodes, %lld traces, %lld SMC iterations, %zu tree nodes | frangi %.3f s, seeds %.3f s, selection %.3f s, "
               "tracing %.3f s, reconstruct %.3f s\n",
               R.swc_path.c_str(), (long long)nn - 1, (long long)used, (long long)iters, R.tree.size() - 1, R.t_frangi, R.t_seeds, R.t_select,
               R.t_trace, R.t_recon);
    }
};
} // namespace

bool reconstruction_func(const unsigned char *data1d, long long w, long long h, long long l, const std::string &inimg_file,
                         const std::vector<std::string> &paras, pnr_params p, int device, Result *result, const uint16_t *data16,
                         const pnr_window *win)
{
    Pipeline P{data1d, w, h, l, inimg_file, paras, p, data16, win};
    Result &R = P.R;
    if (P.sharded && (!P.X || l < 2)) {
        fprintf(stderr, "--ranks needs a stack of at least 2 planes and an open exchange\n");
        return false;
    }
    if (P.rank != 0 && !freopen("/dev/null", "w", stdout)) return false; // only rank 0 talks
    P.p.rng_seed = settings().rng_seed;
    printf("-------------  ADVANTRA  -------------\n");
    P.t_begin = clk::now();
    if (!P.ctx.create(P.p, device, nullptr)) return false;
    pnr_set_option(P.ctx, "local_ranks", P.world);
    P.t_created = P.t0 = P.t1 = P.t2 = clk::now();
    if (P.sharded) P.seeds_sharded();
    else P.seeds_one_gpu();
    P.t3 = clk::now();
    if (P.ok) P.trace();
    P.t4 = clk::now();
    if (!P.ok) return lib_fail(nullptr);
    R.n_seeds_init = P.nfound; R.n_seeds = P.nseeds; R.n_traces = P.used; R.n_iterations = P.iters;
    if (P.rank != 0) { // every rank holds the same graph; rank 0 post-processes and writes it
        if (result) *result = R;
        return true;
    }
    R.t_frangi = secs(P.t0, P.t1); R.t_seeds = secs(P.t1, P.t2); R.t_select = secs(P.t2, P.t3); R.t_trace = secs(P.t3, P.t4);
    R.t_setup = secs(P.t_begin, P.t0); // context, upload of the stack, soma path
    printf("\n-----\n%g%% seeds used \n", P.nseeds ? 100.0 * P.used / P.nseeds : 0.0);
    if (!P.reconstruct() || !P.join() || !P.prune()) return false;
    P.t5 = clk::now();
    R.t_recon = secs(P.t4, P.t5);
    if (!P.measure_radius() || !P.render()) return false;
    P.write();
    if (result) *result = R;
    return true;
}

} // namespace advantra
