// tools.cpp -- the tool modes of advantra_cli (see advantra_host.h): --distance, --join-swc (by gap, or --join-geodesic), --render-swc,
// --prune-swc, --components, --edt, --skeleton, --morph, --watershed, --geodesic and --auto-threshold.  Each loads its files, opens one context, makes one call through the C ABI and prints one JSON line.
#include "host_internal.h"
#include <algorithm>
#include <cmath>
#include <functional>

namespace advantra {

// `name` opened with `mode`, written by `body` and closed: false after a message on stderr
static bool write_file(const std::string &name, const char *mode, const std::function<void(FILE *)> &body)
{
    FILE *f = fopen(name.c_str(), mode);
    if (!f) {
        fprintf(stderr, "%s: cannot write the file\n", name.c_str());
        return false;
    }
    body(f);
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) {
        fprintf(stderr, "%s: write failed\n", name.c_str());
        return false;
    }
    return true;
}

bool morph_stages(pnr_ctx *ctx, std::vector<MorphStage> *stages)
{
    const Settings &S = settings();
    auto run = [&](int op, int conn, int h, const char *name) {
        const pnr_morph_opts o = {op, conn, h, 0};
        pnr_morph_info mi = {};
        if (pnr_morph_volume(ctx, &o, &mi) != PNR_OK) return false;
        if (stages) stages->push_back(MorphStage{name, h, mi});
        return true;
    };
    if (S.fill_holes && !run(PNR_MORPH_FILL, S.fill_holes, 0, "fill")) return false;
    if (S.hmax && !run(PNR_MORPH_HMAX, 26, S.hmax, "hmax")) return false;
    if (S.hdome && !run(PNR_MORPH_HDOME, 26, S.hdome, "hdome")) return false;
    return true;
}

bool local_stage(pnr_ctx *ctx, pnr_local_info *info)
{
    const Settings &S = settings();
    return !S.local.r || pnr_local_threshold_volume(ctx, &S.local, info) == PNR_OK;
}

bool parse_threshold_word(const char *txt, ThrWord &out)
{
    std::string name = txt;
    long lo = 0;
    const size_t colon = name.find(':');
    if (colon != std::string::npos) {
        char *end = nullptr;
        const char *t = txt + colon + 1;
        lo = strtol(t, &end, 10);
        if (!*t || *end || lo < 0 || lo > 255) return false;
        name.resize(colon);
    }
    pnr_threshold_opts o = {0, (int32_t)lo, 0, 0};
    if (name == "mean") o.method = PNR_THR_MEAN;
    else if (name == "otsu") o.method = PNR_THR_OTSU;
    else if (name == "triangle") o.method = PNR_THR_TRIANGLE;
    else if (name == "maxentropy") o.method = PNR_THR_MAXENTROPY;
    else if (name.size() > 3 && name.compare(0, 3, "top") == 0 && (isdigit((unsigned char)name[3]) || name[3] == '.')) {
        char *end = nullptr;
        const double pct = strtod(name.c_str() + 3, &end);
        if (*end || !(pct > 0.0 && pct < 100.0)) return false;
        o.method = PNR_THR_TOP;
        o.top_ppm = (int32_t)std::lround(pct * 1e4);
        if (o.top_ppm < 1 || o.top_ppm > 999999) return false;
    } else
        return false;
    out.given = true, out.opts = o, out.text = txt;
    return true;
}

bool resolve_threshold(pnr_ctx *ctx, const ThrWord &word, int32_t &thr)
{
    if (!word.given) return true;
    pnr_threshold_info ti = {};
    if (pnr_auto_threshold(ctx, &word.opts, &ti, nullptr) != PNR_OK) return lib_fail("pnr_auto_threshold");
    thr = ti.thr;
    return true;
}

std::string thr_method_json(const ThrWord &word) { return word.given ? ", \"thr_method\": \"" + word.text + "\"" : std::string(); }
std::string thr_method_swc(const ThrWord &word) { return word.given ? ",thr_method:" + word.text : std::string(); }

// the volume as it would be traced: windowed to 8 bits, pre-filtered, then --fill-holes / --hmax / --hdome and --local-threshold (never despeckled)
static bool set_traced_volume(pnr_ctx *ctx, const Stack &st, std::vector<MorphStage> *stages = nullptr)
{
    const Settings &S = settings();
    bool ok = (st.bits == 16 ? pnr_set_volume_u16(ctx, st.samples16(), st.w, st.h, st.l, 1, 0, S.windowed ? &S.window : nullptr, nullptr, nullptr)
                             : pnr_set_volume(ctx, st.bytes(), st.w, st.h, st.l)) == PNR_OK;
    if (ok && (S.filter.median || S.filter.tophat_r)) ok = pnr_filter_volume(ctx, &S.filter) == PNR_OK;
    if (ok && S.morph()) ok = morph_stages(ctx, stages);
    if (ok) ok = local_stage(ctx, nullptr);
    return ok || lib_fail("volume");
}

// the JSON value of a voxel index in a stack of w x h pixels per plane: [x, y, z], or null for none
static void print_max_at(int64_t first_max, long long w, long long h)
{
    if (first_max < 0) printf("null");
    else printf("[%lld, %lld, %lld]", (long long)(first_max % w), (long long)(first_max / w % h), (long long)(first_max / (w * h)));
}

bool print_tree_distance(const std::string &a, const std::string &b, const pnr_distance_opts &opts, int device, const std::string &per_node)
{
    SwcTree A, B;
    if (!read_swc(a, A) || !read_swc(b, B)) return false;
    for (const auto &side : {std::make_pair(&a, &A), std::make_pair(&b, &B)})
        if (side.second->n() == 0) {
            fprintf(stderr, "%s: no nodes\n", side.first->c_str());
            return false;
        }
    // the sample points of either side first: the sizes of the per-point arrays (and an empty or malformed tree before any GPU work)
    int64_t na = 0, nb = 0;
    if (pnr_tree_sample(A.xyz.data(), A.parent.data(), A.n(), opts.zscale, opts.step, nullptr, nullptr, 0, &na) != PNR_OK) return lib_fail(a.c_str());
    if (pnr_tree_sample(B.xyz.data(), B.parent.data(), B.n(), opts.zscale, opts.step, nullptr, nullptr, 0, &nb) != PNR_OK) return lib_fail(b.c_str());
    pnr_params p;
    pnr_default_params(&p);
    Ctx ctx;
    if (!ctx.create(p, device)) return false;
    std::vector<float> da((size_t)na), db((size_t)nb);
    std::vector<int32_t> oa((size_t)na), ob((size_t)nb);
    pnr_distance_result r;
    if (pnr_tree_distance(ctx, A.xyz.data(), A.parent.data(), A.n(), B.xyz.data(), B.parent.data(), B.n(), &opts, &r, da.data(), oa.data(), na, db.data(), ob.data(),
                          nb) != PNR_OK)
        return lib_fail("pnr_tree_distance");
    auto csv = [&](const char *tag, const SwcTree &t, const std::vector<float> &d, const std::vector<int32_t> &o) {
        return write_file(per_node + tag, "w", [&](FILE *f) {
            fprintf(f, "id,d\n");
            for (size_t k = 0; k < d.size(); k++) fprintf(f, "%lld,%.9g\n", t.id[(size_t)o[k]], (double)d[k]);
        });
    };
    if (!per_node.empty() && (!csv("_ab.csv", A, da, oa) || !csv("_ba.csv", B, db, ob))) return false;
    auto dir = [](const char *k, const pnr_distance_dir &d) {
        printf("\"%s\": {\"n\": %lld, \"n_big\": %lld, \"mean\": %.17g, \"ssd\": %.17g, \"pct\": %.17g, \"max\": %.17g}, ", k, (long long)d.n, (long long)d.n_big, d.mean,
               d.ssd, d.pct, d.max);
    };
    printf("{\"zscale\": %.9g, \"step\": %.9g, \"thr\": %.9g, \"nodes_a\": %lld, \"nodes_b\": %lld, ", (double)opts.zscale, (double)opts.step, (double)opts.thr, A.n(), B.n());
    dir("ab", r.ab);
    dir("ba", r.ba);
    printf("\"sd\": %.17g, \"ssd\": %.17g, \"pct\": %.17g, \"hausdorff\": %.17g}\n", r.sd, r.ssd, r.pct, r.hausdorff);
    return true;
}

bool join_swc_file(const std::string &in, const std::string &out, float gap, float zscale, long long root_id, bool keep_largest, int device)
{
    SwcTree T;
    if (!read_swc(in, T)) return false;
    const int64_t n = T.n();
    if (n == 0) {
        fprintf(stderr, "%s: no nodes\n", in.c_str());
        return false;
    }
    int64_t root = -1;
    if (root_id > 0) {
        const auto it = std::find(T.id.begin(), T.id.end(), root_id);
        if (it == T.id.end()) {
            fprintf(stderr, "--join-root %lld: %s has no node with this id\n", root_id, in.c_str());
            return false;
        }
        root = it - T.id.begin();
    }
    pnr_params p;
    pnr_default_params(&p);
    Ctx ctx;
    if (!ctx.create(p, device)) return false;
    const pnr_join_opts jo = {zscale, gap, (int32_t)root};
    std::vector<int32_t> par_out((size_t)n), order((size_t)n), comp((size_t)n);
    std::vector<pnr_bridge> bridges((size_t)n);
    int64_t nb = 0, t_in = 0, t_out = 0, rounds = 0;
    const int rc = pnr_join_trees(ctx, T.xyz.data(), T.parent.data(), n, &jo, par_out.data(), order.data(), comp.data(), bridges.data(), n, &nb, &t_in, &t_out);
    pnr_get_option(ctx, "join_rounds", &rounds);
    if (rc != PNR_OK) return lib_fail("pnr_join_trees");
    int64_t written = 0;
    if (!write_file(out, "w", [&](FILE *f) {
            fprintf(f, "#join=gap:%s,bridges:%lld,trees:%lld->%lld\n##n,type,x,y,z,radius,parent\n", f32_text(gap).c_str(), (long long)nb, (long long)t_in, (long long)t_out);
            std::vector<int64_t> pos((size_t)n, -1);
            for (int64_t k = 0; k < n; k++) {
                const size_t v = (size_t)order[(size_t)k];
                if (keep_largest && comp[v] != 0) break;
                pos[v] = ++written;
                fprintf(f, "%lld %d %s %s %s %s %lld\n", (long long)written, T.type[v], f32_text(T.xyz[3 * v]).c_str(), f32_text(T.xyz[3 * v + 1]).c_str(),
                        f32_text(T.xyz[3 * v + 2]).c_str(), f32_text(T.radius[v]).c_str(), par_out[v] < 0 ? -1LL : (long long)pos[(size_t)par_out[v]]);
            }
        }))
        return false;
    printf("{\"nodes\": %lld, \"trees_in\": %lld, \"trees_out\": %lld, \"bridges\": %lld, \"longest_bridge\": %.9g, \"rounds\": %lld}\n", (long long)written,
           (long long)t_in, (long long)t_out, (long long)nb, nb ? (double)bridges[(size_t)nb - 1].d : 0.0, (long long)rounds);
    return true;
}

std::string prune_comment(const pnr_prune_opts &opts, const pnr_prune_info &info)
{
    return "#prune=length:" + f32_text(opts.min_length) + ",radius:" + f32_text(opts.radius_factor) + ",min_tree:" + f32_text(opts.min_tree) + ",removed:" +
           std::to_string((long long)info.n_removed) + ",segments:" + std::to_string((long long)info.n_removed_segments);
}

bool prune_swc_file(const std::string &in, const std::string &out, const pnr_prune_opts &opts, const std::string &per_node, int device)
{
    SwcTree T;
    if (!read_swc(in, T)) return false;
    const int64_t n = T.n();
    if (n == 0) {
        fprintf(stderr, "%s: no nodes\n", in.c_str());
        return false;
    }
    pnr_params p;
    pnr_default_params(&p);
    Ctx ctx;
    if (!ctx.create(p, device)) return false;
    std::vector<uint8_t> keep((size_t)n);
    std::vector<uint32_t> height((size_t)n), path((size_t)n);
    std::vector<int32_t> order((size_t)n), seg((size_t)n), idx((size_t)n), par((size_t)n);
    pnr_prune_info pi = {};
    int64_t m = 0;
    if (pnr_prune_tree(ctx, T.xyz.data(), T.radius.data(), T.parent.data(), n, &opts, &pi, keep.data(), height.data(), path.data(), order.data(), seg.data()) != PNR_OK)
        return lib_fail("pnr_prune_tree");
    if (pnr_prune_apply(T.parent.data(), keep.data(), n, idx.data(), par.data(), &m) != PNR_OK) return lib_fail("pnr_prune_apply");
    if (!out.empty() && !write_file(out, "w", [&](FILE *f) {
            fprintf(f, "##n,type,x,y,z,radius,parent\n%s\n", prune_comment(opts, pi).c_str());
            for (size_t v = 0; v < (size_t)n; v++)
                if (keep[v])
                    fprintf(f, "%lld %d %s %s %s %s %lld\n", (long long)idx[v] + 1, T.type[v], f32_text(T.xyz[3 * v]).c_str(), f32_text(T.xyz[3 * v + 1]).c_str(),
                            f32_text(T.xyz[3 * v + 2]).c_str(), f32_text(T.radius[v]).c_str(), par[(size_t)idx[v]] < 0 ? -1LL : (long long)par[(size_t)idx[v]] + 1);
        }))
        return false;
    if (!per_node.empty() && !write_file(per_node, "w", [&](FILE *f) {
            fprintf(f, "id,keep,height,path,order,seg_id\n");
            for (size_t v = 0; v < (size_t)n; v++)
                fprintf(f, "%lld,%d,%.17g,%.17g,%d,%lld\n", T.id[v], (int)keep[v], height[v] / 256.0, path[v] / 256.0, (int)order[v], T.id[(size_t)seg[v]]);
        }))
        return false;
    printf("{\"nodes\": %lld, \"nodes_out\": %lld, \"zscale\": %.9g, \"min_length\": %.9g, \"radius_factor\": %.9g, \"min_tree\": %.9g, \"n_roots\": %lld, \"n_leaves\": %lld, "
           "\"n_branch\": %lld, \"n_segments\": %lld, \"n_removed\": %lld, \"n_removed_segments\": %lld, \"n_removed_trees\": %lld, \"length_in\": %.17g, \"length_out\": %.17g, "
           "\"h_max\": %.17g, \"order_max\": %d, \"rounds_up\": %d, \"rounds_down\": %d}\n",
           (long long)pi.n, (long long)m, (double)opts.zscale, (double)opts.min_length, (double)opts.radius_factor, (double)opts.min_tree, (long long)pi.n_roots, (long long)pi.n_leaves,
           (long long)pi.n_branch, (long long)pi.n_segments, (long long)pi.n_removed, (long long)pi.n_removed_segments, (long long)pi.n_removed_trees, (double)pi.length_in / 256.0,
           (double)pi.length_out / 256.0, pi.h_max / 256.0, (int)pi.order_max, (int)pi.rounds_up, (int)pi.rounds_down);
    return true;
}

bool geodesic_join(pnr_ctx *ctx, const float *xyz, const int32_t *parent, int64_t n, const pnr_geojoin_opts &opts, int64_t root, long long w, long long h, long long l,
                   GeoJoined &out)
{
    std::vector<int64_t> vox;
    int64_t nb = 0, np = 0;
    for (;;) { // "*n_bridges > cap_bridges or *n_path > cap_path: call again"
        const int64_t cap_b = (int64_t)out.bridges.size(), cap_p = (int64_t)vox.size();
        if (pnr_geodesic_bridges(ctx, xyz, parent, n, &opts, &out.info, out.bridges.data(), cap_b, &nb, vox.data(), cap_p, &np) != PNR_OK) return lib_fail("pnr_geodesic_bridges");
        if (nb <= cap_b && np <= cap_p) break;
        out.bridges.resize((size_t)nb), vox.resize((size_t)np);
    }
    out.bridges.resize((size_t)nb);
    int64_t n2 = 0;
    std::vector<pnr_bridge> join((size_t)nb);
    if (pnr_join_expand(xyz, parent, n, out.bridges.data(), nb, vox.data(), np, w, h, l, nullptr, nullptr, nullptr, 0, &n2, nullptr) != PNR_OK) return lib_fail("pnr_join_expand");
    std::vector<int32_t> par((size_t)n2);
    out.xyz.resize((size_t)n2 * 3), out.bridge_of.resize((size_t)(n2 - n));
    out.par_out.resize((size_t)n2), out.order.resize((size_t)n2), out.comp.resize((size_t)n2);
    if (pnr_join_expand(xyz, parent, n, out.bridges.data(), nb, vox.data(), np, w, h, l, out.xyz.data(), par.data(), out.bridge_of.data(), n2, &n2, join.data()) != PNR_OK)
        return lib_fail("pnr_join_expand");
    if (pnr_join_reroot(par.data(), n2, join.data(), nb, root, out.par_out.data(), out.order.data(), out.comp.data()) != PNR_OK) return lib_fail("pnr_join_reroot");
    return true;
}

bool join_swc_geodesic_file(const std::string &in, const std::string &out, const pnr_geojoin_opts &opts, const std::vector<char *> &infiles, const std::string &raw_dims,
                            float zscale, long long root_id, bool keep_largest, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    SwcTree T;
    if (!read_swc(in, T)) return false;
    const int64_t n = T.n();
    if (n == 0) {
        fprintf(stderr, "%s: no nodes\n", in.c_str());
        return false;
    }
    int64_t root = -1;
    if (root_id > 0) {
        const auto it = std::find(T.id.begin(), T.id.end(), root_id);
        if (it == T.id.end()) {
            fprintf(stderr, "--join-root %lld: %s has no node with this id\n", root_id, in.c_str());
            return false;
        }
        root = it - T.id.begin();
    }
    pnr_params p;
    pnr_default_params(&p);
    p.zdist = zscale; // (also the z half-width of --subtract-background)
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().join_word;
    pnr_geojoin_opts jo = opts;
    if (!resolve_threshold(ctx, word, jo.thr)) return false;
    GeoJoined J;
    if (!geodesic_join(ctx, T.xyz.data(), T.parent.data(), n, jo, root, st.w, st.h, st.l, J)) return false;
    const pnr_geojoin_info &gi = J.info;
    int64_t written = 0;
    if (!write_file(out, "w", [&](FILE *f) {
            fprintf(f, "#join=geodesic:%llu,thr:%d,bridges:%lld,trees:%lld->%lld,inserted:%lld%s\n##n,type,x,y,z,radius,parent\n", (unsigned long long)opts.limit, (int)gi.thr_used,
                    (long long)gi.n_bridges, (long long)gi.n_trees_in, (long long)gi.n_trees_out, (long long)gi.n_inserted, thr_method_swc(word).c_str());
            std::vector<int64_t> pos((size_t)J.n2(), -1);
            for (int64_t k = 0; k < J.n2(); k++) {
                const size_t v = (size_t)J.order[(size_t)k];
                if (keep_largest && J.comp[v] != 0) break;
                pos[v] = ++written;
                // an inserted node: the type of its bridge's node a, the smaller radius of a and b
                const pnr_geo_bridge *b = (int64_t)v >= n ? &J.bridges[(size_t)J.bridge_of[v - (size_t)n]] : nullptr;
                const int type = T.type[b ? (size_t)b->a : v];
                const float radius = b ? std::min(T.radius[(size_t)b->a], T.radius[(size_t)b->b]) : T.radius[v];
                fprintf(f, "%lld %d %s %s %s %s %lld\n", (long long)written, type, f32_text(J.xyz[3 * v]).c_str(), f32_text(J.xyz[3 * v + 1]).c_str(),
                        f32_text(J.xyz[3 * v + 2]).c_str(), f32_text(radius).c_str(), J.par_out[v] < 0 ? -1LL : (long long)pos[(size_t)J.par_out[v]]);
            }
        }))
        return false;
    printf("{\"nodes\": %lld, \"n_trees_in\": %lld, \"n_trees_lost\": %lld, \"n_trees_out\": %lld, \"n_bridges\": %lld, \"n_inserted\": %lld, \"w_max\": %llu, \"thr_used\": %d, "
           "\"n_src\": %lld, \"n_src_dropped\": %lld, \"limit\": %llu, \"zdist\": %.17g, \"rounds\": %d%s}\n",
           (long long)written, (long long)gi.n_trees_in, (long long)gi.n_trees_lost, (long long)gi.n_trees_out, (long long)gi.n_bridges, (long long)gi.n_inserted,
           (unsigned long long)gi.w_max, (int)gi.thr_used, (long long)gi.n_src, (long long)gi.n_src_dropped, (unsigned long long)opts.limit, (double)zscale, (int)gi.rounds, thr_method_json(word).c_str());
    return true;
}

// --render-swc without -i: the mask alone, on the grid of -d
static bool render_mask_on_grid(const RenderJob &job, const SwcTree &T, const pnr_params &p, const std::string &raw_dims, int device)
{
    long long w = 0, h = 0, l = 0;
    if (sscanf(raw_dims.c_str(), "%lld,%lld,%lld", &w, &h, &l) != 3 || w <= 0 || h <= 0 || l <= 0) {
        fprintf(stderr, "--render-swc without -i needs the grid: -d w,h,l\n");
        return false;
    }
    std::string e;
    if (job.mask.size() > 4 && job.mask.substr(job.mask.size() - 4) != ".raw" && tiff_u8_bytes(w, h, l) < 0 && !save_stack_u8(job.mask, nullptr, w, h, l, e)) {
        fprintf(stderr, "%s\n", e.c_str()); // (refused from the dimensions, before any GPU work)
        return false;
    }
    Ctx ctx;
    if (!ctx.create(p, device)) return false;
    std::vector<unsigned char> mask((size_t)(w * h * l));
    int64_t items = 0;
    const int rc = pnr_render_tree(ctx, T.xyz.data(), T.radius.data(), T.parent.data(), T.n(), w, h, l, &job.opts, nullptr, mask.data());
    pnr_get_option(ctx, "render_items", &items);
    if (rc != PNR_OK) return lib_fail("pnr_render_tree");
    if (!write_stack(job.mask, mask.data(), w, h, l)) return false;
    long long n_tree = 0;
    for (unsigned char v : mask) n_tree += v != 0;
    printf("{\"n_vox\": %lld, \"n_tree\": %lld, \"nodes\": %lld, \"items\": %lld}\n", w * h * l, n_tree, T.n(), (long long)items);
    return true;
}

bool render_swc_file(const RenderJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, int device)
{
    SwcTree T;
    if (!read_swc(job.swc, T)) return false;
    const int64_t n = T.n();
    pnr_params p;
    pnr_default_params(&p);
    if (job.opts.zscale >= 1.f) p.zdist = job.opts.zscale; // (the z half-width of --subtract-background)
    if (infiles.empty()) return render_mask_on_grid(job, T, p, raw_dims, device);
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().coverage_word;
    pnr_render_opts ro = job.opts;
    if (!resolve_threshold(ctx, word, ro.thr)) return false;
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<unsigned char> mask(job.mask.empty() ? 0 : N), residual(job.residual.empty() ? 0 : N);
    std::vector<int64_t> vox, fg, sum;
    if (!job.per_node.empty()) vox.assign((size_t)n, 0), fg.assign((size_t)n, 0), sum.assign((size_t)n, 0);
    pnr_coverage c;
    int64_t items = 0;
    const int rc = pnr_tree_coverage(ctx, T.xyz.data(), T.radius.data(), T.parent.data(), n, &ro, &c, job.per_node.empty() ? nullptr : vox.data(),
                                     job.per_node.empty() ? nullptr : fg.data(), job.per_node.empty() ? nullptr : sum.data(),
                                     job.mask.empty() ? nullptr : mask.data(), job.residual.empty() ? nullptr : residual.data());
    pnr_get_option(ctx, "render_items", &items);
    if (rc != PNR_OK) return lib_fail("pnr_tree_coverage");
    if (!job.mask.empty() && !write_stack(job.mask, mask.data(), st.w, st.h, st.l)) return false;
    if (!job.residual.empty() && !write_stack(job.residual, residual.data(), st.w, st.h, st.l)) return false;
    if (!job.per_node.empty() && !write_file(job.per_node, "w", [&](FILE *f) {
            fprintf(f, "id,vox,fg,sum\n");
            for (size_t k = 0; k < (size_t)n; k++) fprintf(f, "%lld,%lld,%lld,%lld\n", T.id[k], (long long)vox[k], (long long)fg[k], (long long)sum[k]);
        }))
        return false;
    printf("{\"n_vox\": %lld, \"n_tree\": %lld, \"n_fg\": %lld, \"n_both\": %lld, \"sum_fg\": %lld, \"sum_both\": %lld, \"thr_used\": %d, \"covered\": %.17g, "
           "\"on_signal\": %.17g, \"covered_intensity\": %.17g, \"nodes\": %lld, \"items\": %lld%s}\n",
           (long long)c.n_vox, (long long)c.n_tree, (long long)c.n_fg, (long long)c.n_both, (long long)c.sum_fg, (long long)c.sum_both, (int)c.thr_used, c.covered,
           c.on_signal, c.covered_intensity, (long long)n, (long long)items, thr_method_json(word).c_str());
    return true;
}

bool components_file(const ComponentsJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    pnr_params p;
    pnr_default_params(&p);
    if (zscale >= 1.f) p.zdist = zscale; // (the z half-width of --subtract-background)
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().thr_word;
    pnr_components_opts co = job.opts;
    if (!resolve_threshold(ctx, word, co.thr)) return false;
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<int32_t> labels(job.labels.empty() ? 0 : N);
    std::vector<pnr_component> comps;
    pnr_components_info ci = {};
    int rc = pnr_label_components(ctx, &co, &ci, job.labels.empty() ? nullptr : labels.data(), nullptr, 0);
    if (rc == PNR_OK && !job.per_component.empty() && ci.n_comp > 0) { // "n_comp > cap: call again"
        comps.resize((size_t)ci.n_comp);
        rc = pnr_label_components(ctx, &co, &ci, nullptr, comps.data(), (int64_t)comps.size());
    }
    if (rc != PNR_OK) return lib_fail("pnr_label_components");
    if (!job.labels.empty() && !write_file(job.labels, "wb", [&](FILE *f) { fwrite(labels.data(), 4, N, f); })) return false; // (the hosts this builds for are little-endian)
    if (!job.per_component.empty() && !write_file(job.per_component, "w", [&](FILE *f) {
            fprintf(f, "id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax\n");
            for (size_t k = 0; k < comps.size(); k++) {
                const pnr_component &c = comps[k];
                fprintf(f, "%lld,%lld,%lld,%.3f,%.3f,%.3f,%d,%d,%d,%d,%d,%d,%d\n", (long long)(k + 1), (long long)c.size, (long long)c.sum, (double)c.sx / (double)c.size,
                        (double)c.sy / (double)c.size, (double)c.sz / (double)c.size, c.x0, c.y0, c.z0, c.x1, c.y1, c.z1, c.vmax);
            }
        }))
        return false;
    printf("{\"n_vox\": %lld, \"n_fg\": %lld, \"n_comp\": %lld, \"n_small\": %lld, \"vox_small\": %lld, \"largest\": %lld, \"thr_used\": %d%s}\n", (long long)ci.n_vox,
           (long long)ci.n_fg, (long long)ci.n_comp, (long long)ci.n_small, (long long)ci.vox_small, (long long)ci.largest, (int)ci.thr_used, thr_method_json(word).c_str());
    return true;
}

bool edt_file(const EdtJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    SwcTree T;
    if (!job.at.empty() && !read_swc(job.at, T)) return false;
    pnr_params p;
    pnr_default_params(&p);
    p.zdist = zscale; // (also the z half-width of --subtract-background)
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().thr_word;
    pnr_edt_opts eo = job.opts;
    if (!resolve_threshold(ctx, word, eo.thr)) return false;
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<float> d(job.out.empty() ? 0 : N), at((size_t)T.n());
    pnr_edt_info ei = {};
    if (pnr_distance_transform(ctx, &eo, &ei, job.out.empty() ? nullptr : d.data(), T.n() ? T.xyz.data() : nullptr, T.n(), T.n() ? at.data() : nullptr) != PNR_OK)
        return lib_fail("pnr_distance_transform");
    for (float &v : d) v = sqrtf(v);
    if (!job.out.empty() && !write_file(job.out, "wb", [&](FILE *f) { fwrite(d.data(), 4, N, f); })) return false; // (the hosts this builds for are little-endian)
    if (!job.per_node.empty() && !write_file(job.per_node, "w", [&](FILE *f) {
            fprintf(f, "id,d\n");
            for (size_t k = 0; k < at.size(); k++) fprintf(f, "%lld,%.9g\n", T.id[k], (double)(at[k] < 0.f ? -1.f : sqrtf(at[k])));
        }))
        return false;
    printf("{\"n_vox\": %lld, \"n_fg\": %lld, \"n_capped\": %lld, \"thr_used\": %d, \"rmax\": %d, \"zdist\": %.17g, \"d_max\": %.17g, \"max_at\": ", (long long)ei.n_vox,
           (long long)ei.n_fg, (long long)ei.n_capped, (int)ei.thr_used, (int)job.opts.rmax, (double)zscale, (double)sqrtf(ei.d2_max));
    print_max_at(ei.first_max, st.w, st.h);
    printf("%s}\n", thr_method_json(word).c_str());
    return true;
}

bool skeleton_file(const SkeletonJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    pnr_params p;
    pnr_default_params(&p);
    p.zdist = zscale; // (the radii of --swc; also the z half-width of --subtract-background)
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().thr_word;
    pnr_thin_opts to = job.opts;
    if (!resolve_threshold(ctx, word, to.thr)) return false;
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<unsigned char> skel(job.out.empty() ? 0 : N);
    pnr_thin_info ti = {};
    if (pnr_skeletonize(ctx, &to, &ti, nullptr, nullptr, nullptr, 0) != PNR_OK) return lib_fail("pnr_skeletonize"); // "n_skel > cap: call again"
    const int64_t n = ti.n_skel;
    std::vector<int64_t> vox((size_t)n);
    std::vector<uint8_t> deg((size_t)n);
    if ((n > 0 || !job.out.empty()) && pnr_skeletonize(ctx, &to, &ti, job.out.empty() ? nullptr : skel.data(), vox.data(), deg.data(), n) != PNR_OK)
        return lib_fail("pnr_skeletonize");
    std::vector<pnr_bridge> edges((size_t)std::max<int64_t>(n - 1, 0));
    int64_t ne = 0;
    if (pnr_skeleton_forest(vox.data(), n, st.w, st.h, st.l, edges.data(), (int64_t)edges.size(), &ne) != PNR_OK) return lib_fail("pnr_skeleton_forest");
    const int64_t trees = n - ne;
    if (!job.swc.empty()) {
        std::vector<float> xyz((size_t)n * 3), d2((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t v = vox[(size_t)i];
            xyz[(size_t)(3 * i)] = (float)(v % st.w), xyz[(size_t)(3 * i + 1)] = (float)(v / st.w % st.h), xyz[(size_t)(3 * i + 2)] = (float)(v / (st.w * st.h));
        }
        std::vector<int32_t> par((size_t)n, -1), par_out((size_t)n), order((size_t)n), comp((size_t)n);
        if (n > 0) {
            const pnr_edt_opts eo = {ti.thr_used, 64};
            if (pnr_distance_transform(ctx, &eo, nullptr, nullptr, xyz.data(), n, d2.data()) != PNR_OK) return lib_fail("pnr_distance_transform");
            const int64_t root = std::max_element(d2.begin(), d2.end()) - d2.begin(); // (the first of the largest: the soma guess of --edt)
            if (pnr_join_reroot(par.data(), n, edges.data(), ne, root, par_out.data(), order.data(), comp.data()) != PNR_OK) return lib_fail("pnr_join_reroot");
        }
        // --prune: the radius column as it is written, then the rule on the nodes in voxel order; a removed node is not written
        std::vector<uint8_t> keep((size_t)n, 1);
        pnr_prune_opts po = job.prune_opts;
        po.zscale = zscale;
        pnr_prune_info pi = {};
        if (job.prune && n > 0) {
            std::vector<float> rad((size_t)n);
            for (int64_t i = 0; i < n; i++) rad[(size_t)i] = sqrtf(d2[(size_t)i]);
            if (pnr_prune_tree(ctx, xyz.data(), rad.data(), par_out.data(), n, &po, &pi, keep.data(), nullptr, nullptr, nullptr, nullptr) != PNR_OK) return lib_fail("pnr_prune_tree");
        }
        if (!write_file(job.swc, "w", [&](FILE *f) {
                fprintf(f, "##n,type,x,y,z,radius,parent\n#skeleton=thr:%d,rounds:%d,voxels:%lld,trees:%lld%s\n", (int)ti.thr_used, (int)ti.rounds, (long long)n, (long long)trees,
                        thr_method_swc(word).c_str());
                if (job.prune) fprintf(f, "%s\n", prune_comment(po, pi).c_str());
                std::vector<int64_t> pos((size_t)n, -1);
                int64_t written = 0;
                for (int64_t k = 0; k < n; k++) {
                    const size_t v = (size_t)order[(size_t)k];
                    if (!keep[v]) continue;
                    pos[v] = ++written;
                    fprintf(f, "%lld 2 %s %s %s %s %lld\n", (long long)written, f32_text(xyz[3 * v]).c_str(), f32_text(xyz[3 * v + 1]).c_str(), f32_text(xyz[3 * v + 2]).c_str(),
                            f32_text(sqrtf(d2[v])).c_str(), par_out[v] < 0 ? -1LL : (long long)pos[(size_t)par_out[v]]);
                }
            }))
            return false;
    }
    if (!job.out.empty() && !write_stack(job.out, skel.data(), st.w, st.h, st.l)) return false;
    printf("{\"n_vox\": %lld, \"n_fg\": %lld, \"n_skel\": %lld, \"n_end\": %lld, \"n_branch\": %lld, \"n_isolated\": %lld, \"tiles\": %lld, \"tile_visits\": %lld, "
           "\"rounds\": %d, \"thr_used\": %d, \"trees\": %lld%s}\n",
           (long long)ti.n_vox, (long long)ti.n_fg, (long long)ti.n_skel, (long long)ti.n_end, (long long)ti.n_branch, (long long)ti.n_isolated, (long long)ti.tiles,
           (long long)ti.tile_visits, (int)ti.rounds, (int)ti.thr_used, (long long)trees, thr_method_json(word).c_str());
    return true;
}

bool morph_file(const std::string &out, const std::vector<char *> &infiles, const std::string &raw_dims, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    pnr_params p;
    pnr_default_params(&p);
    Ctx ctx;
    std::vector<MorphStage> stages;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st, &stages)) return false;
    std::vector<unsigned char> vol((size_t)(st.w * st.h * st.l));
    if (pnr_get_volume(ctx, vol.data()) != PNR_OK) return lib_fail("pnr_get_volume");
    if (!write_stack(out, vol.data(), st.w, st.h, st.l)) return false;
    printf("{\"w\": %lld, \"h\": %lld, \"l\": %lld, \"stages\": [", st.w, st.h, st.l);
    for (size_t k = 0; k < stages.size(); k++) {
        const pnr_morph_info &mi = stages[k].info;
        printf("%s{\"op\": \"%s\", \"h\": %d, \"n_vox\": %lld, \"n_changed\": %lld, \"n_nonzero\": %lld, \"sum_in\": %llu, \"sum_out\": %llu, \"max_delta\": %d, "
               "\"connectivity\": %d, \"tiles\": %lld, \"tile_visits\": %lld, \"rounds\": %d}",
               k ? ", " : "", stages[k].op, stages[k].h, (long long)mi.n_vox, (long long)mi.n_changed, (long long)mi.n_nonzero, (unsigned long long)mi.sum_in,
               (unsigned long long)mi.sum_out, (int)mi.max_delta, (int)mi.connectivity, (long long)mi.tiles, (long long)mi.tile_visits, (int)mi.rounds);
    }
    printf("]}\n");
    return true;
}

// `count` elements of T from the file `name`, which holds exactly those: false after a message on stderr
template <typename T>
static bool read_volume_file(const std::string &name, size_t count, std::vector<T> &out, const char *what)
{
    FILE *f = fopen(name.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "%s: cannot read the file\n", name.c_str());
        return false;
    }
    out.resize(count + 1);
    const size_t got = fread(out.data(), sizeof(T), count + 1, f);
    const bool bad = ferror(f) != 0 || got != count || !feof(f);
    fclose(f);
    out.resize(count);
    if (bad) fprintf(stderr, "%s: not %s of this stack (%zu values of %zu bytes)\n", name.c_str(), what, count, sizeof(T));
    return !bad;
}

bool watershed_file(const WatershedJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    const size_t N = (size_t)(st.w * st.h * st.l);
    SwcTree T;
    std::vector<int32_t> label, mvol;
    std::vector<uint8_t> relief;
    if (!job.markers_swc.empty()) {
        if (!read_swc(job.markers_swc, T)) return false;
        const int64_t n = T.n();
        if (n == 0) {
            fprintf(stderr, "%s: no nodes\n", job.markers_swc.c_str());
            return false;
        }
        label.resize((size_t)n);
        if (job.by_node) {
            for (int64_t i = 0; i < n; i++) {
                if (T.id[(size_t)i] < 1 || T.id[(size_t)i] > 0x7fffffffLL) {
                    fprintf(stderr, "%s: node id %lld is no label (1 .. 2147483647)\n", job.markers_swc.c_str(), T.id[(size_t)i]);
                    return false;
                }
                label[(size_t)i] = (int32_t)T.id[(size_t)i];
            }
        } else { // the trees as pnr_join_reroot numbers them: by descending node count, ties by ascending root index
            if (pnr_join_reroot(T.parent.data(), n, nullptr, 0, -1, nullptr, nullptr, label.data()) != PNR_OK) return lib_fail(job.markers_swc.c_str());
            for (int32_t &v : label) v += 1;
        }
    } else if (!read_volume_file(job.markers_raw, N, mvol, "the int32 marker volume"))
        return false;
    if (!job.relief.empty() && !read_volume_file(job.relief, N, relief, "the relief")) return false;
    pnr_params p;
    pnr_default_params(&p);
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().thr_word;
    pnr_watershed_opts wo = job.opts;
    if (!resolve_threshold(ctx, word, wo.thr)) return false;
    std::vector<int32_t> L(N);
    std::vector<uint8_t> M(job.levels.empty() ? 0 : N);
    pnr_watershed_info wi = {};
    const bool points = mvol.empty();
    if (pnr_watershed(ctx, &wo, relief.empty() ? nullptr : relief.data(), points ? nullptr : mvol.data(), points ? T.xyz.data() : nullptr,
                      points ? label.data() : nullptr, points ? T.n() : 0, &wi, L.data(), M.empty() ? nullptr : M.data()) != PNR_OK)
        return lib_fail("pnr_watershed");
    // (the hosts this builds for are little-endian)
    if (!write_file(job.labels, "wb", [&](FILE *f) { fwrite(L.data(), 4, N, f); })) return false;
    if (!job.levels.empty() && !write_file(job.levels, "wb", [&](FILE *f) { fwrite(M.data(), 1, N, f); })) return false;
    printf("{\"w\": %lld, \"h\": %lld, \"l\": %lld, \"markers_by\": \"%s\", \"n_markers\": %lld, \"n_vox\": %lld, \"n_mask\": %lld, \"n_marker_vox\": %lld, "
           "\"n_dropped\": %lld, \"n_reached\": %lld, \"n_unreached\": %lld, \"n_regions\": %lld, \"m_max\": %d, \"d_max\": %d, \"thr_used\": %d, "
           "\"connectivity\": %d, \"tiles\": %lld, \"flood_visits\": %lld, \"label_visits\": %lld, \"flood_rounds\": %d, \"label_rounds\": %d%s}\n",
           (long long)st.w, (long long)st.h, (long long)st.l, !points ? "volume" : job.by_node ? "node" : "tree", points ? (long long)T.n() : (long long)wi.n_marker_vox + wi.n_dropped,
           (long long)wi.n_vox, (long long)wi.n_mask, (long long)wi.n_marker_vox, (long long)wi.n_dropped, (long long)wi.n_reached, (long long)wi.n_unreached,
           (long long)wi.n_regions, (int)wi.m_max, (int)wi.d_max, (int)wi.thr_used, (int)wi.connectivity, (long long)wi.tiles, (long long)wi.flood_visits,
           (long long)wi.label_visits, (int)wi.flood_rounds, (int)wi.label_rounds, thr_method_json(word).c_str());
    return true;
}

// the sources of --geodesic: the sample points of the tree (step 1, zscale 1), each labelled with the id of its owner node
static bool geodesic_sources(const std::string &from, const SwcTree &A, std::vector<float> &src, std::vector<int32_t> &label)
{
    if (A.n() == 0) {
        fprintf(stderr, "%s: no nodes\n", from.c_str());
        return false;
    }
    for (long long id : A.id)
        if (id < 0 || id > 0x7fffffffLL) {
            fprintf(stderr, "%s: node id %lld is no label (0 .. 2147483647)\n", from.c_str(), id);
            return false;
        }
    int64_t ns = 0;
    if (pnr_tree_sample(A.xyz.data(), A.parent.data(), A.n(), 1.f, 1.f, nullptr, nullptr, 0, &ns) != PNR_OK) return lib_fail(from.c_str());
    src.resize((size_t)ns * 3), label.resize((size_t)ns);
    if (pnr_tree_sample(A.xyz.data(), A.parent.data(), A.n(), 1.f, 1.f, src.data(), label.data(), ns, &ns) != PNR_OK) return lib_fail(from.c_str());
    for (int32_t &v : label) v = (int32_t)A.id[(size_t)v];
    return true;
}

// --paths: every complete path (plen[k] voxels, the first of the `cap` that pvox keeps per target) as a chain of SWC nodes from the
// target's voxel to the source voxel
static void write_paths(FILE *f, const SwcTree &B, const std::vector<uint32_t> &d_at, const std::vector<int32_t> &l_at, const std::vector<int32_t> &plen,
                        const std::vector<int64_t> &pvox, int32_t cap, long long w, long long h)
{
    long long next = 1;
    for (size_t k = 0; k < plen.size(); k++) {
        const int32_t n = plen[k];
        if (n <= 0) continue; // (unreached, not finite, or cut at the cap: reported on stderr)
        fprintf(f, "# path %lld -> %d: %d voxels, cost %u\n", B.id[k], (int)l_at[k], (int)n, (unsigned)d_at[k]);
        for (int32_t j = 0; j < n; j++) {
            const long long v = pvox[k * (size_t)cap + (size_t)j];
            fprintf(f, "%lld 2 %lld %lld %lld 1 %lld\n", next + j, v % w, v / w % h, v / (w * h), j + 1 < n ? next + j + 1 : -1LL);
        }
        next += n;
    }
}

bool geodesic_file(const GeodesicJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    SwcTree A, B;
    if (!read_swc(job.from, A) || (!job.to.empty() && !read_swc(job.to, B))) return false;
    std::vector<float> src;
    std::vector<int32_t> label;
    if (!geodesic_sources(job.from, A, src, label)) return false;
    pnr_params p;
    pnr_default_params(&p);
    p.zdist = zscale; // (also the z half-width of --subtract-background)
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    const ThrWord &word = settings().thr_word;
    pnr_geo_opts go = job.opts;
    if (!resolve_threshold(ctx, word, go.thr)) return false;
    const size_t N = (size_t)(st.w * st.h * st.l);
    const int64_t m = B.n();
    std::vector<uint32_t> D(job.out.empty() ? 0 : N), d_at((size_t)m);
    std::vector<int32_t> L(job.out.empty() ? 0 : N), l_at((size_t)m), plen;
    std::vector<int64_t> pvox;
    pnr_geo_info gi = {};
    // the cap of the walks, fixed before the one call: a path visits a voxel at most once, no path has more than PNR_GEO_MAX_PATH voxels, and
    // all targets together get at most 2^26 entries (512 MB here and on the device)
    int32_t cap = 0;
    if (!job.paths.empty() && m) {
        cap = (int32_t)std::min<size_t>({(size_t)PNR_GEO_MAX_PATH, N, std::max<size_t>(64, ((size_t)1 << 26) / (size_t)m)});
        plen.resize((size_t)m), pvox.resize((size_t)m * (size_t)cap);
    }
    if (pnr_geodesic_distance(ctx, src.data(), label.data(), (int64_t)label.size(), &go, &gi, job.out.empty() ? nullptr : D.data(), job.out.empty() ? nullptr : L.data(),
                              m ? B.xyz.data() : nullptr, m, m ? d_at.data() : nullptr, m ? l_at.data() : nullptr, cap, cap ? plen.data() : nullptr,
                              cap ? pvox.data() : nullptr) != PNR_OK)
        return lib_fail("pnr_geodesic_distance");
    long long cut = 0;
    for (int32_t n : plen) cut += n < 0;
    if (cut) fprintf(stderr, "--paths: %lld path(s) of more than %d voxels are left out of %s\n", cut, (int)cap, job.paths.c_str());
    if (!job.out.empty()) { // (the hosts this builds for are little-endian)
        if (!write_file(job.out + "_d.raw", "wb", [&](FILE *f) { fwrite(D.data(), 4, N, f); })) return false;
        if (!write_file(job.out + "_label.raw", "wb", [&](FILE *f) { fwrite(L.data(), 4, N, f); })) return false;
    }
    if (!job.per_node.empty() && !write_file(job.per_node, "w", [&](FILE *f) {
            fprintf(f, "id,d,label\n");
            for (size_t k = 0; k < (size_t)m; k++) fprintf(f, "%lld,%lld,%d\n", B.id[k], d_at[k] == 0xffffffffu ? -1LL : (long long)d_at[k], (int)l_at[k]);
        }))
        return false;
    if (!job.paths.empty() && !write_file(job.paths, "w", [&](FILE *f) { write_paths(f, B, d_at, l_at, plen, pvox, cap, st.w, st.h); })) return false;
    printf("{\"n_vox\": %lld, \"n_pass\": %lld, \"n_reached\": %lld, \"n_src\": %lld, \"n_src_dropped\": %lld, \"thr_used\": %d, \"dmax\": %u, \"zdist\": %.17g, \"d_max\": %u, "
           "\"len_max\": %.17g, \"max_at\": ",
           (long long)gi.n_vox, (long long)gi.n_pass, (long long)gi.n_reached, (long long)gi.n_src, (long long)gi.n_src_dropped, (int)gi.thr_used, (unsigned)job.opts.dmax,
           (double)zscale, (unsigned)gi.d_max, (double)gi.d_max / 64.0);
    print_max_at(gi.first_max, st.w, st.h);
    printf(", \"rounds\": %d%s}\n", (int)gi.rounds, thr_method_json(word).c_str());
    return true;
}

bool auto_threshold_file(int lo, const std::string &histogram, const std::vector<char *> &infiles, const std::string &raw_dims, int device)
{
    Stack st;
    if (load_input_stack(infiles[0], raw_dims, st) != Loaded::ok) return false;
    pnr_params p;
    pnr_default_params(&p);
    Ctx ctx;
    if (!ctx.create(p, device) || !set_traced_volume(ctx, st)) return false;
    uint64_t H[256];
    const pnr_threshold_opts mean = {PNR_THR_MEAN, lo, 0, 0};
    pnr_threshold_info ti = {};
    if (pnr_auto_threshold(ctx, &mean, &ti, H) != PNR_OK) return lib_fail("pnr_auto_threshold"); // the one histogram pass
    if (!histogram.empty() && !write_file(histogram, "w", [&](FILE *f) {
            fprintf(f, "v,count\n");
            for (int v = 0; v < 256; v++) fprintf(f, "%d,%llu\n", v, (unsigned long long)H[v]);
        }))
        return false;
    printf("{\"w\": %lld, \"h\": %lld, \"l\": %lld, \"n_vox\": %lld, \"lo\": %d", st.w, st.h, st.l, (long long)ti.n_vox, lo);
    const struct { const char *name; pnr_threshold_opts o; } rules[] = {{"mean", mean}, {"otsu", {PNR_THR_OTSU, lo, 0, 0}}, {"triangle", {PNR_THR_TRIANGLE, lo, 0, 0}},
                                                                        {"maxentropy", {PNR_THR_MAXENTROPY, 0, 0, 0}}, {"top1", {PNR_THR_TOP, lo, 10000, 0}}};
    for (const auto &r : rules) {
        if (pnr_threshold_from_hist(H, &r.o, &ti) == PNR_OK) printf(", \"%s\": {\"thr\": %d, \"n_fg\": %lld}", r.name, (int)ti.thr, (long long)ti.n_fg);
        else if (r.o.method == PNR_THR_MAXENTROPY) printf(", \"%s\": null", r.name); // (a bin of 2^31 voxels or more)
        else return lib_fail("pnr_threshold_from_hist");
    }
    printf("}\n");
    return true;
}

} // namespace advantra
