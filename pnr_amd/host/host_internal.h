// host_internal.h -- what the host's source files share with one another and advantra_host.h does not publish.
#pragma once
#include "advantra_host.h"
#include "stack_io.h"
#include <cstdio>
#include <vector>

namespace advantra {

// "<what>: <the library's last error>" on stderr (what = nullptr: the error alone, as the tracing run reports it); false
inline bool lib_fail(const char *what)
{
    fprintf(stderr, what ? "%s: %s\n" : "%s%s\n", what ? what : "", pnr_last_error());
    return false;
}

// save_stack_u8 with its message on stderr
inline bool write_stack(const std::string &name, const unsigned char *vol, long long w, long long h, long long l)
{
    std::string e;
    if (save_stack_u8(name, vol, w, h, l, e)) return true;
    fprintf(stderr, "%s\n", e.c_str());
    return false;
}

// a device context that ends with its scope
struct Ctx {
    pnr_ctx *raw = nullptr;
    Ctx() = default;
    Ctx(const Ctx &) = delete;
    Ctx &operator=(const Ctx &) = delete;
    ~Ctx() { if (raw) pnr_destroy(raw); }
    operator pnr_ctx *() const { return raw; }
    // false after lib_fail(what)
    bool create(const pnr_params &p, int device, const char *what = "pnr_create") { return pnr_create(&p, device, &raw) == PNR_OK || lib_fail(what); }
};

// stack_reader.cpp: load_stack with the channel and raw type of settings(), then the refusal of --window / --saturate on an 8-bit
// stack; either failure is reported on stderr
enum class Loaded { ok, unreadable, not_windowable };
Loaded load_input_stack(const std::string &path, const std::string &raw_dims, Stack &out);

// tools.cpp: the forest joined along the signal on ctx's volume -- pnr_geodesic_bridges, pnr_join_expand, then pnr_join_reroot on the
// n + inserted nodes (root: a node index, or negative for none); false after lib_fail
struct GeoJoined {
    pnr_geojoin_info info = {};
    std::vector<pnr_geo_bridge> bridges;
    std::vector<float> xyz;                    // n2 x 3: the n nodes, then the inserted ones
    std::vector<int32_t> bridge_of;            // per inserted node: its bridge
    std::vector<int32_t> par_out, order, comp; // of pnr_join_reroot, n2 entries each
    int64_t n2() const { return (int64_t)par_out.size(); }
};
bool geodesic_join(pnr_ctx *ctx, const float *xyz, const int32_t *parent, int64_t n, const pnr_geojoin_opts &opts, int64_t root, long long w, long long h, long long l,
                   GeoJoined &out);

// tools.cpp: the last steps of the volume set-up -- --fill-holes, then --hmax or --hdome of settings(), each a pnr_morph_volume on ctx's
// volume; stages (nullable) receives what ran, in order; false when a call failed (pnr_last_error has the reason)
struct MorphStage {
    const char *op; // "fill", "hmax", "hdome"
    int h;
    pnr_morph_info info;
};
bool morph_stages(pnr_ctx *ctx, std::vector<MorphStage> *stages);

// tools.cpp: --local-threshold of settings() on ctx's volume (pnr_local_threshold_volume); nothing to do without the flag; false when the
// call failed (pnr_last_error has the reason)
bool local_stage(pnr_ctx *ctx, pnr_local_info *info);
// tools.cpp: thr = the word's threshold on ctx's current volume (pnr_auto_threshold); a word that was not given leaves thr; false after lib_fail
bool resolve_threshold(pnr_ctx *ctx, const ThrWord &word, int32_t &thr);
// `, "thr_method": "<word>"` for a JSON line, `,thr_method:<word>` for an SWC comment; empty without a word
std::string thr_method_json(const ThrWord &word);
std::string thr_method_swc(const ThrWord &word);

// swc_io.cpp: load_swc with its message on stderr; the shortest decimal text without an exponent (nine digits at the most) that reads
// back as the same f32
bool read_swc(const std::string &path, SwcTree &out);
std::string f32_text(float v);

} // namespace advantra
