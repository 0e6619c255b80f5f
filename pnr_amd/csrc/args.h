// args.h -- what the extern "C" entry points (api.cpp, api_pipeline.cpp, api_tools.cpp, playback.cpp) share: one definition of every
// argument rule that more than one of them applies, with the text pnr_last_error() documents, and the copy into a caller's buffer.
// An entry point calls the rules in the order its checks run; that order decides which text wins when two arguments are bad.
#pragma once
#include "ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#define PNR_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// a capacity that is not negative, and with its buffer where it is above 0; both are named in the text as the caller names them
#define PNR_CAP_NEEDS(who, cap, buf) PNR_REQUIRE((cap) >= 0 && ((cap) == 0 || (buf)), PNR_E_ARG, "%s: " #cap " = %lld needs " #buf, who, (long long)(cap))

namespace pnr {
namespace args {

// context present, its device selected
inline int ctx_device(pnr_ctx *c)
{
    PNR_REQUIRE(c, PNR_E_ARG, "null ctx");
    PNR_HIP(hipSetDevice(c->device));
    return PNR_OK;
}
inline int thr_range(const char *who, int thr) { PNR_REQUIRE(thr >= -1 && thr <= 255, PNR_E_ARG, "%s: thr = %d outside [-1, 255]", who, thr); return PNR_OK; }
// PNR_E_STATE also without a context: the Frangi entry points have no other answer to a null context; a tool has asked for "null ctx" before
inline int volume_set(const pnr_ctx *c, const char *who) { PNR_REQUIRE(c && c->d_img, PNR_E_STATE, "%s: no volume set", who); return PNR_OK; }
// the tools that number voxels in 32 bits (0xffffffff: none): the volume, its size, then the device
inline int volume_u32(pnr_ctx *c, const char *who)
{
    PNR_TRY(volume_set(c, who));
    PNR_REQUIRE(c->N <= 0xfffffffeLL, PNR_E_ARG, "%s: %lld voxels, at most 2^32 - 2", who, (long long)c->N);
    PNR_HIP(hipSetDevice(c->device));
    return PNR_OK;
}
// the 256 entries of a cost table (NULL: the default table)
inline int cost_table(const char *who, const uint16_t *cost)
{
    for (int v = 0; cost && v < 256; v++) PNR_REQUIRE(cost[v] >= 1, PNR_E_ARG, "%s: cost[%d] = 0, every entry is at least 1", who, v);
    return PNR_OK;
}
inline int positive(const char *who, const char *field, float v) { PNR_REQUIRE(std::isfinite(v) && v > 0.f, PNR_E_ARG, "%s: %s = %g must be positive", who, field, (double)v); return PNR_OK; }
inline int not_negative(const char *who, const char *field, float v) { PNR_REQUIRE(std::isfinite(v) && v >= 0.f, PNR_E_ARG, "%s: %s = %g must not be negative", who, field, (double)v); return PNR_OK; }
inline int cap_not_negative(const char *who, int64_t cap) { PNR_REQUIRE(cap >= 0, PNR_E_ARG, "%s: cap = %lld is negative", who, (long long)cap); return PNR_OK; }
inline bool all_finite(const float *v, int64_t count)
{
    for (int64_t i = 0; i < count; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

} // namespace args

// as much of `count` records of `per` elements at src as the caller's capacity (in records) holds; out may be NULL
template <class T> void put(void *out, int64_t cap, const T *src, int64_t count, int64_t per = 1)
{
    const int64_t k = std::min(cap, count);
    if (out && k > 0) std::memcpy(out, src, sizeof(T) * (size_t)(per * k));
}
template <class T> void put(void *out, int64_t cap, const std::vector<T> &v, int64_t per = 1) { put(out, cap, v.data(), (int64_t)v.size() / per, per); }

// a node graph into the caller's buffers: the counts, and as much of either array as its capacity holds
inline int put_graph(const std::vector<pnr_node> &gn, const std::vector<int32_t> &gl, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                     int64_t *n_links)
{
    *n_nodes = (int64_t)gn.size();
    *n_links = (int64_t)gl.size() / 2;
    put(nodes, cap_nodes, gn);
    put(links, cap_links, gl, 2);
    return PNR_OK;
}

} // namespace pnr
