// threshold_rule.cpp -- the threshold rules of include/pnr_hip.h on a 256-bin histogram: mean, Otsu, triangle, brightest share and
// the reference's maximum entropy.  Pure host, integer except where the rule names doubles (Otsu's score, in the stated order; the
// build has -ffp-contract=off) and the reference's own f32 / f64 mix (maximum entropy).  No HIP call, no context: the file builds
// and runs on its own (make -C pnr_amd/csrc rule_check).
#include "threshold.h"
#include <cfloat>
#include <cmath>

namespace pnr {

// what maxentropy_from_hist asks of its counts: the rule reads a bin as the reference's `int`
int maxentropy_bins_fit(const char *who, const unsigned long long *h)
{
    for (int v = 0; v < 256; v++) PNR_REQUIRE(h[v] < (1ull << 31), PNR_E_ARG, "%s: maxentropy needs every bin below 2^31, bin %d holds %llu", who, v, h[v]);
    return PNR_OK;
}

// toolbox.cpp:657-737 on the histogram
unsigned char maxentropy_from_hist(const unsigned long long *h)
{
    float sum = 0;
    for (int i = 0; i < 256; i++) sum += (float)(int)h[i]; // `int hist[]` added into a float
    float nh[256], pT[256], hB[256], hW[256];
    for (int i = 0; i < 256; i++) nh[i] = (float)(int)h[i] / sum;
    pT[0] = nh[0];
    for (int i = 1; i < 256; i++) pT[i] = pT[i - 1] + nh[i];
    const float eps = FLT_MIN;
    for (int t = 0; t < 256; t++) {
        if (pT[t] > eps) {
            float hh = 0;
            for (int i = 0; i <= t; i++)
                if (nh[i] > eps) hh -= nh[i] / pT[t] * std::log(nh[i] / pT[t]); // float overload
            hB[t] = hh;
        } else {
            hB[t] = 0;
        }
        const double pTW = 1 - pT[t];
        if (pTW > eps) {
            float hh = 0;
            for (int i = t + 1; i < 256; i++)
                if (nh[i] > eps) hh = (float)((double)hh - nh[i] / pTW * std::log(nh[i] / pTW));
            hW[t] = hh;
        } else {
            hW[t] = 0;
        }
    }
    float jMax = hB[0] + hW[0];
    unsigned char tMax = 0;
    for (int t = 1; t < 256; t++) {
        const double j = hB[t] + hW[t];
        if (j > jMax) { jMax = (float)j; tMax = (unsigned char)t; }
    }
    return tMax;
}

namespace {

using u64 = unsigned long long;
using i64 = long long;
constexpr u64 MAX_VOX = 1ull << 45; // below it Otsu's four conversions to double are exact (S <= 255 n < 2^53)

// n > 0 counted voxels in [lo, 255] with the sum S
int otsu_raw(const uint64_t *H, int lo, u64 n, u64 S)
{
    u64 n0 = 0, S0 = 0;
    double best = 0;
    int raw = -1, last = lo;
    for (int t = lo + 1; t <= 255; t++) {
        n0 += H[t - 1];
        S0 += (u64)(t - 1) * H[t - 1];
        if (H[t]) last = t;
        const u64 n1 = n - n0, S1 = S - S0;
        if (n0 == 0 || n1 == 0) continue;
        const double w0 = (double)n0, w1 = (double)n1;
        const double d = (double)S1 / w1 - (double)S0 / w0;
        const double score = ((w0 * w1) * d) * d;
        if (raw < 0 || score > best) {
            best = score;
            raw = t;
        }
    }
    return raw >= 0 ? raw : last; // (no valid t: `last` is the one non-empty bin)
}

int triangle_raw(const uint64_t *H, int p, int e)
{
    if (e - p < 2) return e;
    const i64 Hp = (i64)H[p], He = (i64)H[e];
    i64 best = 0;
    int at = -1;
    for (int b = p + 1; b <= e - 1; b++) {
        const i64 g = (Hp - He) * (i64)(e - b) + (He - (i64)H[b]) * (i64)(e - p);
        if (at < 0 || g > best) {
            best = g;
            at = b;
        }
    }
    return at + 1;
}

int top_raw(const uint64_t *H, int lo, u64 n, int top_ppm)
{
    const u64 M = 1000000, k = n / M * (u64)top_ppm + n % M * (u64)top_ppm / M; // floor(n top_ppm / 10^6) without the wide product
    u64 tail = n;                                                                // the counted voxels >= t
    for (int t = lo; t <= 255; t++) {
        if (tail <= k) return t;
        tail -= H[t];
    }
    return 255;
}

} // namespace

int threshold_rule(const char *who, const uint64_t *hist, const pnr_threshold_opts *opts, pnr_threshold_info *info)
{
    PNR_REQUIRE(hist && opts && info, PNR_E_ARG, "null argument");
    const pnr_threshold_opts o = *opts;
    PNR_REQUIRE(o.method >= PNR_THR_MEAN && o.method <= PNR_THR_MAXENTROPY, PNR_E_ARG, "%s: method = %d outside [0, 4]", who, o.method);
    PNR_REQUIRE(o.lo >= 0 && o.lo <= 255, PNR_E_ARG, "%s: lo = %d outside [0, 255]", who, o.lo);
    if (o.method == PNR_THR_TOP)
        PNR_REQUIRE(o.top_ppm >= 1 && o.top_ppm <= 999999, PNR_E_ARG, "%s: top_ppm = %d outside [1, 999999]", who, o.top_ppm);
    else
        PNR_REQUIRE(o.top_ppm == 0, PNR_E_ARG, "%s: top_ppm = %d, not 0 (only method 3 takes a share)", who, o.top_ppm);
    u64 n_vox = 0, me[256]; // me: the counts as maxentropy_from_hist takes them
    for (int v = 0; v < 256; v++) {
        PNR_REQUIRE(hist[v] < MAX_VOX && n_vox + hist[v] < MAX_VOX, PNR_E_ARG, "%s: more than 2^45 - 1 voxels (bin %d holds %llu)", who, v, (u64)hist[v]);
        n_vox += hist[v];
    }
    if (o.method == PNR_THR_MAXENTROPY) {
        PNR_REQUIRE(o.lo == 0, PNR_E_ARG, "%s: maxentropy needs lo = 0, not %d", who, o.lo);
        for (int v = 0; v < 256; v++) me[v] = hist[v];
        if (const int rc = maxentropy_bins_fit(who, me)) return rc;
    }
    u64 n = 0, S = 0;
    int v_min = -1, v_max = -1, peak = -1;
    for (int v = o.lo; v <= 255; v++) {
        if (!hist[v]) continue;
        n += hist[v];
        S += (u64)v * hist[v];
        if (v_min < 0) v_min = v;
        v_max = v;
        if (peak < 0 || hist[v] > hist[peak]) peak = v;
    }
    int thr = 255;
    if (n) {
        int raw = 0;
        switch (o.method) {
        case PNR_THR_MEAN: raw = (int)(S / n); break;
        case PNR_THR_OTSU: raw = otsu_raw(hist, o.lo, n, S); break;
        case PNR_THR_TRIANGLE: raw = triangle_raw(hist, peak, v_max); break;
        case PNR_THR_TOP: raw = top_raw(hist, o.lo, n, o.top_ppm); break;
        default: raw = maxentropy_from_hist(me);
        }
        thr = std::min(255, std::max(raw, std::max(o.lo, 1)));
    }
    u64 n_fg = 0;
    for (int v = thr; v <= 255; v++) n_fg += hist[v];
    *info = pnr_threshold_info{(int64_t)n_vox, (int64_t)n, S, (int64_t)n_fg, thr, o.method, o.lo, v_min, v_max, peak};
    return PNR_OK;
}

} // namespace pnr
