// threshold_rule_check.cpp -- a stand-alone program around threshold_rule.cpp for the host sanitizers (make rule_check): every
// method on the edge histograms of the rule -- empty, one bin, two bins, nothing at or above lo, equal peaks and flat stretches,
// bins of 2^33 counts, the largest total -- and every argument error.  It checks only what needs no second implementation (the
// range of thr, the counts of the info); tests/test_threshold_host.py holds the values against the numpy restatement.
#include "threshold.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace pnr {
static char last[512];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last, sizeof last, fmt, ap);
    va_end(ap);
}
} // namespace pnr

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); fails++; } } while (0)

static void run_all(const uint64_t *H, bool small_bins)
{
    const int los[] = {0, 1, 17, 255};
    for (int method = PNR_THR_MEAN; method <= PNR_THR_MAXENTROPY; method++)
        for (int lo : los)
            for (int ppm : {1, 10000, 999999}) {
                const pnr_threshold_opts o{method, lo, method == PNR_THR_TOP ? ppm : 0, 0};
                pnr_threshold_info info;
                const int rc = pnr::threshold_rule("check", H, &o, &info);
                if (method == PNR_THR_MAXENTROPY && (lo != 0 || !small_bins)) {
                    EXPECT(rc == PNR_E_ARG);
                    continue;
                }
                EXPECT(rc == PNR_OK);
                EXPECT(info.thr >= (lo > 1 ? lo : 1) && info.thr <= 255);
                uint64_t n = 0, fg = 0;
                for (int v = 0; v < 256; v++) n += v >= lo ? H[v] : 0, fg += v >= info.thr ? H[v] : 0;
                EXPECT((uint64_t)info.n_counted == n && (uint64_t)info.n_fg == fg);
                EXPECT(n ? info.v_min >= lo && info.v_max >= info.v_min && info.peak >= info.v_min && info.peak <= info.v_max : info.thr == 255 && info.peak == -1);
                if (method != PNR_THR_TOP) break;
            }
}

int main()
{
    uint64_t H[256] = {0};
    run_all(H, true); // empty
    H[0] = 5;
    run_all(H, true); // one bin, below most lo
    H[0] = 0, H[255] = 1;
    run_all(H, true);
    H[255] = 0, H[17] = 3, H[200] = 3;
    run_all(H, true); // two bins, equal peaks
    for (int v = 0; v < 256; v++) H[v] = 7;
    run_all(H, true); // flat
    for (int v = 0; v < 256; v++) H[v] = (uint64_t)((v * 2654435761u) >> 20);
    run_all(H, true);
    for (int v = 0; v < 256; v++) H[v] = v % 3 ? 1ull << 33 : 0;
    run_all(H, false); // u64 counts
    for (int v = 0; v < 256; v++) H[v] = 0;
    H[0] = (1ull << 45) - 2, H[255] = 1;
    run_all(H, false); // the largest total
    H[3] = 1;          // 2^45 voxels
    pnr_threshold_opts o{PNR_THR_OTSU, 0, 0, 0};
    pnr_threshold_info info;
    EXPECT(pnr::threshold_rule("check", H, &o, &info) == PNR_E_ARG);
    H[0] = ~0ull;
    EXPECT(pnr::threshold_rule("check", H, &o, &info) == PNR_E_ARG);
    { // the boundary of maximum entropy: a bin of 2^31 - 1 is read whole as the reference's `int`, one of 2^31 is refused -- by the
      // rule and by the check pnr_soma shares with it
        uint64_t B[256] = {0};
        unsigned long long b[256] = {0};
        B[0] = b[0] = (1ull << 31) - 1, B[40] = b[40] = 1000, B[200] = b[200] = 10;
        const pnr_threshold_opts me{PNR_THR_MAXENTROPY, 0, 0, 0};
        EXPECT(pnr::threshold_rule("check", B, &me, &info) == PNR_OK && info.thr >= 1 && info.thr <= 255 && info.n_vox == (int64_t)((1ull << 31) + 1009));
        EXPECT(pnr::maxentropy_bins_fit("check", b) == PNR_OK);
        B[0] = b[0] = 1ull << 31;
        EXPECT(pnr::threshold_rule("check", B, &me, &info) == PNR_E_ARG);
        EXPECT(pnr::maxentropy_bins_fit("check", b) == PNR_E_ARG);
        EXPECT(std::string(pnr::last) == "check: maxentropy needs every bin below 2^31, bin 0 holds 2147483648");
        b[0] = 5, b[255] = ~0ull;
        EXPECT(pnr::maxentropy_bins_fit("check", b) == PNR_E_ARG);
    }
    H[0] = 1;
    for (const pnr_threshold_opts bad : {pnr_threshold_opts{-1, 0, 0, 0}, pnr_threshold_opts{5, 0, 0, 0}, pnr_threshold_opts{1, -1, 0, 0}, pnr_threshold_opts{1, 256, 0, 0},
                                         pnr_threshold_opts{3, 0, 0, 0}, pnr_threshold_opts{3, 0, 1000000, 0}, pnr_threshold_opts{1, 0, 5, 0}})
        EXPECT(pnr::threshold_rule("check", H, &bad, &info) == PNR_E_ARG);
    EXPECT(pnr::threshold_rule("check", nullptr, &o, &info) == PNR_E_ARG && pnr::threshold_rule("check", H, nullptr, &info) == PNR_E_ARG &&
           pnr::threshold_rule("check", H, &o, nullptr) == PNR_E_ARG);
    std::printf(fails ? "threshold rule check: %d failures\n" : "threshold rule check ok\n", fails);
    return fails ? 1 : 0;
}
