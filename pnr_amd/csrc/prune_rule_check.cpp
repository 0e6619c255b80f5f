// prune_rule_check.cpp -- a stand-alone program around prune_rule.cpp for the host sanitizers (make prune_check): the closed forms
// of the rule -- the Y with a tie, the star, the single chain, the radius rule, whole trees -- and its edge inputs: one node, two
// nodes, only roots, parents behind their children, every output NULL, the range limit and every argument error, and the compaction.
// It checks only what needs no second implementation; tests/test_prune_host.py holds the values against the numpy restatement.
#include "prune.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

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

struct Tree {
    std::vector<float> xyz, radius;
    std::vector<int32_t> parent;
    void add(float x, float y, float z, int32_t p, float r = 1.f) { xyz.insert(xyz.end(), {x, y, z}), radius.push_back(r), parent.push_back(p); }
    int64_t n() const { return (int64_t)parent.size(); }
};
struct Result {
    int rc;
    pnr_prune_info info;
    std::vector<uint8_t> keep;
    std::vector<uint32_t> height, path;
    std::vector<int32_t> order, seg;
};

static Result run(const Tree &t, pnr_prune_opts o, bool with_radius = true)
{
    const size_t n = (size_t)t.n();
    Result r{0, {}, std::vector<uint8_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<int32_t>(n), std::vector<int32_t>(n)};
    pnr_prune_opts checked;
    r.rc = pnr::prune_args("check", t.xyz.data(), with_radius ? t.radius.data() : nullptr, t.parent.data(), t.n(), &o, checked);
    if (!r.rc)
        r.rc = pnr::prune_rule("check", t.xyz.data(), with_radius ? t.radius.data() : nullptr, t.parent.data(), t.n(), checked, &r.info, r.keep.data(), r.height.data(),
                               r.path.data(), r.order.data(), r.seg.data());
    return r;
}
static int64_t kept(const Result &r) { return std::accumulate(r.keep.begin(), r.keep.end(), (int64_t)0); }

int main()
{
    { // Y with a tie: a stem of 3, two arms of 4
        Tree t;
        for (int i = 0; i < 4; i++) t.add(0, (float)i, 0, i - 1);
        for (int j = 1; j <= 4; j++) t.add((float)j, 3, 0, j == 1 ? 3 : 2 + j);
        for (int j = 1; j <= 4; j++) t.add((float)-j, 3, 0, j == 1 ? 3 : 6 + j);
        Result r = run(t, {1, 4.5f, 0, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == 8 && r.keep[4] && !r.keep[8] && r.seg[11] == 8 && r.order[11] == 1 && r.height[0] == 7 * 256 && r.info.n_removed_segments == 1);
        r = run(t, {1, 4.f, 0, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == 12);
        r = run(t, {2, 0, 0, 0}, false); // no radius; zscale on a flat tree changes nothing
        EXPECT(r.rc == PNR_OK && kept(r) == 12 && r.height[0] == 7 * 256);
        pnr_prune_opts o{1, 4.5f, 0, 0}, checked;
        pnr_prune_info info;
        EXPECT(pnr::prune_args("check", t.xyz.data(), nullptr, t.parent.data(), 12, &o, checked) == PNR_OK);
        EXPECT(pnr::prune_rule("check", t.xyz.data(), nullptr, t.parent.data(), 12, checked, &info, nullptr, nullptr, nullptr, nullptr, nullptr) == PNR_OK && info.n_removed == 4);
        EXPECT(pnr::prune_rule("check", t.xyz.data(), nullptr, t.parent.data(), 12, checked, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PNR_OK);
        // the compaction
        std::vector<int32_t> idx(12), par(12);
        int64_t m = 0;
        EXPECT(pnr::prune_apply(t.parent.data(), r.keep.data(), 12, idx.data(), par.data(), &m) == PNR_OK && m == 12);
        r = run(t, {1, 4.5f, 0, 0});
        EXPECT(pnr::prune_apply(t.parent.data(), r.keep.data(), 12, idx.data(), par.data(), &m) == PNR_OK && m == 8 && idx[8] == -1 && par[7] == 6);
        EXPECT(pnr::prune_apply(t.parent.data(), r.keep.data(), 12, nullptr, nullptr, &m) == PNR_OK && m == 8);
        r.keep[3] = 0; // keeps the children of a removed node
        EXPECT(pnr::prune_apply(t.parent.data(), r.keep.data(), 12, idx.data(), par.data(), &m) == PNR_E_ARG);
        EXPECT(pnr::prune_apply(nullptr, r.keep.data(), 12, idx.data(), par.data(), &m) == PNR_E_ARG && pnr::prune_apply(t.parent.data(), r.keep.data(), 0, nullptr, nullptr, &m) == PNR_E_ARG);
    }
    { // the star, its root last: every parent behind its children
        Tree t;
        for (int i = 0; i < 3000; i++) t.add(i % 2 ? 2.f : -2.f, 0, 0, 3000);
        t.add(0, 0, 0, -1);
        Result r = run(t, {1, 2.f, 0, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == 3001 && r.info.n_segments == 3000 && r.seg[0] == 3000 && r.seg[1] == 1);
        r = run(t, {1, 2.01f, 0, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == 2 && r.keep[0] && r.info.n_removed_segments == 2999);
    }
    { // the single chain, written leaf first
        Tree t;
        const int n = 5000;
        for (int i = 0; i < n; i++) t.add((float)i, 0, 0, i + 1 < n ? i + 1 : -1);
        Result r = run(t, {1, 1e5f, 50.f, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == n && r.info.n_segments == 1 && r.path[0] == 4999 * 256 && r.height[(size_t)n - 1] == 4999 * 256 && r.info.order_max == 0);
        r = run(t, {1, 0, 0, 5000.f});
        EXPECT(r.rc == PNR_OK && kept(r) == 0 && r.info.n_removed_trees == 1);
    }
    { // the radius rule and whole trees
        for (float rp : {1.f, 2.f}) {
            Tree t;
            for (int i = 0; i < 8; i++) t.add((float)i, 0, 0, i - 1, i == 4 ? rp : 1.f);
            t.add(4, 3, 0, 4);
            t.add(50, 50, 50, -1); // a tree of one node
            Result r = run(t, {1, 0, 2.f, 0});
            EXPECT(r.rc == PNR_OK && r.keep[8] == (rp == 1.f) && r.keep[9]);
            r = run(t, {1, 0, 0, 0.01f});
            EXPECT(r.rc == PNR_OK && kept(r) == 9 && !r.keep[9] && r.info.n_removed_trees == 1);
        }
    }
    { // one node, two nodes, only roots
        Tree t;
        t.add(1, 2, 3, -1);
        Result r = run(t, {1, 0, 0, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == 1 && r.info.n_leaves == 1 && r.info.n_segments == 1 && r.seg[0] == 0);
        t.add(1, 2, 4, 0);
        r = run(t, {3, 0, 0, 0});
        EXPECT(r.rc == PNR_OK && r.height[0] == 768 && r.path[1] == 768);
        t.parent[1] = -7;
        r = run(t, {1, 9, 9, 0});
        EXPECT(r.rc == PNR_OK && kept(r) == 2 && r.info.n_roots == 2);
    }
    { // the range and the arguments
        Tree t;
        for (int i = 0; i < 3; i++) t.add(1e7f * (float)i, 0, 0, i - 1);
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_E_ARG);
        t.xyz[6] = 1.5e7f; // 2^32 - 1 is not reached: 2.56e9 + 1.28e9
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_OK);
        t.xyz[3] = 3e38f, t.xyz[6] = -3e38f;
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_E_ARG);
        t.xyz[3] = 1, t.xyz[6] = 2;
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_OK);
        for (const pnr_prune_opts bad : {pnr_prune_opts{0, 0, 0, 0}, pnr_prune_opts{-1, 0, 0, 0}, pnr_prune_opts{1, -1, 0, 0}, pnr_prune_opts{1, 0, -1, 0}, pnr_prune_opts{1, 0, 0, -1},
                                         pnr_prune_opts{1, NAN, 0, 0}, pnr_prune_opts{1, 0, INFINITY, 0}})
            EXPECT(run(t, bad).rc == PNR_E_ARG);
        t.parent[0] = 2; // a cycle
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_E_ARG);
        t.parent[0] = 3; // outside
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_E_ARG);
        t.parent[0] = -1, t.radius[1] = NAN;
        EXPECT(run(t, {1, 0, 0, 0}).rc == PNR_E_ARG && run(t, {1, 0, 0, 0}, false).rc == PNR_OK);
        t.xyz[4] = INFINITY;
        EXPECT(run(t, {1, 0, 0, 0}, false).rc == PNR_E_ARG);
        pnr_prune_opts o;
        EXPECT(pnr::prune_args("check", nullptr, nullptr, t.parent.data(), 3, nullptr, o) == PNR_E_ARG && pnr::prune_args("check", t.xyz.data(), nullptr, nullptr, 3, nullptr, o) == PNR_E_ARG &&
               pnr::prune_args("check", t.xyz.data(), nullptr, t.parent.data(), 0, nullptr, o) == PNR_E_ARG);
    }
    std::printf(fails ? "prune rule check: %d failures\n" : "prune rule check ok\n", fails);
    return fails ? 1 : 0;
}
