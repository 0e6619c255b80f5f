// playback.cpp -- the scheduler of pnr_trace_replay[_sharded] (stream_sched.h) over a HOST engine that plays back map-free traces: no GPU
// involved.  PlaybackEngine is a host model of the HIP engine's stream order; pnr_sched_playback[2] (include/pnr_hip_test.h) run it.
#include "args.h"
#include "replay.h"
#include "stream_sched.h"

using pnr::set_error;

namespace {
struct PlaybackEngine final : pnr::StreamEngine {
    // (s_*: the state wait() hands to the scheduler -- the one behind the first poll - lag steps of the last launch, as PhasedEngine's)
    struct Slot { bool used = false, done = false, s_done = false; int it = 0, T = 0, Tfree = 0, s_it = 0, s_T = 0; std::vector<pnr_xest> xc; };
    const pnr_params &prm;
    int64_t W, H;
    int ni, nslots;
    pnr_trace_fn fn;
    void *user;
    std::vector<Slot> sl;
    std::vector<std::vector<int>> active; // per group
    // stream order, modelled: a control() is queued on its group's stream and has only run for sure once that group has been waited
    // for (or settled); until then no OTHER group may be handed a slot it names (the HIP engine would race: advisor finding, round 3)
    std::vector<int> ctl_pending; // per slot: the group whose control() names it and may not have run yet, or -1
    int s_active[4] = {0, 0, 0, 0};
    std::unordered_map<int64_t, uint8_t> den;
    std::string msg;
    int64_t steps = 0;
    PlaybackEngine(const pnr_params &p, int64_t w, int64_t h, int window, pnr_trace_fn f, void *u)
        : prm(p), W(w), H(h), ni(p.ni), nslots(window), fn(f), user(u), sl((size_t)window), active(4), ctl_pending((size_t)window, -1) {}
    const char *error() const override { return msg.c_str(); }
    int slots() const override { return nslots; }
    int max_groups() const override { return 4; }
    int admit(int g, const int *slots, const float *s6, int m) override
    {
        for (int j = 0; j < m; j++) {
            if (ctl_pending[(size_t)slots[j]] >= 0 && ctl_pending[(size_t)slots[j]] != g) {
                msg = "slot handed to another trace group before the control() that frees it has run";
                return PNR_E_STATE;
            }
            Slot &s = sl[(size_t)slots[j]];
            s = Slot();
            s.used = true;
            s.xc.assign((size_t)ni, pnr_xest{});
            int32_t T = 0;
            const int rc = fn(user, s6 + (size_t)j * 6, &T, s.xc.data());
            if (rc) { msg = "trace callback failed"; return PNR_E_STATE; }
            s.Tfree = T;
            active[(size_t)g].push_back(slots[j]);
        }
        return PNR_OK;
    }
    void snapshot(int g)
    {
        s_active[g] = (int)active[(size_t)g].size();
        for (Slot &s : sl) { s.s_done = s.done; s.s_it = s.it; s.s_T = s.T; } // (all slots: PhasedEngine copies the whole flag array, too)
    }
    int launch(int g, int, int poll, int lag) override
    {
        // what ph_update does with a trace, on the recorded map-free result: iteration `it` fails (T = it), or succeeds and its
        // centroid voxel is saturated in the replayed map (DENSITY stop, T = it + 1), or the trace goes on
        for (int k = 0; k < poll; k++) {
            std::vector<int> keep;
            for (int slot : active[(size_t)g]) {
                Slot &s = sl[(size_t)slot];
                if (s.it >= s.Tfree || s.it >= ni) { s.T = s.Tfree; s.done = true; continue; }
                const pnr_xest &e = s.xc[(size_t)s.it];
                const int64_t v = (int64_t)(int)std::round(e.z) * W * H + (int64_t)(int)std::round(e.y) * W + (int)std::round(e.x);
                auto f = den.find(v);
                s.it++;
                if (f != den.end() && (int)f->second >= prm.nodepervol) { s.T = s.it; s.done = true; continue; }
                keep.push_back(slot);
            }
            active[(size_t)g].swap(keep);
            steps++;
            if (k == poll - 1 - lag) snapshot(g);
        }
        return PNR_OK;
    }
    int wait(int g, int *act) override
    {
        *act = s_active[g];
        for (int &p : ctl_pending) if (p == g) p = -1;
        return PNR_OK;
    }
    int settle(int g) override
    {
        for (int &p : ctl_pending) if (p == g) p = -1;
        return PNR_OK;
    }
    bool finished(int, int slot, int *T) const override { *T = sl[(size_t)slot].s_T; return sl[(size_t)slot].s_done; }
    const pnr_xest *rows(int slot) const override { return sl[(size_t)slot].xc.data(); }
    int progress(int, int slot) const override { return sl[(size_t)slot].s_it; }
    int control(int g, const int *pause, int np, const int *resume, int nr) override
    {
        std::vector<int> &a = active[(size_t)g];
        for (int j = 0; j < np; j++) {
            ctl_pending[(size_t)pause[j]] = g;
            auto f = std::find(a.begin(), a.end(), pause[j]);
            if (f == a.end()) { // (stopped by itself in the steps that ran behind the state the scheduler decided on)
                if (!sl[(size_t)pause[j]].done) { msg = "pause of a trace that is not stepped"; return PNR_E_STATE; }
                continue;
            }
            a.erase(f);
        }
        for (int j = 0; j < nr; j++) {
            if (std::find(a.begin(), a.end(), resume[j]) != a.end()) { msg = "resume of a trace that is stepped"; return PNR_E_STATE; }
            a.push_back(resume[j]);
        }
        return PNR_OK;
    }
    int density_update(const pnr::Replayer &r, int) override
    {
        for (int64_t v : r.touched) den[v] = (uint8_t)r.den_at(v);
        return PNR_OK;
    }
    void drain() override {}
};
} // namespace

extern "C" {

int pnr_sched_playback(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n, int rank, int world,
                       pnr_allgather_fn exchange, void *xuser, int64_t block_bytes, pnr_trace_fn trace, void *tuser, int window, int groups,
                       int poll, int look0, int look_pct, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes, int32_t *links, int64_t cap_links,
                       int64_t *n_links, int64_t *n_traces_used, int64_t *n_iterations)
{
    if (window < 2) window = 2; // (this entry point has always clamped; only pnr_sched_playback2 treats a window below 2 as a set-up failure)
    return pnr_sched_playback2(p, w, h, l, seeds, n, rank, world, exchange, xuser, block_bytes, trace, tuser, window, groups, poll, look0, look_pct,
                               /*tentative*/ 1, /*target*/ -1, /*lag*/ -1, nodes, cap_nodes, n_nodes, links, cap_links, n_links, n_traces_used, n_iterations);
}

int pnr_sched_playback2(const pnr_params *p, int64_t w, int64_t h, int64_t l, const pnr_seed *seeds, int64_t n, int rank, int world,
                        pnr_allgather_fn exchange, void *xuser, int64_t block_bytes, pnr_trace_fn trace, void *tuser, int window, int groups,
                        int poll, int look0, int look_pct, int tentative, int target, int lag, pnr_node *nodes, int64_t cap_nodes, int64_t *n_nodes,
                        int32_t *links, int64_t cap_links, int64_t *n_links, int64_t *n_traces_used, int64_t *n_iterations)
{
    PNR_REQUIRE(p && trace && n_nodes && n_links && (n == 0 || seeds), PNR_E_ARG, "null argument");
    PNR_REQUIRE(w > 0 && h > 0 && l > 0, PNR_E_ARG, "bad dimensions");
    PNR_REQUIRE(world >= 1 && rank >= 0 && rank < world && (world == 1 || exchange), PNR_E_ARG, "bad rank / world / exchange");
    pnr::ShardSpec sh;
    sh.rank = rank; sh.world = world; sh.exchange = exchange; sh.user = xuser; sh.block_bytes = block_bytes;
    if (window < 2) { // the playback engine's "set-up failure" (what an out-of-memory GPU is to the HIP engine): the other ranks must hear of it
        set_error("playback engine: a window of %d trace slots", window);
        if (n > 0) pnr::abort_exchange(sh, p->ni);
        return PNR_E_ARG;
    }
    pnr::Replayer r(*p, w, h, l);
    window &= ~1;
    PlaybackEngine eng(*p, w, h, window, trace, tuser);
    pnr::SchedOptions o;
    o.window = window; o.groups = std::max(1, groups); o.poll = std::max(1, poll);
    o.look0 = std::max(0, look0); o.look_pct = look_pct;
    o.tentative = tentative != 0;
    o.target = std::max(-1, target);
    o.lag = std::max(-1, lag);
    pnr::SchedStats st;
    std::string err;
    const int rc = pnr::run_stream(eng, seeds, n, p->ni, o, sh, r, &st, err);
    if (rc) { set_error("%s", err.c_str()); return rc; }
    pnr::put_graph(r.nodes, r.links, nodes, cap_nodes, n_nodes, links, cap_links, n_links);
    if (n_traces_used) *n_traces_used = r.trace_count;
    if (n_iterations) *n_iterations = st.iters;
    return PNR_OK;
}

} // extern "C"
