// tilework.h -- the flagged-tile relaxation the volume tools share, written once.  Users: morph, watershed (two passes), geodesic; geojoin
// takes the dimensions and the launch cut.  A tool relaxes a monotone rule over the volume in tiles of TX x TY x TZ voxels, a work-group
// per tile, until nothing changes:
//   flags       two int arrays over the tile grid: the tiles to visit in this round, and the ones marked for the next.
//   compaction  tile_compact turns the marked tiles of the current array into a list (cleared as they are listed) and their count.
//   count       comes back through 8 bytes of pinned memory; 0 ends the rounds.
//   launches    the caller's relax kernel runs over the list in launches of at most tiles_per_launch work-groups.  A work-group stages
//               its tile and the halo of 1 in LDS (stage_cells), iterates there, stores what changed -- only the owner tile ever writes a
//               voxel -- and marks in the NEXT array every neighbouring tile whose halo holds a changed voxel (halo_bits, mark_tiles), and
//               itself when the iteration bound cut its convergence short.  A reader may see a stale halo value inside a launch: still a
//               bound on the right side, and its writer has marked the reader.  No work-group waits for another.
//   swap        the arrays change places; the settle bound only ends a loop that a fault keeps alive.
// Order, tiling and launch cuts decide the number of rounds and visits, never a bit of a result.
#pragma once
#include "call.h"
#include "grid.h"

namespace pnr {

constexpr int TILE_TPB = 256;         // threads per work-group of tile_compact, and of the tools' per-voxel kernels (the extent check)
constexpr int AUTO_TILES = 1 << 20;   // tiles per launch where a tool's *_tiles_per_launch option is 0
inline int64_t tiles_per_launch(int option) { return option > 0 ? option : AUTO_TILES; }

// the dimensions of the context's volume in tiles of TX x TY x TZ; PNR_E_ARG where the tile numbers or the work-groups of a per-voxel
// launch would not fit 31 bits
template <int TX, int TY, int TZ>
int tile_dims(const pnr_ctx *c, const char *who, TileDims &d)
{
    d = TileDims{(int)c->w, (int)c->h, (int)c->l, (int)((c->w + TX - 1) / TX), (int)((c->h + TY - 1) / TY), (int)((c->l + TZ - 1) / TZ)};
    PNR_REQUIRE(d.tiles() < (1LL << 31) - TILE_TPB && (c->N + TILE_TPB - 1) / TILE_TPB < (1LL << 31), PNR_E_ARG, "%s: volume extent too large", who);
    return PNR_OK;
}

// what a tool's tile and work-group sizes must satisfy: TX x TY threads relax a tile, TPB threads run its per-voxel kernels
template <int TX, int TY, int TZ, int TPB>
constexpr bool tile_shape_ok()
{
    static_assert(TX * TY % 64 == 0 && TX * TY <= 1024 && TPB % 64 == 0, "whole waves");
    static_assert(TX >= 2 && TY >= 2 && TZ >= 2, "a voxel is on at most one of the two faces of an axis");
    static_assert(TPB == TILE_TPB, "the extent check of tile_dims covers the tool's per-voxel launches");
    return true;
}

// ---- the device half ----

// The TX x TY threads of a work-group walk the (TX + 2) (TY + 2) (TZ + 2) cells of the tile at `o` and its halo of 1:
// f(cx, cy, cz, inside, g, own) with the cell's coordinates (the halo at 0 and T + 1), whether it lies inside the volume, its linear
// voxel index (-1 outside) and whether it is one of the tile's own cells.
template <int TX, int TY, int TZ, typename F>
__device__ inline void stage_cells(const TileDims &d, const TileAt &o, F &&f)
{
    constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;
    for (int cell = threadIdx.x; cell < HX * HY * HZ; cell += TX * TY) {
        const int cx = cell % HX, cy = cell / HX % HY, cz = cell / (HX * HY);
        const int gx = o.x0 + cx - 1, gy = o.y0 + cy - 1, gz = o.z0 + cz - 1;
        const bool inside = gx >= 0 && gx < d.w && gy >= 0 && gy < d.h && gz >= 0 && gz < d.l;
        f(cx, cy, cz, inside, inside ? voxel_index(d.w, d.h, gx, gy, gz) : -1, cx >= 1 && cx <= TX && cy >= 1 && cy <= TY && cz >= 1 && cz <= TZ);
    }
}

// the tiles whose halo holds the voxel (lx, ly, z) of this tile, as bits (az + 1) 9 + (ay + 1) 3 + (ax + 1); bit 13 is the tile itself
template <int TX, int TY, int TZ>
__device__ inline unsigned halo_bits(int lx, int ly, int z)
{
    const unsigned mx = 2u | (lx == 0 ? 1u : 0u) | (lx == TX - 1 ? 4u : 0u), my = 2u | (ly == 0 ? 1u : 0u) | (ly == TY - 1 ? 4u : 0u);
    const unsigned mz = 2u | (z == 0 ? 1u : 0u) | (z == TZ - 1 ? 4u : 0u);
    unsigned bits = 0;
#pragma unroll
    for (int az = 0; az < 3; az++)
#pragma unroll
        for (int ay = 0; ay < 3; ay++)
            if ((mz >> az & 1u) && (my >> ay & 1u)) bits |= mx << (az * 9 + ay * 3);
    return bits;
}

// The end of a visit, by every thread: `mine`, the halo_bits of the voxels the thread changed, goes into the work-group's LDS word
// `touched` (zeroed before the last barrier), and the first 27 threads mark in flag_next the tiles it names, and the tile itself where
// `again` says that the iteration bound cut its convergence short
__device__ inline void mark_tiles(int *flag_next, const TileDims &d, const TileAt &o, int tile, unsigned &touched, unsigned mine, int again)
{
    if (mine) atomicOr(&touched, mine);
    __syncthreads();
    if (threadIdx.x >= 27) return;
    const int ax = (int)threadIdx.x % 3 - 1, ay = (int)threadIdx.x / 3 % 3 - 1, az = (int)threadIdx.x / 9 - 1;
    if (threadIdx.x == 13) {
        if (again) flag_next[tile] = 1;
    } else if (touched >> threadIdx.x & 1u) {
        const int nx = o.tx + ax, ny = o.ty + ay, nz = o.tz + az;
        if (nx >= 0 && nx < d.ntx && ny >= 0 && ny < d.nty && nz >= 0 && nz < d.ntz) flag_next[(nz * d.nty + ny) * d.ntx + nx] = 1;
    }
}

// ---- the host half: the rounds of one tool call ----
class TileRounds {
    pnr_ctx *c_;
    const char *who_;
    int64_t tiles_;
    Part<int> flag_, list_;
    Part<unsigned long long> count_;
    PinBuf<unsigned long long> h_count_;

public:
    struct Tally {
        int64_t rounds = 0, visits = 0;
    };

    // registers the two flag arrays, the list and the count (12 bytes per tile and a word) on the caller's buffer, before its alloc()
    TileRounds(pnr_ctx *c, const char *who, CallBuf &buf, const TileDims &d)
        : c_(c), who_(who), tiles_(d.tiles()), flag_(buf.add<int>((size_t)tiles_ * 2)), list_(buf.add<int>((size_t)tiles_)), count_(buf.add<unsigned long long>(1)) {}
    // the pinned word, after the buffer's alloc(): PNR_E_NOMEM with its message set on failure
    int pin();
    int *flag0() const { return flag_.get(); } // the array the first round lists
    void seed_all(Call &call) { call.fill(flag0(), 1, (size_t)tiles_), call.fill(flag0() + tiles_, 0, (size_t)tiles_); } // round 1: every tile
    void seed_none(Call &call) { call.fill(flag_, 0); } // round 1: what the caller's kernel marks in flag0()
    // Rounds until a compaction lists nothing: per round the compaction under the timer `group` (the last, empty one included), the
    // count, and relax(const int *list, int64_t n, int *flag_next) once per launch of at most per_launch tiles.  More than `bound` rounds is
    // PNR_E_HIP "the relaxation did not settle"; pass > 0 names the pass in that message.  `tally` receives the rounds and tile visits.
    // Returns with the stream synchronised.
    template <typename F>
    int run(Call &call, const char *group, int64_t per_launch, int64_t bound, int pass, F &&relax, Tally &tally)
    {
        tally = Tally{};
        for (int cur = 0; call.ok(); cur ^= 1) {
            int64_t count = 0;
            const int rc = list_tiles(call, group, cur, bound, pass, tally, count);
            if (rc || count == 0) return rc;
            for (int64_t at = 0; at < count; at += per_launch) relax((const int *)list_.get() + at, std::min(per_launch, count - at), flag0() + (cur ^ 1) * tiles_);
        }
        return call.finish();
    }

private:
    // the head of a round: the marked tiles of flag array `cur` into the list; their number, synchronised, counted into `tally`
    int list_tiles(Call &call, const char *group, int cur, int64_t bound, int pass, Tally &tally, int64_t &count);
};

} // namespace pnr
