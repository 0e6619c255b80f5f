// tilework.hip -- the host half of the flagged-tile relaxation (tilework.h): the compaction kernel and the rounds.
#include "tilework.h"
#include <cstdio>

namespace {

typedef unsigned long long u64;
using pnr::TILE_TPB;

__global__ __launch_bounds__(TILE_TPB) void tile_compact(int *flag, int tiles, int *list, u64 *count)
{
    const int i = blockIdx.x * TILE_TPB + threadIdx.x;
    if (i >= tiles || !flag[i]) return;
    flag[i] = 0;
    list[atomicAdd(count, 1ull)] = i; // (at most `tiles` entries: every tile is listed once)
}

} // namespace

namespace pnr {

int TileRounds::pin()
{
    if (h_count_.alloc(1) == hipSuccess) return PNR_OK;
    (void)hipGetLastError();
    set_error("%s: pinned allocation of 8 B failed", who_);
    return PNR_E_NOMEM;
}

int TileRounds::list_tiles(Call &call, const char *group, int cur, int64_t bound, int pass, Tally &tally, int64_t &count)
{
    c_->tic();
    call.fill(count_, 0);
    call.launch(tile_compact, dim3((unsigned)((tiles_ + TILE_TPB - 1) / TILE_TPB)), dim3(TILE_TPB), flag0() + cur * tiles_, (int)tiles_, list_.get(), count_.get());
    c_->toc(group, 1);
    call.down(h_count_.get(), count_);
    const int rc = call.finish();
    if (rc) return rc;
    count = (int64_t)*h_count_.get();
    if (count == 0) return PNR_OK;
    char in_pass[24] = "";
    if (pass > 0) snprintf(in_pass, sizeof in_pass, "pass %d, ", pass);
    PNR_REQUIRE(count <= tiles_ && tally.rounds < bound, PNR_E_HIP, "%s: the relaxation did not settle (%sround %lld, %lld tiles listed)", who_, in_pass,
                (long long)tally.rounds, (long long)count);
    tally.rounds++, tally.visits += count;
    return PNR_OK;
}

} // namespace pnr
