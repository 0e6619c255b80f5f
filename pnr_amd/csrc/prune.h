// prune.h -- pruning a tree's short side branches and the per-node morphometry (the rule of include/pnr_hip.h): the sequential host
// pass (prune_rule.cpp, pure host), the pointer jumping on the device (prune.hip) and the compaction; behind pnr_prune_tree,
// pnr_prune_tree_host and pnr_prune_apply.
#pragma once
#include "ctx.h"
#include <cmath>

namespace pnr {

// Q(x) = floor(256 x + 0.5) in double: a length in units of 1/256 xy voxel
inline __host__ __device__ double prune_q(double x) { return floor(256.0 * x + 0.5); }
constexpr double PRUNE_LIMIT = 4294967296.0; // 2^32 units: rule 7
#define PNR_PRUNE_RANGE_TEXT "%s: a path reaches 2^32 units of 1/256 voxel: the limit is 2^24 xy voxels of path"

// the options as the rule uses them: the two thresholds in units, and what the radius is multiplied with
struct PruneRule {
    double zscale, q_length, factor, q_tree;
    explicit PruneRule(const pnr_prune_opts &o) : zscale((double)o.zscale), q_length(prune_q((double)o.min_length)), factor((double)o.radius_factor), q_tree(prune_q((double)o.min_tree)) {}
    // rule 1 as a double: the caller compares it with PRUNE_LIMIT before it becomes a u32
    __host__ __device__ double edge(const float *a, const float *b) const
    {
        const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = ((double)a[2] - (double)b[2]) * zscale;
        return prune_q(sqrt(dx * dx + dy * dy + dz * dz));
    }
    // rule 5 for a non-root head of segment length S on a parent of radius r
    __host__ __device__ bool cut(uint32_t S, float r) const
    {
        const double by_radius = prune_q(factor * (double)r);
        return (double)S < (q_length > by_radius ? q_length : by_radius);
    }
    __host__ __device__ bool cut_tree(uint32_t H) const { return (double)H < q_tree; }
};

// The arguments of both calls, in the order of the header (texts as `who`'s); o = the options with the defaults filled in.  Pure host.
int prune_args(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts *opts, pnr_prune_opts &o);
// The rule as one sequential pass in topological order on checked arguments; every output is nullable.  Pure host.
int prune_rule(const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts &o, pnr_prune_info *info, uint8_t *keep,
               uint32_t *height, uint32_t *path, int32_t *order, int32_t *seg);
// pnr_prune_apply on its own arguments.  Pure host.
int prune_apply(const int32_t *parent, const uint8_t *keep, int64_t n, int32_t *new_index_out, int32_t *parent_out, int64_t *m);

} // namespace pnr

// The rule on c's GPU on checked arguments (prune.hip): every output is nullable, every device buffer is freed before it returns.
int pnr_prune_run(pnr_ctx *c, const char *who, const float *xyz, const float *radius, const int32_t *parent, int64_t n, const pnr_prune_opts &o, pnr_prune_info *info,
                  uint8_t *keep, uint32_t *height, uint32_t *path, int32_t *order, int32_t *seg);
