"""pnr_amd -- MI355X (gfx950) implementation of the PNR / Advantra neurite-tracer hot path:
multi-scale Frangi vesselness, seed extraction and the batched SMC particle tracer, as
hand-written HIP kernels behind a C ABI (include/pnr_hip.h).  See DESIGN.md."""
from . import lib  # noqa: F401
from .lib import Context, Params, PnrError, RadiusOpts, ComponentsOpts, ComponentsInfo, COMPONENT_DT, EdtOpts, EdtInfo, ThinOpts, ThinInfo, GeoOpts, GeoInfo, GeoJoinOpts, GeoJoinInfo, GEO_BRIDGE, MorphOpts, MorphInfo, MORPH_OPS, WatershedOpts, WatershedInfo, ThresholdOpts, ThresholdInfo, THRESHOLD_METHODS, LocalOpts, LocalInfo, PruneOpts, PruneInfo, prune_tree_host, prune_apply, parse_threshold, threshold_from_hist, make_params, radius_offsets, pair_tiles, read_swc, read_swc_nodes, render_items, tree_sample, join_reroot, join_expand, skeleton_forest  # noqa: F401
from .advantra import Frangi, SeedExtractor, Tracker, advantra_func, write_swc, write_swc_tree  # noqa: F401
