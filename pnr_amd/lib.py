"""ctypes binding of libpnr_hip.so (include/pnr_hip.h).  Plumbing only: every compute call goes
through the C ABI into the HIP kernels; there is no Python or CPU implementation behind it, and
loading fails loudly when the extension has not been built."""
import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNR_LIB_DIAG") or os.path.join(HERE, "libpnr_hip.so")  # PNR_LIB_DIAG: diagnostic builds only
PNR_MAX_SIGMAS = 8


class Window(C.Structure):
    """pnr_window (include/pnr_hip.h): a fixed [lo, hi], or lo = hi = -1 and the saturated voxels in parts per million"""
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32), ("sat_lo_ppm", C.c_int32), ("sat_hi_ppm", C.c_int32)]


def make_window(window):
    """None -> NULL ([min, max]); (lo, hi) -> that window; {"saturate": (lo_pct, hi_pct)} -> the window that clips those percentages
    of the voxels to 0 / to 255 (up to 4 decimals: parts per million)"""
    if window is None:
        return None
    if isinstance(window, dict):
        if set(window) != {"saturate"}:
            raise PnrError(f"window: (lo, hi) or {{'saturate': (lo_pct, hi_pct)}}, got {window!r}")
        a, b = window["saturate"]
        return Window(-1, -1, int(round(float(a) * 1e4)), int(round(float(b) * 1e4)))
    lo, hi = window
    return Window(int(lo), int(hi), 0, 0)


class RadiusOpts(C.Structure):
    """pnr_radius_opts (include/pnr_hip.h): thr -1..255 (-1: the global mean), rel_pct 0..100 (0: the absolute mode), rmax 1..64, bg_permille 0..999"""
    _fields_ = [("thr", C.c_int32), ("rel_pct", C.c_int32), ("rmax", C.c_int32), ("bg_permille", C.c_int32)]


PNR_RADIUS_MAX = 64


class FilterOpts(C.Structure):
    """pnr_filter_opts (include/pnr_hip.h): median 0 / 2 (3 x 3 in every slice) / 3 (3 x 3 x 3), tophat_r 0..64 (0: off)"""
    _fields_ = [("median", C.c_int32), ("tophat_r", C.c_int32)]


PNR_TOPHAT_MAX_R = 64


class DistanceOpts(C.Structure):
    """pnr_distance_opts (include/pnr_hip.h): zscale > 0 (z *= zscale first), step >= 0 (0: the nodes only), thr (the "big" distances)"""
    _fields_ = [("zscale", C.c_float), ("step", C.c_float), ("thr", C.c_float)]


class DistanceDir(C.Structure):
    """pnr_distance_dir: one direction of the tree distance"""
    _fields_ = [("n", C.c_int64), ("n_big", C.c_int64), ("mean", C.c_double), ("ssd", C.c_double), ("pct", C.c_double), ("max", C.c_double)]


class DistanceResult(C.Structure):
    """pnr_distance_result: ab = A's points against B's segments, ba = the reverse, and the combined metrics"""
    _fields_ = [("ab", DistanceDir), ("ba", DistanceDir), ("sd", C.c_double), ("ssd", C.c_double), ("pct", C.c_double), ("hausdorff", C.c_double)]

    def as_dict(self):
        d = {k: {f: getattr(getattr(self, k), f) for f, _ in DistanceDir._fields_} for k in ("ab", "ba")}
        d.update(sd=self.sd, ssd=self.ssd, pct=self.pct, hausdorff=self.hausdorff)
        return d


PNR_DISTANCE_MAX_N = 1 << 22


class JoinOpts(C.Structure):
    """pnr_join_opts (include/pnr_hip.h): zscale > 0 (z *= zscale first), gap >= 0 (0: no limit), root (a node index, negative: none)"""
    _fields_ = [("zscale", C.c_float), ("gap", C.c_float), ("root", C.c_int32)]


BRIDGE = np.dtype([("lo", np.int32), ("hi", np.int32), ("d", np.float32)])  # pnr_bridge
PNR_JOIN_MAX_N = 1 << 22


class RenderOpts(C.Structure):
    """pnr_render_opts (include/pnr_hip.h): zscale > 0 (z *= zscale first), rr = max(radius * rscale + radd, 0), thr -1..255 (-1: the global mean)"""
    _fields_ = [("zscale", C.c_float), ("rscale", C.c_float), ("radd", C.c_float), ("thr", C.c_int32)]


class Coverage(C.Structure):
    """pnr_coverage: the exact counts of a tree rendered on the context's volume and the three ratios derived from them"""
    _fields_ = [("n_vox", C.c_int64), ("n_tree", C.c_int64), ("n_fg", C.c_int64), ("n_both", C.c_int64), ("sum_fg", C.c_int64), ("sum_both", C.c_int64),
                ("thr_used", C.c_int32), ("pad", C.c_int32), ("covered", C.c_double), ("on_signal", C.c_double), ("covered_intensity", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


PNR_RENDER_MAX_N = 1 << 22
PNR_RENDER_MAX_R = 1024


class ComponentsOpts(C.Structure):
    """pnr_components_opts (include/pnr_hip.h): thr -1..255 (-1: the global mean), connectivity 6 or 26, min_size >= 1"""
    _fields_ = [("thr", C.c_int32), ("connectivity", C.c_int32), ("min_size", C.c_int64)]


class ComponentsInfo(C.Structure):
    """pnr_components_info: the exact counts of a labelling (n_comp: the kept components; n_small / vox_small: those below min_size)"""
    _fields_ = [("n_vox", C.c_int64), ("n_fg", C.c_int64), ("n_comp", C.c_int64), ("n_small", C.c_int64), ("vox_small", C.c_int64), ("largest", C.c_int64),
                ("thr_used", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


class EdtOpts(C.Structure):
    """pnr_edt_opts (include/pnr_hip.h): thr -1..255 (-1: the global mean), rmax 1..PNR_EDT_MAX_R (D2 is capped at rmax^2)"""
    _fields_ = [("thr", C.c_int32), ("rmax", C.c_int32)]


class EdtInfo(C.Structure):
    """pnr_edt_info: the exact summary of a distance transform (first_max: the smallest linear index that attains d2_max, -1 without foreground)"""
    _fields_ = [("n_vox", C.c_int64), ("n_fg", C.c_int64), ("n_capped", C.c_int64), ("first_max", C.c_int64), ("d2_max", C.c_float), ("thr_used", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


PNR_EDT_MAX_R = 1024


class ThinOpts(C.Structure):
    """pnr_thin_opts (include/pnr_hip.h): thr -1..255 (-1: the global mean), max_rounds >= 0 (0: until nothing is deleted)"""
    _fields_ = [("thr", C.c_int32), ("max_rounds", C.c_int32)]


class ThinInfo(C.Structure):
    """pnr_thin_info: the exact summary of a thinning (tile_visits: the work of the passes, a property of the implementation)"""
    _fields_ = [("n_vox", C.c_int64), ("n_fg", C.c_int64), ("n_skel", C.c_int64), ("n_end", C.c_int64), ("n_branch", C.c_int64), ("n_isolated", C.c_int64),
                ("tiles", C.c_int64), ("tile_visits", C.c_int64), ("rounds", C.c_int32), ("thr_used", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class GeoOpts(C.Structure):
    """pnr_geo_opts (include/pnr_hip.h): thr -1..255 (-1: the global mean; 0: every voxel is passable), dmax 1..2^31 - 1 (no path above it
    is kept), cost: 256 u16 entries >= 1 (NULL: c(v) = 256 - v)"""
    _fields_ = [("thr", C.c_int32), ("dmax", C.c_uint32), ("cost", C.POINTER(C.c_uint16))]


class GeoInfo(C.Structure):
    """pnr_geo_info: the exact summary of a geodesic distance (first_max: the smallest linear index that attains d_max, -1 when nothing is
    reached; rounds: relaxation rounds of the call)"""
    _fields_ = [("n_vox", C.c_int64), ("n_pass", C.c_int64), ("n_reached", C.c_int64), ("n_src", C.c_int64), ("n_src_dropped", C.c_int64), ("first_max", C.c_int64),
                ("d_max", C.c_uint32), ("thr_used", C.c_int32), ("rounds", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


PNR_GEO_MAX_PATH = 1 << 16
PNR_GEO_DMAX = 2**31 - 1


class GeoJoinOpts(C.Structure):
    """pnr_geojoin_opts (include/pnr_hip.h): thr and cost as in pnr_geo_opts, limit (0: none) the largest bridge weight W, step the spacing
    of the sample points along the segments (0: the nodes only)"""
    _fields_ = [("thr", C.c_int32), ("limit", C.c_uint64), ("step", C.c_float), ("cost", C.POINTER(C.c_uint16))]


class GeoJoinInfo(C.Structure):
    """pnr_geojoin_info: the exact summary of pnr_geodesic_bridges (rounds: Boruvka rounds of the call)"""
    _fields_ = [(k, C.c_int64) for k in ("n_trees_in", "n_trees_lost", "n_trees_out", "n_bridges", "n_inserted", "n_src", "n_src_dropped")] + [
        ("w_max", C.c_uint64), ("thr_used", C.c_int32), ("rounds", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class MorphOpts(C.Structure):
    """pnr_morph_opts (include/pnr_hip.h): op 1..5 (MORPH_OPS), connectivity 0 (the op's default: 6 for fill, 26 for the others), 4, 8, 6
    or 26, h 1..255 for hmax / hdome and 0 otherwise"""
    _fields_ = [("op", C.c_int32), ("connectivity", C.c_int32), ("h", C.c_int32), ("pad", C.c_int32)]


class MorphInfo(C.Structure):
    """pnr_morph_info: the exact summary of a morphological reconstruction (tile_visits and rounds: scheduling, a property of the implementation)"""
    _fields_ = [("n_vox", C.c_int64), ("n_changed", C.c_int64), ("n_nonzero", C.c_int64), ("sum_in", C.c_uint64), ("sum_out", C.c_uint64), ("tiles", C.c_int64),
                ("tile_visits", C.c_int64), ("max_delta", C.c_int32), ("connectivity", C.c_int32), ("rounds", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


class WatershedOpts(C.Structure):
    """pnr_watershed_opts (include/pnr_hip.h): thr -1..255 (-1: the global mean; 0: every voxel is in the mask), connectivity 0 (26), 4, 8, 6 or 26"""
    _fields_ = [("thr", C.c_int32), ("connectivity", C.c_int32)]


class WatershedInfo(C.Structure):
    """pnr_watershed_info: the exact summary of a watershed (the visits and rounds of the two passes: scheduling, a property of the implementation)"""
    _fields_ = [(k, C.c_int64) for k in ("n_vox", "n_mask", "n_marker_vox", "n_dropped", "n_reached", "n_unreached", "n_regions", "tiles", "flood_visits", "label_visits")] + [
        (k, C.c_int32) for k in ("m_max", "d_max", "thr_used", "connectivity", "flood_rounds", "label_rounds")]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class ThresholdOpts(C.Structure):
    """pnr_threshold_opts (include/pnr_hip.h): method 0..4 (THRESHOLD_METHODS), lo 0..255 (the counted bins are [lo, 255]), top_ppm 1..999999 for "top" and 0 otherwise"""
    _fields_ = [("method", C.c_int32), ("lo", C.c_int32), ("top_ppm", C.c_int32), ("pad", C.c_int32)]


class ThresholdInfo(C.Structure):
    """pnr_threshold_info: the threshold and the exact counts it was read from (v_min, v_max, peak: over the counted bins, -1 when they are empty)"""
    _fields_ = [("n_vox", C.c_int64), ("n_counted", C.c_int64), ("sum_counted", C.c_uint64), ("n_fg", C.c_int64)] + [
        (k, C.c_int32) for k in ("thr", "method", "lo", "v_min", "v_max", "peak")]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["method"] = THRESHOLD_NAMES[self.method]
        return d


THRESHOLD_METHODS = {"mean": 0, "otsu": 1, "triangle": 2, "top": 3, "maxentropy": 4}
THRESHOLD_NAMES = {v: k for k, v in THRESHOLD_METHODS.items()}


def parse_threshold(word):
    """a threshold word -> (method name, lo, top_ppm or None): "mean", "otsu", "triangle", "maxentropy" or "topP" (the brightest P per cent,
    up to 4 decimals), each with an optional ":LO" (the counted bins are [LO, 255])"""
    name, sep, lo = str(word).partition(":")
    try:
        lo = int(lo) if sep else 0
        if name.startswith("top") and name != "top":
            ppm = int(round(float(name[3:]) * 1e4))
            return "top", lo, ppm
    except ValueError:
        name = None
    if name not in THRESHOLD_METHODS or name == "top":
        raise ValueError("threshold %r: a number, or mean, otsu, triangle, maxentropy or topP (P per cent), each with an optional :LO" % (word,))
    return name, lo, None


def _threshold_opts(method, lo, top_ppm):
    if isinstance(method, str) and method not in THRESHOLD_METHODS:
        raise ValueError("threshold: method %r, not one of %s" % (method, ", ".join(THRESHOLD_METHODS)))
    m = THRESHOLD_METHODS[method] if isinstance(method, str) else int(method)
    return ThresholdOpts(m, int(lo), int(top_ppm) if top_ppm is not None else 0, 0)


def threshold_from_hist(H, method, lo=0, top_ppm=None):
    """pnr_threshold_from_hist: the threshold rule of include/pnr_hip.h on 256 counts -> the info dict {n_vox, n_counted, sum_counted, n_fg,
    thr, method, lo, v_min, v_max, peak}.  method: "mean", "otsu", "triangle", "top" (with top_ppm, the brightest share in parts per
    million) or "maxentropy".  Pure host: needs no GPU."""
    H = np.ascontiguousarray(H, np.uint64).reshape(-1)
    if len(H) != 256:
        raise ValueError("threshold_from_hist: %d counts, not 256" % len(H))
    o = _threshold_opts(method, lo, top_ppm)
    info = ThresholdInfo()
    check(load().pnr_threshold_from_hist(H.ctypes.data, C.byref(o), C.byref(info)))
    return info.as_dict()


class LocalOpts(C.Structure):
    """pnr_local_opts (include/pnr_hip.h): r 1..64, offset -255..255, scale_256 0..4096, floor 1..255, binary 0 / 1"""
    _fields_ = [(k, C.c_int32) for k in ("r", "offset", "scale_256", "floor", "binary", "pad")]


class LocalInfo(C.Structure):
    """pnr_local_info: the exact counts of a local threshold and the half-widths of its box"""
    _fields_ = [("n_vox", C.c_int64), ("n_kept", C.c_int64), ("sum_in", C.c_uint64), ("sum_out", C.c_uint64)] + [(k, C.c_int32) for k in ("rx", "ry", "rz", "pad")]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


class PruneOpts(C.Structure):
    """pnr_prune_opts (include/pnr_hip.h): zscale > 0, min_length, radius_factor and min_tree >= 0 (xy voxels; all 0: nothing is removed)"""
    _fields_ = [(k, C.c_float) for k in ("zscale", "min_length", "radius_factor", "min_tree")]


class PruneInfo(C.Structure):
    """pnr_prune_info: the exact summary of a pruning (lengths in units of 1/256 xy voxel; rounds_up / rounds_down: launches of the two
    jumping loops on the GPU, 0 on the host)"""
    _fields_ = ([(k, C.c_int64) for k in ("n", "n_roots", "n_leaves", "n_branch", "n_segments", "n_removed", "n_removed_segments", "n_removed_trees")] +
                [("length_in", C.c_uint64), ("length_out", C.c_uint64), ("h_max", C.c_uint32)] + [(k, C.c_int32) for k in ("order_max", "rounds_up", "rounds_down")])

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


PNR_LOCAL_MAX_R = 64


MORPH_OPS = {"dilate": 1, "erode": 2, "fill": 3, "hmax": 4, "hdome": 5}


def _morph_op(op):
    """a name of MORPH_OPS, or the number itself (the library checks its range)"""
    if isinstance(op, str) and op not in MORPH_OPS:
        raise ValueError("morph: op %r, not one of %s" % (op, ", ".join(MORPH_OPS)))
    return MORPH_OPS[op] if isinstance(op, str) else int(op)


# pnr_geo_bridge: the attachment nodes, the meet voxel p and offset o (13..25 of the offset order), the weight W and the bridge's voxel chain
GEO_BRIDGE = np.dtype([("a", np.int32), ("b", np.int32), ("p", np.int64), ("o", np.int32), ("path_len", np.int32), ("w", np.uint64), ("path_off", np.int64)])


# pnr_component
COMPONENT_DT = np.dtype([(k, np.int64) for k in ("first", "size", "sum", "sx", "sy", "sz")] + [(k, np.int32) for k in ("x0", "y0", "z0", "x1", "y1", "z1", "vmax", "pad")])


class Params(C.Structure):
    _fields_ = [("sig", C.c_float * PNR_MAX_SIGMAS), ("nsig", C.c_int), ("somaradius", C.c_int), ("tolerance", C.c_float),
                ("znccth", C.c_float), ("kappa", C.c_float), ("step", C.c_int), ("ni", C.c_int), ("np", C.c_int),
                ("zdist", C.c_float), ("nodepervol", C.c_int), ("vol", C.c_int), ("Kc", C.c_float),
                ("neff_ratio", C.c_float), ("alpha", C.c_float), ("beta", C.c_float), ("C", C.c_float),
                ("rng_seed", C.c_uint32), ("max_trace_count", C.c_int)]


SEED_DT = np.dtype([(k, "f4") for k in ("x", "y", "z", "vx", "vy", "vz", "score", "corr")])
XEST_DT = np.dtype([(k, "f4") for k in ("x", "y", "z", "vx", "vy", "vz", "sig", "corr")])
NODE_DT = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("vx", "f4"), ("vy", "f4"), ("vz", "f4"), ("corr", "f4"),
                    ("sig", "f4"), ("type", "i4")])


class PnrError(RuntimeError):
    pass


# pnr_allgather_fn / pnr_trace_fn (include/pnr_hip.h)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
TRACE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p)


def build(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(HERE, "csrc")
    if force:
        subprocess.run(["make", "-s", "-C", src, "clean"], check=True)
    subprocess.run(["make", "-s", "-j4", "-C", src], check=True)
    return LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PnrError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the PNR hot path)")
    # A process must not end up with two HIP runtimes (torch wheels bundle their own libamdhip64): if torch is
    # around, let it load its runtime first so that libpnr_hip.so binds to the same one.
    if not os.environ.get("PNR_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise PnrError(f"libpnr_hip error {rc}: {load().pnr_last_error().decode()}")


def make_params(sigmas=(2, 4, 6), somaradius=0, tolerance=5, znccth=0.3, kappa=3, step=2, ni=200, np_=20, zdist=2,
                nodepervol=4, vol=1, rng_seed=42, **const):
    p = Params()
    load().pnr_default_params(C.byref(p))
    sig = sorted(float(s) for s in sigmas)  # parse_csv_string sorts (Advantra_plugin.cpp:1885-1897)
    if len(sig) > PNR_MAX_SIGMAS:
        raise PnrError("too many sigmas")
    for i, s in enumerate(sig):
        p.sig[i] = s
    p.nsig = len(sig)
    p.somaradius, p.tolerance, p.znccth, p.kappa = somaradius, tolerance, znccth, kappa
    p.step, p.ni, p.np, p.zdist, p.nodepervol, p.vol, p.rng_seed = step, ni, np_, zdist, nodepervol, vol, rng_seed
    for k, v in const.items():
        setattr(p, k, v)
    return p


# pnr_phased_likelihood (include/pnr_hip_test.h): modes and the flag words it returns
PHL_FIRST, PHL_REGULAR, PHL_TAIL = 0, 1, 2
PHL_OX, PHL_OY, PHL_OZ, PHL_Y0, PHL_Y1, PHL_Z0, PHL_Z1, PHL_FAST, PHL_NCH = 5, 6, 7, 8, 9, 10, 11, 12, 13
# pnr_phased_decide: the flag words it reads and writes besides, and its two argument blocks
PHL_RES, PHL_STOP, PHL_T, PHL_IT, PHL_DONE, PHL_PAUSE = 0, 1, 2, 3, 4, 14
PHD_IN = ("flags", "seeds", "part", "prior", "idxres", "xcs", "corr", "cmap", "draws", "den")
PHD_OUT = ("part_u", "neff", "xcs_u", "oxc", "oT", "ostop", "idxres_u", "prior_u", "flags_u", "cnt_next", "list_next",
           "part_p", "prior_p", "flags_p", "uidx", "cmap_p", "cnt_p")


class PhdIn(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in PHD_IN] + [("lp", C.c_int32), ("mode", C.c_int32)]


class PhdOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in PHD_OUT]


# The C boundary, one entry per function: name -> (restype, argtypes).  load() binds exactly these, and the export lists are their keys.
_vp, _i64, _i32, _f32, _str, _rc = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_char_p, C.c_int
_pi64, _pi32, _pf32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
_volume_u16 = [_vp, _vp, _i64, _i64, _i64, _i32, _i32, C.POINTER(Window), _pi32, _pi32]
_seed_filter = [_vp, _vp, _i64, _pi64]
_graph_out = [_vp, _i64, _pi64, _vp, _i64, _pi64]  # nodes, cap_nodes, n_nodes, links, cap_links, n_links
_recon_in = [_vp, _i64, _vp, _i64, _f32, _f32, _i32, _f32, _f32, _i32]  # nodes, links, the five constants, tree_size_min or stage
_playback = [C.POINTER(Params), _i64, _i64, _i64, _vp, _i64, _i32, _i32, ALLGATHER_FN, _vp, _i64, TRACE_FN, _vp, _i32, _i32, _i32, _i32, _i32]
# the drop-in boundary (include/pnr_hip.h)
PRODUCT_SIGNATURES = {
    "pnr_last_error": (_str, []),
    "pnr_default_params": (None, [C.POINTER(Params)]),
    "pnr_create": (_rc, [C.POINTER(Params), _i32, C.POINTER(_vp)]),
    "pnr_destroy": (None, [_vp]),
    "pnr_set_stream": (_rc, [_vp, _vp]),
    "pnr_synchronize": (_rc, [_vp]),
    "pnr_set_volume": (_rc, [_vp, _vp, _i64, _i64, _i64]),
    "pnr_set_volume_device": (_rc, [_vp, _vp, _i64, _i64, _i64]),
    "pnr_set_volume_u16": (_rc, _volume_u16),
    "pnr_set_volume_u16_device": (_rc, _volume_u16),
    "pnr_get_volume": (_rc, [_vp, _vp]),
    "pnr_measure_radii": (_rc, [_vp, _vp, _i64, C.POINTER(RadiusOpts), _vp, _pi32]),
    "pnr_filter_volume": (_rc, [_vp, C.POINTER(FilterOpts)]),
    "pnr_point_segment_distance": (_rc, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "pnr_tree_sample": (_rc, [_vp, _vp, _i64, _f32, _f32, _vp, _vp, _i64, _pi64]),
    "pnr_tree_distance": (_rc, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, C.POINTER(DistanceOpts), C.POINTER(DistanceResult), _vp, _vp, _i64, _vp, _vp, _i64]),
    "pnr_nearest_other": (_rc, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "pnr_join_trees": (_rc, [_vp, _vp, _vp, _i64, C.POINTER(JoinOpts), _vp, _vp, _vp, _vp, _i64, _pi64, _pi64, _pi64]),
    "pnr_join_reroot": (_rc, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    "pnr_render_tree": (_rc, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, C.POINTER(RenderOpts), _vp, _vp]),
    "pnr_tree_coverage": (_rc, [_vp, _vp, _vp, _vp, _i64, C.POINTER(RenderOpts), C.POINTER(Coverage), _vp, _vp, _vp, _vp, _vp]),
    "pnr_label_components": (_rc, [_vp, C.POINTER(ComponentsOpts), C.POINTER(ComponentsInfo), _vp, _vp, _i64]),
    "pnr_despeckle_volume": (_rc, [_vp, C.POINTER(ComponentsOpts), C.POINTER(ComponentsInfo)]),
    "pnr_distance_transform": (_rc, [_vp, C.POINTER(EdtOpts), C.POINTER(EdtInfo), _vp, _vp, _i64, _vp]),
    "pnr_skeletonize": (_rc, [_vp, C.POINTER(ThinOpts), C.POINTER(ThinInfo), _vp, _vp, _vp, _i64]),
    "pnr_skeleton_forest": (_rc, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _pi64]),
    "pnr_geodesic_distance": (_rc, [_vp, _vp, _vp, _i64, C.POINTER(GeoOpts), C.POINTER(GeoInfo), _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp]),
    "pnr_geodesic_bridges": (_rc, [_vp, _vp, _vp, _i64, C.POINTER(GeoJoinOpts), C.POINTER(GeoJoinInfo), _vp, _i64, _pi64, _vp, _i64, _pi64]),
    "pnr_join_expand": (_rc, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _pi64, _vp]),
    "pnr_morph_reconstruct": (_rc, [_vp, C.POINTER(MorphOpts), _vp, C.POINTER(MorphInfo), _vp]),
    "pnr_morph_volume": (_rc, [_vp, C.POINTER(MorphOpts), C.POINTER(MorphInfo)]),
    "pnr_watershed": (_rc, [_vp, C.POINTER(WatershedOpts), _vp, _vp, _vp, _vp, _i64, C.POINTER(WatershedInfo), _vp, _vp]),
    "pnr_threshold_from_hist": (_rc, [_vp, C.POINTER(ThresholdOpts), C.POINTER(ThresholdInfo)]),
    "pnr_auto_threshold": (_rc, [_vp, C.POINTER(ThresholdOpts), C.POINTER(ThresholdInfo), _vp]),
    "pnr_local_threshold": (_rc, [_vp, C.POINTER(LocalOpts), C.POINTER(LocalInfo), _vp]),
    "pnr_local_threshold_volume": (_rc, [_vp, C.POINTER(LocalOpts), C.POINTER(LocalInfo)]),
    "pnr_prune_tree": (_rc, [_vp, _vp, _vp, _vp, _i64, C.POINTER(PruneOpts), C.POINTER(PruneInfo), _vp, _vp, _vp, _vp, _vp]),
    "pnr_prune_tree_host": (_rc, [_vp, _vp, _vp, _i64, C.POINTER(PruneOpts), C.POINTER(PruneInfo), _vp, _vp, _vp, _vp, _vp]),
    "pnr_prune_apply": (_rc, [_vp, _vp, _i64, _vp, _vp, _pi64]),
    "pnr_frangi": (_rc, [_vp, _pf32, _pf32]),
    "pnr_frangi_slab": (_rc, [_vp, _i64, _i64, _pf32, _pf32]),
    "pnr_quantise_j8": (_rc, [_vp, _f32, _f32]),
    "pnr_get_frangi": (_rc, [_vp] + [_vp] * 5),
    "pnr_extract_seeds": (_rc, [_vp, C.POINTER(_vp), _pi64]),
    "pnr_extract_seeds_range": (_rc, [_vp, _i64, _i64, C.POINTER(_vp), _pi64]),
    "pnr_zncc_batch": (_rc, [_vp, _vp, _i64, _vp, _vp]),
    "pnr_score_filter_sort_seeds": (_rc, _seed_filter),
    "pnr_score_filter_seeds": (_rc, _seed_filter),
    "pnr_sort_seeds": (_rc, _seed_filter),
    "pnr_trace_batch": (_rc, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "pnr_soma": (_rc, [_vp, _vp, _pi32, _pi64]),
    "pnr_get_soma": (_rc, [_vp, _vp, _i64, _pi64, _vp, _vp, _i64, _pi64]),
    "pnr_replay_traces": (_rc, [C.POINTER(Params), _i64, _i64, _i64, _vp, _i64, _vp, _vp] + _graph_out + [_pi64]),
    "pnr_replay_traces_ctx": (_rc, [_vp, _vp, _i64, _vp, _vp] + _graph_out + [_pi64]),
    "pnr_trace_replay": (_rc, [_vp, _vp, _i64, _i64] + _graph_out + [_pi64, _pi64]),
    "pnr_trace_replay_sharded": (_rc, [_vp, _vp, _i64, _i32, _i32, ALLGATHER_FN, _vp] + _graph_out + [_pi64, _pi64]),
    "pnr_get_graph": (_rc, [_vp] + _graph_out),
    "pnr_get_trace_log": (_rc, [_vp, _vp, _i64, _pi64]),
    "pnr_reconstruct": (_rc, _recon_in + [_vp, _vp, _i64, _pi64]),
    "pnr_reconstruct_ctx": (_rc, [_vp] + _recon_in + [_vp, _vp, _i64, _pi64]),
    "pnr_reconstruct_stage": (_rc, _recon_in + _graph_out),
    "pnr_set_profiling": (_rc, [_vp, _i32]),
    "pnr_set_smc_driver": (_rc, [_vp, _i32]),
    "pnr_get_kernel_ms": (_rc, [_vp, _str, C.POINTER(C.c_double), _pi64]),
    "pnr_reset_kernel_ms": (_rc, [_vp]),
    "pnr_set_option": (_rc, [_vp, _str, _i64]),
    "pnr_get_option": (_rc, [_vp, _str, _pi64]),
    "pnr_shm_exchange_open": (_rc, [_str, _i32, _i32, _i64, C.POINTER(_vp)]),
    "pnr_shm_allgather": (_rc, [_vp, _vp, _vp, _i64]),
    "pnr_shm_exchange_close": (None, [_vp]),
    "pnr_rccl_unique_id": (_rc, [_vp]),
    "pnr_rccl_exchange_open": (_rc, [_vp, _i32, _i32, _i32, _i64, C.POINTER(_vp)]),
    "pnr_rccl_allgather": (_rc, [_vp, _vp, _vp, _i64]),
    "pnr_rccl_allreduce_minmax": (_rc, [_vp, _pf32, _pf32]),
    "pnr_rccl_exchange_close": (None, [_vp]),
}
# test taps (include/pnr_hip_test.h): single stages of the device code and the scheduler over a host engine, for tests/ only
TEST_SIGNATURES = {
    "pnr_gaussian": (_rc, [_vp, _f32, _vp]),
    "pnr_hessian": (_rc, [_vp, _f32] + [_vp] * 6),
    "pnr_set_j8_v": (_rc, [_vp] + [_vp] * 4),
    "pnr_get_frangi_box": (_rc, [_vp, _vp, _vp] + [_vp] * 5),
    "pnr_get_table": (_rc, [_vp, _str, _vp, _i64, _pi64]),
    "pnr_expf_batch": (_rc, [_vp, _vp, _i64, _vp]),
    "pnr_eigen_batch": (_rc, [_vp, _vp, _i64, _vp, _vp]),
    "pnr_sched_playback": (_rc, _playback + _graph_out + [_pi64, _pi64]),
    "pnr_sched_playback2": (_rc, _playback + [_i32, _i32, _i32] + _graph_out + [_pi64, _pi64]),
    "pnr_reconstruct_stage_ctx": (_rc, [_vp] + _recon_in + _graph_out),
    "pnr_radius_offsets": (_rc, [_f32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _pi64]),
    "pnr_pair_tiles": (_rc, [_i64, _i64, _i64, _i64, _vp, _i64, _pi64]),
    "pnr_live_bytes": (_rc, [_pi64, _pi64]),
    "pnr_render_items": (_rc, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, C.POINTER(RenderOpts), _i64, _i64, _vp, _i64, _pi64]),
    "pnr_test_write_tiff": (_rc, [_str, _vp, _i64, _i64, _i64]),
    "pnr_test_histogram": (_rc, [_vp, _vp, _i64, _i32, _vp]),
    "pnr_test_local_threshold": (_rc, [_vp, _vp, _i64, _i64, _i64, C.POINTER(LocalOpts), C.POINTER(LocalInfo), _vp]),
    "pnr_seed_handover": (_rc, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _pi64, _vp, _vp]),
    "pnr_phased_likelihood": (_rc, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pnr_phased_decide": (_rc, [_vp, _i64, C.POINTER(PhdIn), C.POINTER(PhdOut)]),
}
SIGNATURES = {**PRODUCT_SIGNATURES, **TEST_SIGNATURES}
PRODUCT_EXPORTS, TEST_EXPORTS, EXPORTS = list(PRODUCT_SIGNATURES), list(TEST_SIGNATURES), list(SIGNATURES)


# what a new Context starts with (tests run every case with both SMC drivers by patching this; the library itself reads no
# environment variable): {"smc_driver": "phased" | "persistent", "options": {key: value}}
DEFAULTS = {"smc_driver": None, "options": {}}


class Context:
    """One GPU worth of PNR hot path (pnr_ctx)."""

    def __init__(self, params, device=0):
        self.L = load()
        self.p = params
        h = C.c_void_p()
        check(self.L.pnr_create(C.byref(params), device, C.byref(h)))
        self.h = h
        self.device = device
        self.shape = None
        self.window = None  # (lo, hi) of the last 16-bit set_volume
        self._keep = None
        if DEFAULTS.get("smc_driver"):
            self.set_smc_driver(DEFAULTS["smc_driver"])
        for k, v in (DEFAULTS.get("options") or {}).items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "h", None):
            self.L.pnr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- volume ----
    def set_volume(self, img, channel=0, window=None):
        """u8 (l, h, w): traced as it is.  uint16 (l, h, w) or (l, h, w, c) with the channels interleaved: channel `channel` is
        windowed to 8 bits on the GPU (pnr_set_volume_u16; `window` see make_window) and ctx.window is the (lo, hi) it used.  A u8
        (l, h, w, c) stack only selects its channel; 8-bit input is never windowed."""
        if isinstance(img, np.ndarray) and img.dtype.kind == "u" and img.dtype.itemsize == 2:
            img = np.ascontiguousarray(img, np.uint16)
            l, h, w, nc = img.shape if img.ndim == 4 else (*img.shape, 1)
            self._set_u16(self.L.pnr_set_volume_u16, img.ctypes.data, (l, h, w), nc, channel, window)
            return
        if window is not None:
            raise PnrError("8-bit input is never windowed (window / saturate need a 16-bit stack)")
        if isinstance(img, np.ndarray) and img.ndim == 4:
            img = img[..., channel]
        img = np.ascontiguousarray(img, np.uint8)
        l, h, w = img.shape
        check(self.L.pnr_set_volume(self.h, img.ctypes.data, w, h, l))
        self.shape = (l, h, w)
        self.window = None

    def set_volume_device(self, data_ptr, shape, keepalive=None, dtype=np.uint8, nchan=1, channel=0, window=None):
        """a device pointer (e.g. a torch tensor's data_ptr()): u8 is borrowed until the next set_volume; uint16 (nchan samples per
        voxel, interleaved) is windowed into the context's own 8-bit volume during the call"""
        l, h, w = shape
        if np.dtype(dtype) == np.uint16:
            self._set_u16(self.L.pnr_set_volume_u16_device, data_ptr, (l, h, w), nchan, channel, window)
            self._keep = None
            return
        if window is not None or nchan != 1:
            raise PnrError("8-bit device input: one channel, never windowed")
        check(self.L.pnr_set_volume_device(self.h, data_ptr, w, h, l))
        self.shape = (l, h, w)
        self.window = None
        self._keep = keepalive

    def _set_u16(self, fn, ptr, shape, nchan, channel, window):
        l, h, w = shape
        win = make_window(window)
        lo, hi = C.c_int32(), C.c_int32()
        check(fn(self.h, ptr, w, h, l, int(nchan), int(channel), C.byref(win) if win is not None else None, C.byref(lo), C.byref(hi)))
        self.shape = (l, h, w)
        self.window = (lo.value, hi.value)

    def get_volume(self):
        """the 8-bit volume the context traces (pnr_get_volume)"""
        out = np.empty(self.shape, np.uint8)
        check(self.L.pnr_get_volume(self.h, out.ctypes.data))
        return out

    def filter_volume(self, median=0, tophat=0):
        """pnr_filter_volume: the traced volume is replaced by its 3 x 3 (median = 2) or 3 x 3 x 3 (median = 3) median, then by its
        top-hat with the flat box of half-width `tophat` (1..64; the z half-width is int(tophat / zdist)); 0 skips a stage.  The
        result is an owned volume (a borrowed one is left as it was and released) and the later pipeline state is invalidated."""
        o = FilterOpts(int(median), int(tophat))
        check(self.L.pnr_filter_volume(self.h, C.byref(o)))
        if o.median or o.tophat_r:
            self._keep = None

    def measure_radii(self, xyz, thr=-1, rel_pct=50, rmax=32, bg_permille=1):
        """pnr_measure_radii at n x 3 positions (x, y, z) on the context's volume -> (k int32[n], thr_used): k = the measured radius
        in xy voxels (0: thinner than one voxel, -1: a position that is not finite); thr_used = the threshold of the absolute mode
        (rel_pct = 0; thr = -1: the global mean), 0 in the relative mode"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        k = np.empty(len(xyz), np.int32)
        o = RadiusOpts(self._thr(thr), int(rel_pct), int(rmax), int(bg_permille))
        t = C.c_int32()
        check(self.L.pnr_measure_radii(self.h, xyz.ctypes.data, len(xyz), C.byref(o), k.ctypes.data, C.byref(t)))
        return k, t.value

    def point_segment_distance(self, pts, a, b):
        """pnr_point_segment_distance: n x 3 points against the m segments (a[j], b[j]) -> (d float32[n], j int32[n]): the distance to
        the nearest segment and the smallest index of a segment at that distance"""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
        if len(a) != len(b):
            raise PnrError("point_segment_distance: a and b differ in length")
        d = np.empty(len(pts), np.float32)
        j = np.empty(len(pts), np.int32)
        check(self.L.pnr_point_segment_distance(self.h, pts.ctypes.data, len(pts), a.ctypes.data, b.ctypes.data, len(a), d.ctypes.data, j.ctypes.data))
        return d, j

    def tree_distance(self, xyzA, parentA, xyzB, parentB, zscale=1, step=1, thr=2, per_point=False):
        """pnr_tree_distance of two trees (n x 3 positions, parent indices with a negative value for none; drop the dummy node of a
        reconstruct() result first) -> the result as a dict {"ab", "ba": {n, n_big, mean, ssd, pct, max}, sd, ssd, pct, hausdorff};
        per_point: -> (dict, (dA, ownerA), (dB, ownerB)) with the distance and the node of every sample point of A and of B"""
        xa = np.ascontiguousarray(xyzA, np.float32).reshape(-1, 3)
        xb = np.ascontiguousarray(xyzB, np.float32).reshape(-1, 3)
        pa = np.ascontiguousarray(parentA, np.int32).reshape(-1)
        pb = np.ascontiguousarray(parentB, np.int32).reshape(-1)
        if len(pa) != len(xa) or len(pb) != len(xb):
            raise PnrError("tree_distance: one parent per node")
        o = DistanceOpts(float(zscale), float(step), float(thr))
        r = DistanceResult()
        out = [None] * 4
        if per_point:
            na, nb = (tree_sample(x, p, zscale, step, count_only=True) for x, p in ((xa, pa), (xb, pb)))
            out = [np.empty(na, np.float32), np.empty(na, np.int32), np.empty(nb, np.float32), np.empty(nb, np.int32)]
        ptr = [v.ctypes.data if v is not None else None for v in out]
        check(self.L.pnr_tree_distance(self.h, xa.ctypes.data, pa.ctypes.data, len(xa), xb.ctypes.data, pb.ctypes.data, len(xb), C.byref(o), C.byref(r),
                                       ptr[0], ptr[1], len(out[0]) if per_point else 0, ptr[2], ptr[3], len(out[2]) if per_point else 0))
        return (r.as_dict(), (out[0], out[1]), (out[2], out[3])) if per_point else r.as_dict()

    def nearest_other(self, xyz, label):
        """pnr_nearest_other: for every point with label >= 0 the nearest point of another non-negative label -> (d float32[n], j int32[n]):
        its distance and the smallest index at that distance; (+inf, -1) without one and for a negative label"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        label = np.ascontiguousarray(label, np.int32).reshape(-1)
        if len(label) != len(xyz):
            raise PnrError("nearest_other: one label per point")
        d = np.empty(len(xyz), np.float32)
        j = np.empty(len(xyz), np.int32)
        check(self.L.pnr_nearest_other(self.h, xyz.ctypes.data, label.ctypes.data, len(xyz), d.ctypes.data, j.ctypes.data))
        return d, j

    def join_trees(self, xyz, parent, zscale=1, gap=0, root=-1, counts=False):
        """pnr_join_trees of a forest (n x 3 positions, parent indices with a negative value for none; drop the dummy node of a
        reconstruct() result first): fragments whose closest nodes lie within `gap` (0: any distance) are bridged, every component is
        re-rooted (at `root` where given) -> (parent int32[n], order int32[n], comp int32[n], bridges BRIDGE[k]); a file written in
        `order` has every parent before its children.  counts: a fifth item {"trees_in", "trees_out", "rounds"}"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        if len(parent) != len(xyz):
            raise PnrError("join_trees: one parent per node")
        n = len(xyz)
        o = JoinOpts(float(zscale), float(gap), int(root))
        out = [np.empty(n, np.int32) for _ in range(3)]
        nb, t0, t1 = C.c_int64(), C.c_int64(), C.c_int64()
        cap = 64
        while True:  # "*n_bridges > cap: call again"
            bridges = np.empty(cap, BRIDGE)
            check(self.L.pnr_join_trees(self.h, xyz.ctypes.data, parent.ctypes.data, n, C.byref(o), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                        bridges.ctypes.data, cap, C.byref(nb), C.byref(t0), C.byref(t1)))
            if nb.value <= cap:
                break
            cap = nb.value
        res = (out[0], out[1], out[2], bridges[:nb.value].copy())
        return res + ({"trees_in": t0.value, "trees_out": t1.value, "rounds": self.get_option("join_rounds")},) if counts else res

    def prune_tree(self, xyz, radius, parent, zscale=1, min_length=0, radius_factor=0, min_tree=0):
        """pnr_prune_tree of a forest (n x 3 positions, n radii in xy voxels or None, parent indices with a negative value for a root):
        a side branch shorter than max(min_length, radius_factor x its parent's radius) and a tree lower than min_tree (xy voxels) are
        removed by the rule of include/pnr_hip.h -> (info dict, keep uint8[n], height uint32[n], path uint32[n], order int32[n], seg
        int32[n]); the lengths in units of 1/256 xy voxel.  All three at 0: the morphometry alone.  Needs no volume."""
        return _prune_call(lambda *a: self.L.pnr_prune_tree(self.h, *a), "prune_tree", xyz, radius, parent, zscale, min_length, radius_factor, min_tree)

    def render_tree(self, xyz, radius, parent, shape, zscale=1, rscale=1, radd=0, labels=True, mask=False):
        """pnr_render_tree of a tree (n x 3 positions, n radii in xy voxels, parent indices with a negative value for none) on the grid
        shape = (l, h, w) -> labels int32[l, h, w] (1 + the smallest node whose segment to its parent holds the voxel, 0: none), or the
        mask uint8[l, h, w] (255 under the tree), or (labels, mask) when both are asked for.  Needs no volume."""
        xyz, radius, parent = _tree_arrays("render_tree", xyz, radius, parent)
        l, h, w = (int(v) for v in shape)
        o = RenderOpts(float(zscale), float(rscale), float(radd), -1)
        lab = np.empty((l, h, w), np.int32) if labels else None
        msk = np.empty((l, h, w), np.uint8) if mask else None
        check(self.L.pnr_render_tree(self.h, xyz.ctypes.data, radius.ctypes.data, parent.ctypes.data, len(xyz), w, h, l, C.byref(o),
                                     lab.ctypes.data if labels else None, msk.ctypes.data if mask else None))
        return (lab, msk) if labels and mask else lab if labels else msk

    def tree_coverage(self, xyz, radius, parent, zscale=1, rscale=1, radd=0, thr=-1, per_node=False, mask=False, residual=False):
        """pnr_tree_coverage: the tree rendered on the context's volume V -> a dict {n_vox, n_tree, n_fg, n_both, sum_fg, sum_both, thr_used,
        covered, on_signal, covered_intensity} (foreground: V >= thr; thr = -1: the global mean); per_node adds "seg_vox", "seg_fg",
        "seg_sum" (int64[n]: the voxels labelled with the node, the foreground among them, the sum of V over them), mask adds "mask"
        (uint8, 255 under the tree), residual adds "residual" (V where the tree is not, else 0)"""
        xyz, radius, parent = _tree_arrays("tree_coverage", xyz, radius, parent)
        o = RenderOpts(float(zscale), float(rscale), float(radd), self._thr(thr))
        cov = Coverage()
        out = {}
        if per_node:
            out.update({k: np.zeros(len(xyz), np.int64) for k in ("seg_vox", "seg_fg", "seg_sum")})
        if mask:
            out["mask"] = np.empty(self.shape, np.uint8)
        if residual:
            out["residual"] = np.empty(self.shape, np.uint8)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        check(self.L.pnr_tree_coverage(self.h, xyz.ctypes.data, radius.ctypes.data, parent.ctypes.data, len(xyz), C.byref(o), C.byref(cov), ptr("seg_vox"),
                                       ptr("seg_fg"), ptr("seg_sum"), ptr("mask"), ptr("residual")))
        return {**cov.as_dict(), **out}

    def label_components(self, thr=-1, connectivity=26, min_size=1, labels=True, cap=None):
        """pnr_label_components: the connected components of {V >= thr} (thr = -1: the global mean) of the context's volume under 6- or
        26-connectivity -> (info dict {n_vox, n_fg, n_comp, n_small, vox_small, largest, thr_used}, labels int32[l, h, w] or None,
        comps COMPONENT_DT[n_comp]).  The components of at least min_size voxels are numbered 1.. by their first voxel in raster order;
        label 0 is background and the dropped components.  cap: at most this many entries of comps (info["n_comp"] stays the full count)."""
        o = ComponentsOpts(self._thr(thr), int(connectivity), int(min_size))
        info = ComponentsInfo()
        lab = np.empty(self.shape, np.int32) if labels else None
        lp = lab.ctypes.data if labels else None
        if cap is None:  # count first, then fetch: "n_comp > cap: call again"
            check(self.L.pnr_label_components(self.h, C.byref(o), C.byref(info), lp, None, 0))
            comps = np.zeros(info.n_comp, COMPONENT_DT)
            if info.n_comp:
                check(self.L.pnr_label_components(self.h, C.byref(o), C.byref(info), None, comps.ctypes.data, len(comps)))
        else:
            comps = np.zeros(int(cap), COMPONENT_DT)
            check(self.L.pnr_label_components(self.h, C.byref(o), C.byref(info), lp, comps.ctypes.data, len(comps)))
            comps = comps[:min(len(comps), info.n_comp)]
        return info.as_dict(), lab, comps

    def despeckle(self, min_size, thr=-1, connectivity=26):
        """pnr_despeckle_volume: the foreground components ({V >= thr}, thr = -1: the global mean) of fewer than min_size voxels are set
        to 0 in the traced volume -> the info dict of label_components (n_small / vox_small: what was removed).  The result is an owned
        volume (a borrowed one is left as it was and released) and the later pipeline state is invalidated; min_size = 1 changes nothing."""
        o = ComponentsOpts(self._thr(thr), int(connectivity), int(min_size))
        info = ComponentsInfo()
        check(self.L.pnr_despeckle_volume(self.h, C.byref(o), C.byref(info)))
        if o.min_size > 1:
            self._keep = None
        return info.as_dict()

    def distance_transform(self, thr=-1, rmax=64, volume=True, points=None, squared=True):
        """pnr_distance_transform: the exact squared distance D2 of every voxel of {V >= thr} (thr = -1: the global mean) to the nearest
        background voxel inside the volume, in xy voxels with z counted zdist-fold, capped at rmax^2 -> (info dict {n_vox, n_fg, n_capped,
        first_max, d2_max, thr_used, d_max, max_at}, d2 float32[l, h, w] or None, at float32[n] or None).  points: n x 3 positions
        (x, y, z) -> D2 at their centre voxels (-1: a position that is not finite).  squared=False: the f32 square roots of both (and -1
        stays -1).  d_max = sqrt(d2_max); max_at = (x, y, z) of first_max, None without foreground."""
        o = EdtOpts(self._thr(thr), int(rmax))
        info = EdtInfo()
        d2 = np.empty(self.shape, np.float32) if volume else None
        xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3) if points is not None else None
        at = np.empty(len(xyz), np.float32) if xyz is not None else None
        check(self.L.pnr_distance_transform(self.h, C.byref(o), C.byref(info), d2.ctypes.data if volume else None,
                                            xyz.ctypes.data if xyz is not None and len(xyz) else None, len(xyz) if xyz is not None else 0,
                                            at.ctypes.data if at is not None and len(at) else None))
        out = info.as_dict()
        out["d_max"] = float(np.sqrt(np.float32(info.d2_max)))
        l, h, w = self.shape
        i = info.first_max
        out["max_at"] = (i % w, (i // w) % h, i // (w * h)) if i >= 0 else None
        if not squared:
            d2 = np.sqrt(d2) if volume else None
            if at is not None:
                at = np.where(at >= 0, np.sqrt(np.maximum(at, np.float32(0))), at).astype(np.float32)
        return out, d2, at

    def skeletonize(self, thr=-1, max_rounds=0, volume=True, voxels=True, cap=None):
        """pnr_skeletonize: {V >= thr} (thr = -1: the global mean) of the context's volume thinned to a one-voxel-wide curve skeleton under
        the rule of include/pnr_hip.h -> (info dict {n_vox, n_fg, n_skel, n_end, n_branch, n_isolated, tiles, tile_visits, rounds,
        thr_used}, skel uint8[l, h, w] of 0 / 255 or None, vox int64[n_skel] ascending linear indices or None, deg uint8[n_skel] the
        skeleton voxels in N26 or None).  max_rounds: stop after this many rounds (0: when nothing is deleted).  cap: at most this many
        entries of vox and deg (info["n_skel"] stays the full count)."""
        o = ThinOpts(self._thr(thr), int(max_rounds))
        info = ThinInfo()
        skel = np.empty(self.shape, np.uint8) if volume else None
        sp = skel.ctypes.data if volume else None
        if not voxels:
            check(self.L.pnr_skeletonize(self.h, C.byref(o), C.byref(info), sp, None, None, 0))
            return info.as_dict(), skel, None, None
        if cap is None:  # count first, then fetch
            check(self.L.pnr_skeletonize(self.h, C.byref(o), C.byref(info), None, None, None, 0))
            cap = info.n_skel
        vox, deg = np.zeros(max(int(cap), 0), np.int64), np.zeros(max(int(cap), 0), np.uint8)
        check(self.L.pnr_skeletonize(self.h, C.byref(o), C.byref(info), sp, vox.ctypes.data if len(vox) else None, deg.ctypes.data if len(deg) else None, int(cap)))
        k = min(len(vox), info.n_skel)
        return info.as_dict(), skel, vox[:k], deg[:k]

    def geodesic(self, sources, labels=None, thr=0, dmax=PNR_GEO_DMAX, cost=None, volume=True, targets=None, path_cap=0):
        """pnr_geodesic_distance: the gray-weighted geodesic distance D of every passable voxel (V >= thr; thr = -1: the global mean) to the
        nearest of the sources (n x 3 positions (x, y, z); labels int32 >= 0, None: 0 .. n - 1) along 26-connected paths whose steps cost
        len * (c(V(p)) + c(V(q))), c = cost (256 u16 >= 1; None: 256 - v), and the label L of that source -> (info dict {n_vox, n_pass,
        n_reached, n_src, n_src_dropped, first_max, d_max, thr_used, rounds, max_at}, D uint32[l, h, w] or None (0xFFFFFFFF: unreached),
        L int32[l, h, w] or None (-1: unreached), at or None).  targets: m x 3 positions -> at = {"d": uint32[m], "label": int32[m]} at
        their centre voxels, and with path_cap > 0 also {"path_len": int32[m], "paths": a list of m int64 arrays of linear voxel indices
        from the target to its source voxel}: path_len k > 0 is a complete path, 0 an unreached or non-finite target (an empty array),
        -path_cap a walk cut after path_cap voxels (those are in the array)."""
        src = np.ascontiguousarray(sources, np.float32).reshape(-1, 3)
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1) if labels is not None else None
        if lab is not None and len(lab) != len(src):
            raise ValueError("geodesic: %d labels for %d sources" % (len(lab), len(src)))
        tab = np.ascontiguousarray(cost, np.uint16).reshape(-1) if cost is not None else None
        if tab is not None and len(tab) != 256:
            raise ValueError("geodesic: the cost table has 256 entries")
        o = GeoOpts(self._thr(thr), int(dmax), tab.ctypes.data_as(C.POINTER(C.c_uint16)) if tab is not None else None)
        info = GeoInfo()
        D = np.empty(self.shape, np.uint32) if volume else None
        Lv = np.empty(self.shape, np.int32) if volume else None
        xyz = np.ascontiguousarray(targets, np.float32).reshape(-1, 3) if targets is not None else None
        m = len(xyz) if xyz is not None else 0
        cap = int(path_cap)
        d_at, l_at = (np.empty(m, np.uint32), np.empty(m, np.int32)) if xyz is not None else (None, None)
        plen = np.zeros(m, np.int32) if m and cap > 0 else None
        pvox = np.empty((m, cap), np.int64) if plen is not None else None
        check(self.L.pnr_geodesic_distance(self.h, src.ctypes.data if len(src) else None, lab.ctypes.data if lab is not None and len(lab) else None, len(src),
                                           C.byref(o), C.byref(info), D.ctypes.data if volume else None, Lv.ctypes.data if volume else None,
                                           xyz.ctypes.data if m else None, m, d_at.ctypes.data if m else None, l_at.ctypes.data if m else None,
                                           cap, plen.ctypes.data if plen is not None else None, pvox.ctypes.data if pvox is not None else None))
        out = info.as_dict()
        l, h, w = self.shape
        i = info.first_max
        out["max_at"] = (i % w, (i // w) % h, i // (w * h)) if i >= 0 else None
        at = None
        if xyz is not None:
            at = {"d": d_at, "label": l_at}
            if cap > 0:
                if plen is None:
                    plen = np.zeros(0, np.int32)
                at["path_len"] = plen
                at["paths"] = [pvox[k, :abs(int(n))].copy() for k, n in enumerate(plen)]
        return out, D, Lv, at

    def morph_reconstruct(self, marker=None, op="dilate", h=0, connectivity=0, volume=True):
        """pnr_morph_reconstruct: the grey-level morphological reconstruction of the context's volume V under the rule of include/pnr_hip.h
        -> (info dict {n_vox, n_changed, n_nonzero, sum_in, sum_out, tiles, tile_visits, max_delta, connectivity, rounds}, out uint8[l, h, w]
        or None).  op: "dilate" / "erode" (the reconstruction of `marker`, uint8 of V's size, by dilation / by erosion under V), "fill"
        (grey fill-holes), "hmax" (maxima of height below h removed), "hdome" (V minus the hmax volume); connectivity 0 (6 for fill, 26
        for the others), 4, 8, 6 or 26.  The context and its volume stay as they are."""
        m = None
        if marker is not None:
            m = np.ascontiguousarray(marker, np.uint8)
            if m.size != int(np.prod(self.shape)):
                raise ValueError("morph_reconstruct: a marker of %d voxels for a volume of %d" % (m.size, int(np.prod(self.shape))))
        o = MorphOpts(_morph_op(op), int(connectivity), int(h), 0)
        info = MorphInfo()
        out = np.empty(self.shape, np.uint8) if volume else None
        check(self.L.pnr_morph_reconstruct(self.h, C.byref(o), m.ctypes.data if m is not None else None, C.byref(info), out.ctypes.data if volume else None))
        return info.as_dict(), out

    def morph_volume(self, op, h=0, connectivity=0):
        """pnr_morph_volume: the traced volume is replaced by its "fill", "hmax" or "hdome" (see morph_reconstruct) -> the info dict.  The
        result is an owned volume (a borrowed one is left as it was and released) and the later pipeline state is invalidated."""
        o = MorphOpts(_morph_op(op), int(connectivity), int(h), 0)
        info = MorphInfo()
        check(self.L.pnr_morph_volume(self.h, C.byref(o), C.byref(info)))
        self._keep = None
        return info.as_dict()

    def watershed(self, markers=None, points=None, labels=None, relief=None, thr=-1, connectivity=26, volume=True, levels=False):
        """pnr_watershed: the marker-controlled watershed of the context's volume under the rule of include/pnr_hip.h -> (info dict {n_vox,
        n_mask, n_marker_vox, n_dropped, n_reached, n_unreached, n_regions, tiles, flood_visits, label_visits, m_max, d_max, thr_used,
        connectivity, flood_rounds, label_rounds}, L int32[l, h, w] or None, M uint8[l, h, w] or None).  The mask is V >= thr (-1: the
        global mean), the relief `relief` (uint8 of V's size; None: 255 - V).  The markers come in exactly one form: `markers`, an int32
        volume (> 0: a label, 0: none), or `points`, n x 3 positions (x, y, z) with `labels` (>= 1; None: 1 .. n).  L: the label of every
        reached voxel, 0 elsewhere; M (levels=True): the pass height at which a voxel joined its region, 0 where none did.  The context
        and its volume stay as they are."""
        n = int(np.prod(self.shape))
        mv = xyz = lab = rel = None
        if markers is not None:
            mv = np.ascontiguousarray(markers, np.int32)
            if mv.size != n:
                raise ValueError("watershed: a marker volume of %d voxels for a volume of %d" % (mv.size, n))
        if points is not None:
            xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        if labels is not None:
            lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
            if xyz is None or len(lab) != len(xyz):
                raise ValueError("watershed: %d labels for %d points" % (len(lab), len(xyz) if xyz is not None else 0))
        if relief is not None:
            rel = np.ascontiguousarray(relief, np.uint8)
            if rel.size != n:
                raise ValueError("watershed: a relief of %d voxels for a volume of %d" % (rel.size, n))
        o = WatershedOpts(self._thr(thr), int(connectivity))
        info = WatershedInfo()
        Lv = np.empty(self.shape, np.int32) if volume else None
        Mv = np.empty(self.shape, np.uint8) if levels else None
        check(self.L.pnr_watershed(self.h, C.byref(o), rel.ctypes.data if rel is not None else None, mv.ctypes.data if mv is not None else None,
                                   xyz.ctypes.data if xyz is not None and len(xyz) else None, lab.ctypes.data if lab is not None and len(lab) else None,
                                   len(xyz) if xyz is not None else 0, C.byref(info), Lv.ctypes.data if volume else None, Mv.ctypes.data if levels else None))
        return info.as_dict(), Lv, Mv

    def split_touching(self, h, thr=-1, rmax=64, scale=4, connectivity=26):
        """Touching cells of {V >= thr} parted along their necks: the classical chain distance transform -> extended maxima -> markers ->
        watershed, each stage one call of this library, the volumes passing through the host between them (four downloads and three
        uploads of N voxels; a device-resident chain does not exist):
          1. D2 = distance_transform(thr, rmax);  2. the thickness map Q = min(255, floor(scale * sqrt(D2))) in f32 single operations;
          3. on a second context of the same device that holds Q: morph_volume("hmax", h), then morph_reconstruct(op="hdome", h=1) -- its
             voxels > 0 are the extended maxima of Q, the cores that stand at least h above their necks;
          4. label_components(thr=1, connectivity=26) of those cores: the markers;
          5. watershed(relief=255 - Q, markers, thr, connectivity) on this context.
        -> (info dict of the watershed, labels int32[l, h, w], n_cells = the number of markers).  h in 1..255 is in units of Q."""
        thr = self._thr(thr)
        _, d2, _ = self.distance_transform(thr=thr, rmax=rmax)
        q = np.minimum(np.float32(255), np.floor(np.float32(scale) * np.sqrt(d2, dtype=np.float32), dtype=np.float32)).astype(np.uint8)
        other = Context(self.p, self.device)
        try:
            other.set_volume(q)
            other.morph_volume("hmax", h=int(h), connectivity=26)
            _, dome = other.morph_reconstruct(op="hdome", h=1, connectivity=26)
            other.set_volume(dome)  # (0 or 1)
            cinfo, markers, _ = other.label_components(thr=1, connectivity=26)
        finally:
            other.close()
        info, lab, _ = self.watershed(markers=markers, relief=(255 - q).astype(np.uint8), thr=thr, connectivity=connectivity)
        return info, lab, int(cinfo["n_comp"])

    def join_trees_geodesic(self, xyz, parent, limit=0, thr=0, step=1, cost=None):
        """pnr_geodesic_bridges of a forest (n x 3 voxel positions, parent indices with a negative value for none) through the context's
        volume: the unique minimum spanning forest of the fragments under gray-weighted path cost (bridges heavier than `limit` are not
        made; 0: no limit; thr, cost as in geodesic(); step: the spacing of the sources along the segments) -> (bridges GEO_BRIDGE[k] in
        ascending key order, paths {"vox": int64[...] the bridges' voxel chains s_a .. p, q .. s_b one after the other (bridge k:
        vox[path_off : path_off + path_len]), "shape": (l, h, w)}, info dict {n_trees_in, n_trees_lost, n_trees_out, n_bridges,
        n_inserted, n_src, n_src_dropped, w_max, thr_used, rounds}).  join_expand() turns the result into nodes for join_reroot()."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        if len(parent) != len(xyz):
            raise PnrError("join_trees_geodesic: one parent per node")
        tab = np.ascontiguousarray(cost, np.uint16).reshape(-1) if cost is not None else None
        if tab is not None and len(tab) != 256:
            raise ValueError("join_trees_geodesic: the cost table has 256 entries")
        o = GeoJoinOpts(self._thr(thr), int(limit), float(step), tab.ctypes.data_as(C.POINTER(C.c_uint16)) if tab is not None else None)
        info = GeoJoinInfo()
        nb, npath = C.c_int64(), C.c_int64()
        cap_b, cap_p = 64, 4096
        while True:  # "*n_bridges > cap_bridges or *n_path > cap_path: call again"
            bridges = np.empty(cap_b, GEO_BRIDGE)
            vox = np.empty(cap_p, np.int64)
            check(self.L.pnr_geodesic_bridges(self.h, xyz.ctypes.data, parent.ctypes.data, len(xyz), C.byref(o), C.byref(info), bridges.ctypes.data, cap_b, C.byref(nb),
                                              vox.ctypes.data, cap_p, C.byref(npath)))
            if nb.value <= cap_b and npath.value <= cap_p:
                break
            cap_b, cap_p = max(cap_b, nb.value), max(cap_p, npath.value)
        return bridges[:nb.value].copy(), {"vox": vox[:npath.value].copy(), "shape": tuple(int(v) for v in self.shape)}, info.as_dict()

    def auto_threshold(self, method="otsu", lo=0, top_ppm=None, hist=False):
        """pnr_auto_threshold: the threshold of the context's volume under the rule of include/pnr_hip.h, from one histogram pass on the GPU
        -> the info dict of threshold_from_hist, or (info, H uint64[256]) with hist=True.  The context stays as it is."""
        o = _threshold_opts(method, lo, top_ppm)
        info = ThresholdInfo()
        H = np.zeros(256, np.uint64) if hist else None
        check(self.L.pnr_auto_threshold(self.h, C.byref(o), C.byref(info), H.ctypes.data if hist else None))
        return (info.as_dict(), H) if hist else info.as_dict()

    def _thr(self, thr):
        """the thr of a tool: a number as it is (-1: the tool's own mean rule), or a threshold word (parse_threshold) resolved by
        auto_threshold on the context's current volume"""
        if not isinstance(thr, str):
            return int(thr)
        method, lo, ppm = parse_threshold(thr)
        return self.auto_threshold(method, lo, ppm)["thr"]

    def local_threshold(self, r, offset=0, scale_256=256, floor=1, binary=False, volume=True):
        """pnr_local_threshold: a voxel is kept where V >= floor and 256 n V >= scale_256 S + 256 offset n, with n and S the size and the
        sum of the box (r, r, int(r / zdist)) around it cut to the volume; out = V (255 with binary) where kept, else 0 -> (info dict
        {n_vox, n_kept, sum_in, sum_out, rx, ry, rz}, out uint8[l, h, w] or None).  The context and its volume stay as they are."""
        o = LocalOpts(int(r), int(offset), int(scale_256), int(floor), int(bool(binary)), 0)
        info = LocalInfo()
        out = np.empty(self.shape, np.uint8) if volume else None
        check(self.L.pnr_local_threshold(self.h, C.byref(o), C.byref(info), out.ctypes.data if volume else None))
        return info.as_dict(), out

    def local_threshold_volume(self, r, offset=0, scale_256=256, floor=1, binary=False):
        """pnr_local_threshold_volume: the traced volume is replaced by its local threshold (see local_threshold) -> the info dict.  The
        result is an owned volume (a borrowed one is left as it was and released) and the later pipeline state is invalidated."""
        o = LocalOpts(int(r), int(offset), int(scale_256), int(floor), int(bool(binary)), 0)
        info = LocalInfo()
        check(self.L.pnr_local_threshold_volume(self.h, C.byref(o), C.byref(info)))
        self._keep = None
        return info.as_dict()

    def tap_histogram(self, data, offset=0):
        """pnr_test_histogram (test tap): the histogram kernel on the bytes `data`, `offset` bytes past a 16-byte boundary -> uint64[256]"""
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        H = np.zeros(256, np.uint64)
        check(self.L.pnr_test_histogram(self.h, data.ctypes.data, len(data), int(offset), H.ctypes.data))
        return H

    def tap_local_threshold(self, V, r, offset=0, scale_256=256, floor=1, binary=False):
        """pnr_test_local_threshold (test tap): local_threshold on the volume V (l, h, w) of any size -> (info dict, out)"""
        V = np.ascontiguousarray(V, np.uint8)
        l, h, w = V.shape
        o = LocalOpts(int(r), int(offset), int(scale_256), int(floor), int(bool(binary)), 0)
        info = LocalInfo()
        out = np.empty(V.shape, np.uint8)
        check(self.L.pnr_test_local_threshold(self.h, V.ctypes.data, w, h, l, C.byref(o), C.byref(info), out.ctypes.data))
        return info.as_dict(), out

    def set_stream(self, stream_ptr):
        check(self.L.pnr_set_stream(self.h, stream_ptr))

    def synchronize(self):
        check(self.L.pnr_synchronize(self.h))

    # ---- Frangi ----
    def frangi(self):
        a, b = C.c_float(), C.c_float()
        check(self.L.pnr_frangi(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def frangi_slab(self, z_keep0, z_keep1):
        """Frangi of a slab with halo: (Jmin, Jmax) over the kept planes only, J not yet quantised (pnr_frangi_slab)"""
        a, b = C.c_float(), C.c_float()
        check(self.L.pnr_frangi_slab(self.h, z_keep0, z_keep1, C.byref(a), C.byref(b)))
        return a.value, b.value

    def quantise_j8(self, jmin, jmax):
        check(self.L.pnr_quantise_j8(self.h, jmin, jmax))

    def get_frangi(self, J=True, J8=True, V=True):
        out = {}
        if J:
            out["J"] = np.empty(self.shape, np.float32)
        if J8:
            out["J8"] = np.empty(self.shape, np.uint8)
        if V:
            for k in ("Vx", "Vy", "Vz"):
                out[k] = np.empty(self.shape, np.uint8)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        check(self.L.pnr_get_frangi(self.h, ptr("J"), ptr("J8"), ptr("Vx"), ptr("Vy"), ptr("Vz")))
        return out

    def get_frangi_box(self, lo, hi, J=True, J8=True, V=True):
        """test tap pnr_get_frangi_box: get_frangi of the box lo <= (z, y, x) < hi alone"""
        lo, hi = np.array(lo, np.int64), np.array(hi, np.int64)
        shape = tuple(int(b - a) for a, b in zip(lo, hi))
        out = {}
        if J:
            out["J"] = np.empty(shape, np.float32)
        if J8:
            out["J8"] = np.empty(shape, np.uint8)
        if V:
            for k in ("Vx", "Vy", "Vz"):
                out[k] = np.empty(shape, np.uint8)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        check(self.L.pnr_get_frangi_box(self.h, lo.ctypes.data, hi.ctypes.data, ptr("J"), ptr("J8"), ptr("Vx"), ptr("Vy"), ptr("Vz")))
        return out

    def gaussian(self, sig):
        F = np.empty(self.shape, np.float32)
        check(self.L.pnr_gaussian(self.h, sig, F.ctypes.data))
        return F

    def hessian(self, sig):
        H = [np.empty(self.shape, np.float32) for _ in range(6)]
        check(self.L.pnr_hessian(self.h, sig, *[a.ctypes.data for a in H]))
        return dict(zip(("Dzz", "Dyy", "Dyz", "Dxx", "Dxy", "Dxz"), H))

    def set_j8_v(self, J8, Vx, Vy, Vz):
        arrs = [np.ascontiguousarray(a, np.uint8) for a in (J8, Vx, Vy, Vz)]
        check(self.L.pnr_set_j8_v(self.h, *[a.ctypes.data for a in arrs]))

    # ---- seeds ----
    def extract_seeds(self, z0=None, z1=None):
        ptr, n = C.c_void_p(), C.c_int64()
        if z0 is None:
            check(self.L.pnr_extract_seeds(self.h, C.byref(ptr), C.byref(n)))
        else:
            check(self.L.pnr_extract_seeds_range(self.h, z0, z1, C.byref(ptr), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, SEED_DT)
        buf = (C.c_char * (n.value * SEED_DT.itemsize)).from_address(ptr.value)
        return np.frombuffer(buf, SEED_DT).copy()

    def seed_handover(self, z0=None, z1=None):
        """test tap pnr_seed_handover: what the GPU half of extract_seeds(z0, z1) hands to the host's flood fill -- per layer vmin,
        vmax, ltot (pixels above the minimum), the candidate keys sorted inside each layer with key_off [nl + 1], the layers as the
        fill's loader rebuilds them (nl, h, w) and restored (1: the loader's image is uniform again after its restore)"""
        l, h, w = self.shape
        z0, z1 = (0, l) if z0 is None else (int(z0), int(z1))
        nl = max(z1 - z0, 0)
        out = dict(vmin=np.zeros(nl, np.int32), vmax=np.zeros(nl, np.int32), ltot=np.zeros(nl, np.int64), key_off=np.zeros(nl + 1, np.int64),
                   layers=np.zeros((nl, h, w), np.uint8), restored=np.zeros(nl, np.int32))
        keys, n = np.zeros(0, np.int64), C.c_int64()
        while True:
            check(self.L.pnr_seed_handover(self.h, z0, z1, out["vmin"].ctypes.data, out["vmax"].ctypes.data, out["ltot"].ctypes.data,
                                           out["key_off"].ctypes.data, keys.ctypes.data, len(keys), C.byref(n), out["layers"].ctypes.data,
                                           out["restored"].ctypes.data))
            if n.value <= len(keys):
                break
            keys = np.zeros(n.value, np.int64)
        out["keys"] = keys[:n.value]
        return out

    def phased_likelihood(self, poses, centroids, modes):
        """test tap pnr_phased_likelihood: the likelihood half of one phased SMC step over the given traces -- poses (nt, np, 6),
        centroids (nt, 6), modes (nt,) in PHL_FIRST / PHL_REGULAR / PHL_TAIL.  Returns corr (nt, S, np_pad) per scale and chain, uidx
        and cmap (nt, np_pad), flags (nt, 16) (PHL_OX .. PHL_NCH) and info: the launch forms the step took"""
        n_p, S = int(self.p.np), int(self.p.nsig)
        poses = np.ascontiguousarray(poses, np.float32)
        cen = np.ascontiguousarray(centroids, np.float32)
        modes = np.ascontiguousarray(modes, np.int32)
        nt = len(modes)
        if poses.shape != (nt, n_p, 6) or cen.shape != (nt, 6):
            raise PnrError(f"poses {poses.shape} / centroids {cen.shape} for {nt} traces of {n_p} particles")
        np_pad = (n_p + 1 + 63) // 64 * 64
        out = dict(corr=np.zeros((nt, S, np_pad), np.float32), uidx=np.zeros((nt, np_pad), np.int32), cmap=np.zeros((nt, np_pad), np.int32),
                   flags=np.zeros((nt, 16), np.int32))
        info = np.zeros(8, np.int32)
        check(self.L.pnr_phased_likelihood(self.h, nt, poses.ctypes.data, cen.ctypes.data, modes.ctypes.data, out["corr"].ctypes.data,
                                           out["uidx"].ctypes.data, out["cmap"].ctypes.data, out["flags"].ctypes.data, info.ctypes.data))
        out["info"] = dict(zip(("np_pad", "S", "nsplit", "share", "deep", "cube_copy", "ng", "rounds"), (int(v) for v in info)))
        return out

    def phased_decide(self, flags, seeds, part, prior, idxres, xcs, corr, cmap, draws=None, den=None, lp=0, predict_only=False):
        """test tap pnr_phased_decide: ph_update, then the following step's ph_predict, over the given traces in the device's layout --
        flags (nt, 16), seeds (nt, 6), part (nt, 2, np, 9), prior (nt, np), idxres (nt, np), xcs (nt, 2, 8), corr (nt, S, np_pad), cmap
        (nt, np_pad), draws (np + 1,) or None, den (l, h, w) or None.  Returns the state after ph_update (part_u, neff, xcs_u, oxc, oT,
        ostop, idxres_u, prior_u, flags_u, cnt_next, list_next) and after ph_predict (part_p, prior_p, flags_p, uidx, cmap_p, cnt_p);
        predict_only: ph_predict alone, at the traces' own iterations (iteration 0's draw)"""
        n_p, S, ni = int(self.p.np), int(self.p.nsig), int(self.p.ni)
        np_pad = (n_p + 1 + 63) // 64 * 64
        flags = np.ascontiguousarray(flags, np.int32)
        nt = len(flags)
        a = dict(flags=flags, seeds=np.ascontiguousarray(seeds, np.float32), part=np.ascontiguousarray(part, np.float32),
                 prior=np.ascontiguousarray(prior, np.float32), idxres=np.ascontiguousarray(idxres, np.int32), xcs=np.ascontiguousarray(xcs, np.float32),
                 corr=np.ascontiguousarray(corr, np.float32), cmap=np.ascontiguousarray(cmap, np.int32))
        shapes = dict(flags=(nt, 16), seeds=(nt, 6), part=(nt, 2, n_p, 9), prior=(nt, n_p), idxres=(nt, n_p), xcs=(nt, 2, 8), corr=(nt, S, np_pad),
                      cmap=(nt, np_pad))
        for k, shp in shapes.items():
            if a[k].shape != shp:
                raise PnrError(f"{k} {a[k].shape} for {nt} traces of {n_p} particles: {shp}")
        if draws is not None:
            a["draws"] = np.ascontiguousarray(draws, np.uint32)
            if a["draws"].shape != (n_p + 1,):
                raise PnrError(f"draws {a['draws'].shape}")
        if den is not None:
            a["den"] = np.ascontiguousarray(den, np.uint8)
            if a["den"].shape != tuple(self.shape):
                raise PnrError(f"den {a['den'].shape} for a volume {self.shape}")
        i32, f32 = np.int32, np.float32
        out = dict(part_u=np.zeros(shapes["part"], f32), neff=np.zeros((nt, ni), f32), xcs_u=np.zeros(shapes["xcs"], f32), oxc=np.zeros((nt, ni, 8), f32),
                   oT=np.zeros(nt, i32), ostop=np.zeros(nt, i32), idxres_u=np.zeros(shapes["idxres"], i32), prior_u=np.zeros(shapes["prior"], f32),
                   flags_u=np.zeros(shapes["flags"], i32), cnt_next=np.zeros(1, i32), list_next=np.zeros(nt, i32),
                   part_p=np.zeros(shapes["part"], f32), prior_p=np.zeros(shapes["prior"], f32), flags_p=np.zeros(shapes["flags"], i32),
                   uidx=np.zeros((nt, np_pad), i32), cmap_p=np.zeros((nt, np_pad), i32), cnt_p=np.zeros(2, i32))
        pin, pout = PhdIn(), PhdOut()
        for k in PHD_IN:
            setattr(pin, k, a[k].ctypes.data if k in a else None)
        pin.lp, pin.mode = int(lp), int(bool(predict_only))
        for k in PHD_OUT:
            setattr(pout, k, out[k].ctypes.data)
        check(self.L.pnr_phased_decide(self.h, nt, C.byref(pin), C.byref(pout)))
        return out

    def zncc(self, pos_dir):
        pd = np.ascontiguousarray(pos_dir, np.float32).reshape(-1, 6)
        corr = np.empty(len(pd), np.float32)
        sig = np.empty(len(pd), np.float32)
        check(self.L.pnr_zncc_batch(self.h, pd.ctypes.data, len(pd), corr.ctypes.data, sig.ctypes.data))
        return corr, sig

    def score_filter_sort(self, seeds, fn="pnr_score_filter_sort_seeds"):
        s = np.ascontiguousarray(seeds, SEED_DT).copy()
        n = C.c_int64()
        check(getattr(self.L, fn)(self.h, s.ctypes.data, len(s), C.byref(n)))
        return s[:n.value].copy()

    def score_filter(self, seeds):
        """score + threshold, order kept (a rank's own z-slab of seeds)"""
        return self.score_filter_sort(seeds, "pnr_score_filter_seeds")

    def sort_seeds(self, seeds):
        """stable sort by corr of already scored seeds (the merged list of all ranks)"""
        return self.score_filter_sort(seeds, "pnr_sort_seeds")

    # ---- tracing ----
    def trace_batch(self, seeds, dbg_iters=0):
        s = np.ascontiguousarray(seeds, SEED_DT)
        n, ni, npc = len(s), self.p.ni, self.p.np
        T = np.zeros(2 * n, np.int32)
        stop = np.zeros(2 * n, np.int32)
        xc = np.zeros((2 * n, ni), XEST_DT)
        dbg = {}
        xf = idx = neff = None
        if dbg_iters > 0:
            dbg_iters = min(dbg_iters, ni)
            xf = np.zeros((2 * n, dbg_iters, npc, 9), np.float32)
            idx = np.zeros((2 * n, dbg_iters, npc), np.int32)
            neff = np.zeros((2 * n, dbg_iters), np.float32)
            dbg = dict(xfilt=xf, idxres=idx, neff=neff)
        p = lambda a: a.ctypes.data if a is not None else None
        check(self.L.pnr_trace_batch(self.h, s.ctypes.data, n, T.ctypes.data, stop.ctypes.data, xc.ctypes.data, dbg_iters,
                                     p(xf), p(idx), p(neff)))
        return T, stop, xc, dbg

    def replay(self, seeds, T, xc):
        """host replay of the trace bookkeeping with this context's parameters, dimensions and soma (pnr_replay_traces_ctx)"""
        s = np.ascontiguousarray(seeds, SEED_DT)
        T = np.ascontiguousarray(T, np.int32)
        xc = np.ascontiguousarray(xc, XEST_DT)
        cap = int(T.sum()) + 2 + 4096
        while True:
            nodes = np.zeros(cap, NODE_DT)
            links = np.zeros((2 * cap + 2, 2), np.int32)
            nn, nl, nt = C.c_int64(), C.c_int64(), C.c_int64()
            check(self.L.pnr_replay_traces_ctx(self.h, s.ctypes.data, len(s), T.ctypes.data, xc.ctypes.data, nodes.ctypes.data, cap,
                                               C.byref(nn), links.ctypes.data, len(links), C.byref(nl), C.byref(nt)))
            if nn.value <= cap and nl.value <= len(links):
                return nodes[:nn.value].copy(), links[:nl.value].copy(), nt.value
            cap = int(nn.value) + 2

    # ---- soma path (somaradius > 0) ----
    def soma(self, want_e8=False):
        """pnr_soma: threshold, soma nodes, sparse label map (voxel index, node index) [, the eroded + blurred stack]"""
        l, h, w = self.shape
        E8 = np.zeros((l, h, w), np.uint8) if want_e8 else None
        th, n = C.c_int32(), C.c_int64()
        check(self.L.pnr_soma(self.h, E8.ctypes.data if want_e8 else None, C.byref(th), C.byref(n)))
        nn, nv = C.c_int64(), C.c_int64()
        check(self.L.pnr_get_soma(self.h, None, 0, C.byref(nn), None, None, 0, C.byref(nv)))
        nodes = np.zeros(nn.value, NODE_DT)
        vox = np.zeros(nv.value, np.int64)
        lab = np.zeros(nv.value, np.int32)
        check(self.L.pnr_get_soma(self.h, nodes.ctypes.data, len(nodes), C.byref(nn), vox.ctypes.data, lab.ctypes.data, len(vox), C.byref(nv)))
        out = dict(threshold=th.value, nodes=nodes, vox=vox, lab=lab)
        if want_e8:
            out["E8"] = E8
        return out

    def get_graph(self):
        """node graph of the last trace_replay / trace_replay_sharded (pnr_get_graph)"""
        nn, nl = C.c_int64(), C.c_int64()
        check(self.L.pnr_get_graph(self.h, None, 0, C.byref(nn), None, 0, C.byref(nl)))
        nodes = np.zeros(nn.value, NODE_DT)
        links = np.zeros((nl.value, 2), np.int32)
        check(self.L.pnr_get_graph(self.h, nodes.ctypes.data, len(nodes), C.byref(nn), links.ctypes.data, len(links), C.byref(nl)))
        return nodes, links

    def trace_log(self):
        """[(seed rank, direction, ti_limit, reason, value)] of the last trace_replay with option trace_log = 1 (pnr_get_trace_log)"""
        n = C.c_int64()
        check(self.L.pnr_get_trace_log(self.h, None, 0, C.byref(n)))
        rec = np.zeros((n.value, 5), np.int32)
        check(self.L.pnr_get_trace_log(self.h, rec.ctypes.data, n.value, C.byref(n)))
        return rec

    def trace_replay(self, seeds, first_batch=0):
        """streamed trace + replay (pnr_trace_replay): nodes, links, traces used, SMC iterations run"""
        s = np.ascontiguousarray(seeds, SEED_DT)
        nn, nl, nt, it = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.L.pnr_trace_replay(self.h, s.ctypes.data, len(s), first_batch, None, 0, C.byref(nn), None, 0, C.byref(nl), C.byref(nt), C.byref(it)))
        nodes, links = self.get_graph()
        return nodes, links, nt.value, it.value

    def trace_replay_sharded(self, seeds, rank, world, exchange):
        """this rank's part of tracing ONE sorted seed list on `world` GPUs (pnr_trace_replay_sharded); `exchange` is an ALLGATHER_FN
        (a Python callback, e.g. multigpu.make_exchange) or a ShmExchange (the library's own shared-memory all-gather: no Python in
        the loop).  Every rank returns the same graph; the iteration count is this rank's."""
        s = np.ascontiguousarray(seeds, SEED_DT)
        nn, nl, nt, it = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        fn, user = (exchange.fn, exchange.handle) if hasattr(exchange, "handle") else (exchange, None)  # ShmExchange / RcclExchange: no Python in the loop
        check(self.L.pnr_trace_replay_sharded(self.h, s.ctypes.data, len(s), rank, world, fn, user, None, 0, C.byref(nn), None, 0,
                                              C.byref(nl), C.byref(nt), C.byref(it)))
        nodes, links = self.get_graph()
        return nodes, links, nt.value, it.value

    def have_soma(self):
        nn, nv = C.c_int64(), C.c_int64()
        return self.L.pnr_get_soma(self.h, None, 0, C.byref(nn), None, None, 0, C.byref(nv)) == 0

    def set_option(self, key, value):
        check(self.L.pnr_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64()
        check(self.L.pnr_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    def set_options(self, spec):
        """'window=512,groups=2' (bench.py / tests: PNR_BENCH_OPTS); returns what was set"""
        out = {}
        for kv in filter(None, (spec or "").split(",")):
            k, v = kv.split("=")
            self.set_option(k.strip(), int(v))
            out[k.strip()] = int(v)
        return out

    def table(self, name):
        n = C.c_int64()
        check(self.L.pnr_get_table(self.h, name.encode(), None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint32 if name == "rng" else np.int32 if name == "scale_share" else np.float32)
        check(self.L.pnr_get_table(self.h, name.encode(), out.ctypes.data, n.value, C.byref(n)))
        return out

    def set_smc_driver(self, driver):
        """'phased' (0, default) or 'persistent' (1): how the particle filter is scheduled; results are identical."""
        d = {"phased": 0, "persistent": 1}.get(driver, driver)
        check(self.L.pnr_set_smc_driver(self.h, int(d)))

    # ---- profiling ----
    def set_profiling(self, on=True):
        check(self.L.pnr_set_profiling(self.h, int(on)))

    # ---- reconstruct() with its neighbour stages on this GPU ----
    def reconstruct(self, nodes, links, trace_rsmpl=0.0, sig2radius=0.0, refine_iter=0, epsilon2=0.0, group_radius=0.0, tree_size_min=0):
        """pnr_reconstruct_ctx: the output of lib.reconstruct, byte for byte -> tree nodes (index 0 dummy), parents (-1 = root)"""
        return _reconstruct(self.L.pnr_reconstruct_ctx, (self.h,), nodes, links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, tree_size_min)

    def reconstruct_stage(self, nodes, links, stage, trace_rsmpl=0.0, sig2radius=0.0, refine_iter=0, epsilon2=0.0, group_radius=0.0):
        """test tap pnr_reconstruct_stage_ctx: lib.reconstruct_stage with the device stages -> nodes, link pairs"""
        return _reconstruct_stage(self.L.pnr_reconstruct_stage_ctx, (self.h,), nodes, links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, stage)

    def kernel_ms(self, group):
        ms, n = C.c_double(), C.c_int64()
        check(self.L.pnr_get_kernel_ms(self.h, group.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def reset_kernel_ms(self):
        check(self.L.pnr_reset_kernel_ms(self.h))

    def eigen(self, A, vectors=True):
        """test tap: the device's JAMA solver on n symmetric 3 x 3 matrices -> (V or None, d)"""
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 3, 3)
        d = np.empty((len(A), 3), np.float64)
        V = np.empty((len(A), 3, 3), np.float64) if vectors else None
        check(self.L.pnr_eigen_batch(self.h, A.ctypes.data, len(A), V.ctypes.data if vectors else None, d.ctypes.data))
        return V, d

    def expf(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        check(self.L.pnr_expf_batch(self.h, x.ctypes.data, x.size, y.ctypes.data))
        return y


def replay(params, shape, seeds, T, xc):
    """Host replay of trackPos/trackNeg bookkeeping (pure host; no GPU needed)."""
    L = load()
    l, h, w = shape
    s = np.ascontiguousarray(seeds, SEED_DT)
    T = np.ascontiguousarray(T, np.int32)
    xc = np.ascontiguousarray(xc, XEST_DT)
    cap = int(T.sum()) + 2
    nodes = np.zeros(cap, NODE_DT)
    links = np.zeros((2 * cap + 2, 2), np.int32)
    nn, nl, nt = C.c_int64(), C.c_int64(), C.c_int64()
    check(L.pnr_replay_traces(C.byref(params), w, h, l, s.ctypes.data, len(s), T.ctypes.data, xc.ctypes.data,
                              nodes.ctypes.data, cap, C.byref(nn), links.ctypes.data, len(links), C.byref(nl), C.byref(nt)))
    return nodes[:nn.value].copy(), links[:nl.value].copy(), nt.value


class ShmExchange:
    """pnr_shm_exchange: an all-gather between the ranks of ONE host through POSIX shared memory (include/pnr_hip.h).  `fn` / `handle`
    are what pnr_trace_replay_sharded takes as exchange / user; allgather() is the same call for other small host-side collectives."""

    def __init__(self, name, rank, world, capacity=1 << 20):
        self.L = load()
        h = C.c_void_p()
        check(self.L.pnr_shm_exchange_open(name.encode(), rank, world, capacity, C.byref(h)))
        self.handle, self.rank, self.world, self.capacity = h, rank, world, capacity
        self.fn = C.cast(self.L.pnr_shm_allgather, ALLGATHER_FN)

    def allgather(self, block):
        """bytes of equal length on every rank -> list of `world` bytes objects"""
        n = len(block)
        send = (C.c_char * max(n, 1)).from_buffer_copy(block.ljust(1, b"\0"))
        recv = (C.c_char * max(n * self.world, 1))()
        rc = self.L.pnr_shm_allgather(self.handle, send, recv, n)
        if rc != 0:
            raise PnrError(f"shared-memory all-gather failed ({rc})")
        raw = bytes(recv)
        return [raw[r * n:(r + 1) * n] for r in range(self.world)]

    def close(self):
        if self.handle:
            self.L.pnr_shm_exchange_close(self.handle)
            self.handle = None


class RcclExchange:
    """pnr_rccl_exchange: the same collectives over RCCL from a host that is not torch (include/pnr_hip.h): ncclAllGather of one block
    per rank (`fn` / `handle` = exchange / user of pnr_trace_replay_sharded) and the (min, max) all-reduce.  `uid` = the 128 bytes
    of RcclExchange.unique_id() of one rank, handed to the others by the launcher.  A collective call: one rank per GPU."""

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        check(load().pnr_rccl_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid, rank, world, device, capacity=1 << 20):
        self.L = load()
        h = C.c_void_p()
        check(self.L.pnr_rccl_exchange_open(uid, rank, world, device, capacity, C.byref(h)))
        self.handle, self.rank, self.world, self.capacity = h, rank, world, capacity
        self.fn = C.cast(self.L.pnr_rccl_allgather, ALLGATHER_FN)

    def allgather(self, block):
        n = len(block)
        send = (C.c_char * max(n, 1)).from_buffer_copy(block.ljust(1, b"\0"))
        recv = (C.c_char * max(n * self.world, 1))()
        check(self.L.pnr_rccl_allgather(self.handle, send, recv, n))
        raw = bytes(recv)
        return [raw[r * n:(r + 1) * n] for r in range(self.world)]

    def minmax(self, mn, mx):
        a, b = C.c_float(mn), C.c_float(mx)
        check(self.L.pnr_rccl_allreduce_minmax(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.handle:
            self.L.pnr_rccl_exchange_close(self.handle)
            self.handle = None


def sched_playback(params, shape, seeds, trace_fn, rank=0, world=1, exchange=None, block_bytes=0, window=768, groups=1, poll=4, look0=0, look_pct=-1, tentative=True, target=-1, lag=-1):
    """The streaming scheduler over a host engine that plays back map-free traces (pnr_sched_playback; no GPU): `trace_fn(pos_dir6)`
    -> (T, xc[ni][8]).  Returns nodes, links, traces used, iterations on this rank."""
    L = load()
    l, h, w = shape
    s = np.ascontiguousarray(seeds, SEED_DT)
    ni = params.ni

    def _tr(user, pd, T, xc):
        try:
            Tn, rows = trace_fn(np.ctypeslib.as_array(pd, (6,)).copy())
            T[0] = int(Tn)
            out = np.ctypeslib.as_array(C.cast(xc, C.POINTER(C.c_float)), (ni, 8))
            k = min(int(Tn), ni)
            out[:k] = np.asarray(rows, np.float32).reshape(-1, 8)[:k]
            return 0
        except Exception:  # noqa: BLE001 -- must not propagate through the C frames
            import traceback
            traceback.print_exc()
            return 1

    tcb = TRACE_FN(_tr)
    xuser = None
    if isinstance(exchange, (ShmExchange, RcclExchange)):
        exchange, xuser = exchange.fn, exchange.handle
    xcb = exchange if exchange is not None else C.cast(None, ALLGATHER_FN)
    nn, nl, nt, it = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    cap = 2 * len(s) * ni + 2
    nodes = np.zeros(cap, NODE_DT)
    links = np.zeros((2 * cap + 2, 2), np.int32)
    check(L.pnr_sched_playback2(C.byref(params), w, h, l, s.ctypes.data, len(s), rank, world, xcb, xuser, block_bytes, tcb, None, window, groups, poll, look0, look_pct,
                                int(bool(tentative)), int(target), int(lag), nodes.ctypes.data, cap, C.byref(nn), links.ctypes.data, len(links), C.byref(nl), C.byref(nt), C.byref(it)))
    return nodes[:nn.value].copy(), links[:nl.value].copy(), nt.value, it.value


def reconstruct(nodes, links, trace_rsmpl=0.0, sig2radius=0.0, refine_iter=0, epsilon2=0.0, group_radius=0.0, tree_size_min=0):
    """reconstruct() chain on the host (pnr_reconstruct): tree nodes (index 0 dummy) and parent indices (-1 = root)."""
    return _reconstruct(load().pnr_reconstruct, (), nodes, links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, tree_size_min)


def _reconstruct(fn, head, nodes, links, *consts):
    """pnr_reconstruct[_ctx] (head: nothing, or the context): grow the outputs until the tree fits"""
    nodes = np.ascontiguousarray(nodes, NODE_DT)
    links = np.ascontiguousarray(links, np.int32).reshape(-1, 2)
    cap = max(16, 4 * len(nodes))
    while True:
        out = np.zeros(cap, NODE_DT)
        par = np.zeros(cap, np.int32)
        n = C.c_int64()
        check(fn(*head, nodes.ctypes.data, len(nodes), links.ctypes.data, len(links), *consts, out.ctypes.data, par.ctypes.data, cap, C.byref(n)))
        if n.value <= cap:
            return out[:n.value].copy(), par[:n.value].copy()
        cap = int(n.value)


def _reconstruct_stage(fn, head, nodes, links, *consts):
    """pnr_reconstruct_stage[_ctx]: count first, then fetch"""
    nodes = np.ascontiguousarray(nodes, NODE_DT)
    links = np.ascontiguousarray(links, np.int32).reshape(-1, 2)
    args = (*head, nodes.ctypes.data, len(nodes), links.ctypes.data, len(links), *consts)
    nn, nl = C.c_int64(), C.c_int64()
    check(fn(*args, None, 0, C.byref(nn), None, 0, C.byref(nl)))
    out = np.zeros(nn.value, NODE_DT)
    lk = np.zeros((nl.value, 2), np.int32)
    check(fn(*args, out.ctypes.data, len(out), C.byref(nn), lk.ctypes.data, len(lk), C.byref(nl)))
    return out, lk


def tree_sample(xyz, parent, zscale=1, step=1, count_only=False):
    """pnr_tree_sample (pure host; no GPU needed): the sample points of a tree by the rule of the tree distance -> (pts float32[k, 3],
    owner int32[k]), or only k"""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    if len(parent) != len(xyz):
        raise PnrError("tree_sample: one parent per node")
    n = C.c_int64()
    check(L.pnr_tree_sample(xyz.ctypes.data, parent.ctypes.data, len(xyz), float(zscale), float(step), None, None, 0, C.byref(n)))
    if count_only:
        return n.value
    pts = np.empty((n.value, 3), np.float32)
    owner = np.empty(n.value, np.int32)
    check(L.pnr_tree_sample(xyz.ctypes.data, parent.ctypes.data, len(xyz), float(zscale), float(step), pts.ctypes.data, owner.ctypes.data, n.value, C.byref(n)))
    return pts, owner


def join_reroot(parent, bridges=(), root=-1):
    """pnr_join_reroot (pure host; no GPU needed): the re-rooting and ordering half of the join -> (parent int32[n], order int32[n],
    comp int32[n]); bridges: a BRIDGE array, or (lo, hi) pairs"""
    L = load()
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    if not (isinstance(bridges, np.ndarray) and bridges.dtype == BRIDGE):
        pairs = np.asarray(bridges, np.int64).reshape(-1, 2)
        bridges = np.zeros(len(pairs), BRIDGE)
        bridges["lo"], bridges["hi"] = pairs[:, 0], pairs[:, 1]
    bridges = np.ascontiguousarray(bridges)
    out = [np.empty(len(parent), np.int32) for _ in range(3)]
    check(L.pnr_join_reroot(parent.ctypes.data, len(parent), bridges.ctypes.data if len(bridges) else None, len(bridges), int(root),
                            out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
    return tuple(out)


def skeleton_forest(vox, shape):
    """pnr_skeleton_forest (pure host; no GPU needed): the k voxels vox (linear indices of a stack of shape (l, h, w)) as a forest -- the
    unique minimum spanning forest of their 26-adjacent pairs under (squared step length, lo, hi) -> BRIDGE[k - components] sorted by
    (lo, hi), d = the step length; join_reroot(np.full(k, -1), edges) gives parents and tree order"""
    L = load()
    vox = np.ascontiguousarray(vox, np.int64).reshape(-1)
    l, h, w = (int(v) for v in shape)
    edges = np.zeros(max(len(vox) - 1, 0), BRIDGE)
    n = C.c_int64()
    check(L.pnr_skeleton_forest(vox.ctypes.data if len(vox) else None, len(vox), w, h, l, edges.ctypes.data if len(edges) else None, len(edges), C.byref(n)))
    return edges[:n.value]


def join_expand(xyz, parent, bridges, paths):
    """pnr_join_expand (pure host; no GPU needed): the interior voxels of the bridges' chains as new nodes n, n + 1, ... behind the n nodes
    of the forest; bridges, paths: what Context.join_trees_geodesic returned -> (xyz float32[n2, 3], parent int32[n2], bridge_of
    int32[n2 - n] the bridge of every new node, join BRIDGE[k] for join_reroot(parent, join))"""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    if len(parent) != len(xyz):
        raise PnrError("join_expand: one parent per node")
    bridges = np.ascontiguousarray(bridges, GEO_BRIDGE)
    vox = np.ascontiguousarray(paths["vox"], np.int64).reshape(-1)
    l, h, w = (int(v) for v in paths["shape"])
    n, nb = len(xyz), len(bridges)
    join = np.zeros(nb, BRIDGE)
    n2 = C.c_int64()
    args = (xyz.ctypes.data, parent.ctypes.data, n, bridges.ctypes.data if nb else None, nb, vox.ctypes.data if len(vox) else None, len(vox), w, h, l)
    check(L.pnr_join_expand(*args, None, None, None, 0, C.byref(n2), None))
    xyz2, parent2, of = np.empty((n2.value, 3), np.float32), np.empty(n2.value, np.int32), np.empty(n2.value - n, np.int32)
    check(L.pnr_join_expand(*args, xyz2.ctypes.data, parent2.ctypes.data, of.ctypes.data if len(of) else None, n2.value, C.byref(n2), join.ctypes.data if nb else None))
    return xyz2, parent2, of, join


def _prune_call(fn, who, xyz, radius, parent, zscale, min_length, radius_factor, min_tree):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    if radius is not None:
        radius = np.ascontiguousarray(radius, np.float32).reshape(-1)
    if len(parent) != len(xyz) or (radius is not None and len(radius) != len(xyz)):
        raise PnrError(f"{who}: one radius and one parent per node")
    n = len(xyz)
    o, info = PruneOpts(float(zscale), float(min_length), float(radius_factor), float(min_tree)), PruneInfo()
    out = [np.zeros(n, t) for t in (np.uint8, np.uint32, np.uint32, np.int32, np.int32)]
    check(fn(xyz.ctypes.data if n else None, radius.ctypes.data if radius is not None and n else None, parent.ctypes.data if n else None, n, C.byref(o), C.byref(info),
             *(a.ctypes.data if n else None for a in out)))
    return (info.as_dict(), *out)


def prune_tree_host(xyz, radius, parent, zscale=1, min_length=0, radius_factor=0, min_tree=0):
    """pnr_prune_tree_host (pure host; no GPU needed): Context.prune_tree as one sequential pass, the same outputs (rounds_up =
    rounds_down = 0)"""
    return _prune_call(load().pnr_prune_tree_host, "prune_tree_host", xyz, radius, parent, zscale, min_length, radius_factor, min_tree)


def prune_apply(parent, keep):
    """pnr_prune_apply (pure host; no GPU needed): the kept nodes in input order -> (new_index int32[n] (-1: removed), parent int32[m]
    remapped); a keep that holds a child of a removed node is refused"""
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
    if len(parent) != len(keep):
        raise PnrError("prune_apply: one keep per node")
    n, m = len(parent), C.c_int64()
    idx, par = np.empty(n, np.int32), np.empty(n, np.int32)
    check(load().pnr_prune_apply(parent.ctypes.data if n else None, keep.ctypes.data if n else None, n, idx.ctypes.data if n else None, par.ctypes.data if n else None, C.byref(m)))
    return idx, par[:m.value].copy()


def _tree_arrays(who, xyz, radius, parent):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    radius = np.ascontiguousarray(radius, np.float32).reshape(-1)
    parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
    if len(parent) != len(xyz) or len(radius) != len(xyz):
        raise PnrError(f"{who}: one radius and one parent per node")
    return xyz, radius, parent


def render_items(xyz, radius, parent, shape, zscale=1, rscale=1, radd=0, piece=0, box=0):
    """test tap pnr_render_items (pure host; no GPU needed): the work items of render_tree on the grid shape = (l, h, w) with the options
    render_piece = piece and render_box = box -> int64[items, 7] of (segment, x0, y0, z0, x1, y1, z1), the box inclusive"""
    L = load()
    xyz, radius, parent = _tree_arrays("render_items", xyz, radius, parent)
    l, h, w = (int(v) for v in shape)
    o = RenderOpts(float(zscale), float(rscale), float(radd), -1)
    k = C.c_int64()
    args = (xyz.ctypes.data, radius.ctypes.data, parent.ctypes.data, len(xyz), w, h, l, C.byref(o), int(piece), int(box))
    check(L.pnr_render_items(*args, None, 0, C.byref(k)))
    items = np.zeros((k.value, 7), np.int64)
    check(L.pnr_render_items(*args, items.ctypes.data, k.value, C.byref(k)))
    return items


def write_tiff(path, img):
    """test tap pnr_test_write_tiff (pure host): the host's volume writer on a uint8 (l, h, w) stack -- a multi-page TIFF, or bare bytes
    for a .raw name"""
    img = np.ascontiguousarray(img, np.uint8)
    l, h, w = img.shape
    check(load().pnr_test_write_tiff(os.fsencode(path), img.ctypes.data, w, h, l))


def read_swc_nodes(path):
    """an SWC file with all its columns, read by the rules of read_swc -> (xyz float32[n, 3], radius float32[n], type int32[n], parent
    int32[n] (index among the nodes, -1: none), ids int64[n])"""
    xyz, parent, ids = read_swc(path)
    radius, typ = [], []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            typ.append(int(float(t[1])))
            radius.append(float(t[5]))
    return xyz, np.array(radius, np.float64).astype(np.float32).reshape(-1), np.array(typ, np.int32).reshape(-1), parent, ids


def read_swc(path):
    """an SWC file as advantra_cli --distance reads it -> (xyz float32[n, 3], parent int32[n] (index of the parent's line among the
    nodes, -1: none or not in the file), ids int64[n]).  Lines `n type x y z r parent`; `#` comments and blank lines are skipped; ids
    may be written as 3.0 and come in any order; a duplicate id or a short line is an error that names the file and the line."""
    ids, xyz, par, index = [], [], [], {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            try:
                if len(t) < 7:
                    raise ValueError
                v = [float(x) for x in t[:7]]
                if not all(np.isfinite(v)) or v[0] != int(v[0]) or v[6] != int(v[6]):
                    raise ValueError
            except (ValueError, OverflowError):
                raise PnrError(f"{path}:{ln}: not an SWC line `n type x y z r parent`") from None
            if int(v[0]) in index:
                raise PnrError(f"{path}:{ln}: duplicate node id {int(v[0])}")
            index[int(v[0])] = len(ids)
            ids.append(int(v[0]))
            xyz.append(v[2:5])
            par.append(int(v[6]))
    parent = np.array([index.get(p, -1) if p >= 0 else -1 for p in par], np.int32).reshape(-1)
    return np.array(xyz, np.float64).reshape(-1, 3).astype(np.float32), parent, np.array(ids, np.int64).reshape(-1)


def live_bytes():
    """test tap pnr_live_bytes: (device bytes, pinned host bytes) the library holds now, over every context and exchange of the process"""
    dev, pin = C.c_int64(), C.c_int64()
    check(load().pnr_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def radius_offsets(zdist, rmax, is2d=False):
    """test tap pnr_radius_offsets (pure host; no GPU needed): the shells of measure_radii's rule -> (starts int32[rmax + 2],
    offsets int32[n, 3] as (dx, dy, dz)); shell k = offsets[starts[k]:starts[k + 1]]"""
    L = load()
    n = C.c_int64()
    starts = np.zeros(int(rmax) + 2 if 1 <= int(rmax) <= PNR_RADIUS_MAX else 2, np.int32)
    check(L.pnr_radius_offsets(float(zdist), int(rmax), int(bool(is2d)), starts.ctypes.data, None, None, None, 0, C.byref(n)))
    d = np.zeros((3, n.value), np.int32)
    check(L.pnr_radius_offsets(float(zdist), int(rmax), int(bool(is2d)), starts.ctypes.data, d[0].ctypes.data, d[1].ctypes.data, d[2].ctypes.data,
                               n.value, C.byref(n)))
    return starts, np.ascontiguousarray(d.T)


def pair_tiles(n, m, split=0, budget=0):
    """test tap pnr_pair_tiles (pure host; no GPU needed): the launches of the pair minimum over n points x m segments or targets with the
    options *_split = split and *_pairs_per_launch = budget -> int64[launches, 7] of (p0, p1, s0, s1, split, grid x, grid y)"""
    L = load()
    k = C.c_int64()
    check(L.pnr_pair_tiles(int(n), int(m), int(split), int(budget), None, 0, C.byref(k)))
    tiles = np.zeros((k.value, 7), np.int64)
    check(L.pnr_pair_tiles(int(n), int(m), int(split), int(budget), tiles.ctypes.data, k.value, C.byref(k)))
    return tiles


def reconstruct_stage(nodes, links, stage, trace_rsmpl=0.0, sig2radius=0.0, refine_iter=0, epsilon2=0.0, group_radius=0.0):
    """the node list behind a stage of reconstruct() (pnr_reconstruct_stage: 1 _n0res_, 2 _n1_, 3 _n2_, 4 _n2tree_) -> nodes, link pairs"""
    return _reconstruct_stage(load().pnr_reconstruct_stage, (), nodes, links, trace_rsmpl, sig2radius, refine_iter, epsilon2, group_radius, stage)


def kernel_source_hash(names=("smc_phased.hip", "smc_device.h", "smc.hip", "ctx.h", "stream_sched.h")):
    """sha256 (first 16 hex digits) over the sources the bytes of a trace-iteration depend on: the SMC kernels, and the defaults
    (ctx.h: max_split, sums_deep_max ...) and the scheduler (stream_sched.h) that decide which kernel form and split a launch
    takes.  The committed PMC traffic profiles carry it, and bench.py only quotes a profile whose hash equals the hash of the sources
    it runs (a changed kernel or default is never priced with the bytes of an older one)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for n in names:
        with open(os.path.join(d, n), "rb") as f:
            h.update(n.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]
