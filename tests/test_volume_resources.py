"""CPU (hipcc cross-compiles gfx950 without a GPU): the one byte-sum kernel behind "thr = -1" of the radii, the coverage and the
components.  From the compiler's own report (-Rpass-analysis=kernel-resource-usage): vol_sum is reported exactly once by volume.hip,
runs without scratch and light enough for eight waves per SIMD -- and no other .hip file of pnr_amd/csrc has a copy of it."""
import glob
import os
import threading
from concurrent.futures import ThreadPoolExecutor
import pytest
from test_kernel_resources import SRC, compile_isa, find

SUM = "vol_sum"


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_isa(tmp_path_factory, "volume.hip")


def test_sum_kernel_is_reported_once_without_scratch(compiled):
    usage, _ = compiled
    u, _ = find(usage, SUM)  # (exactly one)
    assert u["ScratchSize"] == 0 and u["VGPRs"] <= 64 and u["Occupancy"] == 8, u


class _Serial:
    """tmp_path_factory behind a lock: the other files are compiled side by side"""

    def __init__(self, factory):
        self.factory, self.lock = factory, threading.Lock()

    def mktemp(self, name):
        with self.lock:
            return self.factory.mktemp(name)


def test_no_other_file_has_a_sum_kernel(compiled, tmp_path_factory):
    _, name = find(compiled[0], SUM)
    others = sorted(os.path.basename(p) for p in glob.glob(os.path.join(SRC, "*.hip")) if os.path.basename(p) != "volume.hip")
    assert len(others) >= 12, others
    factory = _Serial(tmp_path_factory)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        reports = list(pool.map(lambda src: compile_isa(factory, src), others))
    for src, (usage, asm) in zip(others, reports):
        assert usage, src
        assert not [k for k in usage if SUM in k or "rad_sum" in k or "rn_sum" in k], (src, sorted(usage))
        assert not [ln for ln in asm if name in ln], src
