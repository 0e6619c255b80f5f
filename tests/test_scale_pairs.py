"""CPU: the nesting rule of tables.cpp find_scale_pairs (a guest scale whose template grid is, axis by axis, a contiguous run of
its host's grid is not sampled; its ordered sums come from the host's stash).  tables.cpp is compiled with a small driver."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pnr_amd", "csrc")
DRIVER = r"""
#include "ctx.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    pnr_params P;
    pnr_default_params_host(&P);
    const int is2d = atoi(argv[1]);
    P.nsig = argc - 2;
    for (int s = 0; s < P.nsig; s++) P.sig[s] = (float)atof(argv[2 + s]);
    pnr::Tables t;
    t.nsig = P.nsig;
    pnr::build_tables(P, is2d != 0, t);
    for (const auto &p : t.pairs)
        printf("%d %d %d %d %d %d %d %d\n", p.guest, p.host, p.v0, p.nv, p.u0, p.nu, p.w0, p.nw);
    // the device table: every guest sample's row in its host's stash -- ascending, and at the host's row the same offsets
    for (const auto &p : t.pairs) {
        const int g = p.guest, h = p.host, r0 = t.share_tab[8 + g];
        if (t.share_tab[g] != h) { printf("BAD host\n"); return 1; }
        for (int m = 0; m < t.M[g]; m++) {
            const int r = t.grows[r0 + m];
            if (r < 0 || r >= t.M[h] || (m > 0 && r <= t.grows[r0 + m - 1])) { printf("BAD order\n"); return 1; }
            for (int a = 0; a < 3; a++)
                if (t.tmpl[4 * (t.moff[h] + r) + a] != t.tmpl[4 * (t.moff[g] + m) + a]) { printf("BAD offset\n"); return 1; }
        }
    }
    printf("mask %d\n", t.guest_mask);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pairs_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs")
    src, exe = d / "drv.cpp", d / "drv"
    # pnr_default_params lives in api.cpp with the whole runtime: the driver fills what build_tables reads itself
    src.write_text(DRIVER.replace("pnr_default_params_host(&P);", "std::memset(&P, 0, sizeof(P)); P.np = 50; P.step = 2; P.kappa = 3; P.zdist = 2; P.rng_seed = 1;")
                   .replace("#include <cstdlib>", "#include <cstdlib>\n#include <cstring>"))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "-w", "-I", SRC, str(src),
                        os.path.join(SRC, "tables.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(sigs, is2d=False):
        r = subprocess.run([str(exe), "1" if is2d else "0", *map(str, sigs)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.split("\n")
        pairs = [tuple(map(int, ln.split())) for ln in lines if ln and not ln.startswith("mask")]
        mask = int(next(ln for ln in lines if ln.startswith("mask")).split()[1])
        return pairs, mask
    return run


def test_bench_scales_sigma2_nests_in_sigma4(pairs_bin):
    pairs, mask = pairs_bin([2, 4, 6])
    # guest 0 (sigma 2) in host 1 (sigma 4): v indices 2..6, u and w indices 6..18
    assert pairs == [(0, 1, 2, 5, 6, 13, 6, 13)]
    assert mask == 1


@pytest.mark.parametrize("sigs", [[4, 6], [6, 8], [6, 4]])
def test_no_sub_grid_no_pair(pairs_bin, sigs):
    assert pairs_bin(sigs) == ([], 0)


def test_one_guest_per_host(pairs_bin):
    pairs, mask = pairs_bin([2, 3, 4])
    guests = [p[0] for p in pairs]
    hosts = [p[1] for p in pairs]
    assert len(pairs) >= 1 and len(set(hosts)) == len(hosts)
    assert not set(guests) & set(hosts)  # a guest is not sampled: it cannot be a host
    # the largest guest first: sigma 3 (7 x 19 x 19) in sigma 4, and sigma 2 then has no free sampled host
    assert pairs == [(1, 2, 1, 7, 3, 19, 3, 19)] and mask == 2


def test_two_d_tables(pairs_bin):
    pairs, mask = pairs_bin([2, 4, 6], is2d=True)
    assert pairs == [(0, 1, 2, 5, 6, 13, 0, 1)] and mask == 1  # the w axis is {0} at every scale


def test_equal_scales_pair(pairs_bin):
    pairs, _ = pairs_bin([4, 4])
    assert len(pairs) == 1 and pairs[0][2:] == (0, 9, 0, 25, 0, 25)
