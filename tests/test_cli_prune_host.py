"""CPU: advantra_cli's pruning flags without a GPU -- the usage errors of --prune, --prune-swc and its companions, each with exit status 1
and exactly one line on stderr; --help names the flags; and the order in which --prune-swc fails: the SWC reader first, then pnr_create
(the expectations of test_cli_tool_order.py)."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
NO_GPU = "no HIP device: libpnr_hip has no CPU path (MI355X / gfx950 required)"
PRUNE = "--prune L[,K[,M]]: numbers, 0 or more: the shortest side branch kept, times its parent's radius, the lowest tree kept (xy voxels)"
NEEDS = "--prune-length / --prune-radius / --prune-min-tree need --prune-swc IN.swc [OUT.swc]"
WHERE = "--prune L[,K[,M]] needs a tracing run or --skeleton --swc OUT.swc"
NOT_WITH = "--prune-swc: not with a tracing run (-p), another tool mode, --threshold, --despeckle, --measure-radius or --join"


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def check(r, status, line):
    assert (r.returncode, r.stderr) == (status, line + "\n"), (r.returncode, r.stderr)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CLI)], check=True)
    d = tmp_path_factory.mktemp("prune")
    f = {k: str(d / v) for k, v in (("swc", "t.swc"), ("bad", "bad.swc"), ("empty", "empty.swc"), ("out", "out.swc"), ("csv", "out.csv"))}
    with open(f["swc"], "w") as fh:
        fh.write("# four nodes\n1 2 4 4 2 1 -1\n2 2 10 6 3 1 1\n3 2 16 9 4 1.5 2\n4 2 10 8 3 1 2\n")
    with open(f["bad"], "w") as fh:
        fh.write("# the second line is short\n1 2 3\n")
    with open(f["empty"], "w") as fh:
        fh.write("# no nodes\n")
    return f


@pytest.mark.parametrize("value", ["-1", "x", "1,2,3,4", "", "3,", "3,-0.5", "nan", "1e39", "2,,1"])
def test_bad_values_of_prune(files, value):
    check(run("--prune", value), 1, PRUNE)


def test_prune_without_a_value(files):
    check(run("--prune"), 1, PRUNE)


@pytest.mark.parametrize("flag,line", [("--prune-length", "--prune-length L: the shortest side branch kept, in xy voxels, a number, 0 or more"),
                                       ("--prune-radius", "--prune-radius K: a side branch is kept from K times its parent's radius on, a number, 0 or more"),
                                       ("--prune-min-tree", "--prune-min-tree M: the lowest tree kept, in xy voxels, a number, 0 or more")])
def test_bad_values_of_the_three_thresholds(files, flag, line):
    for value in ("-1", "x", "1,2", "inf"):
        check(run("--prune-swc", files["swc"], files["out"], flag, value), 1, line)
    check(run("--prune-swc", files["swc"], files["out"], flag), 1, line)
    check(run(flag, "3"), 1, NEEDS)
    assert not os.path.exists(files["out"])


def test_flags_that_do_not_go_together(files):
    check(run("--prune-swc"), 1, "--prune-swc IN.swc [OUT.swc]")
    check(run("--prune-swc", "--prune-length", "3"), 1, "--prune-swc IN.swc [OUT.swc]")
    check(run("--prune-swc", files["swc"], files["out"], "--prune", "3"), 1,
          "--prune L[,K[,M]] and --prune-swc: one or the other (--prune-swc takes --prune-length, --prune-radius, --prune-min-tree)")
    check(run("--prune", "3", "--distance", files["swc"], files["swc"]), 1, WHERE)
    check(run("--prune", "3", "--join-swc", files["swc"], files["out"]), 1, WHERE)
    check(run("--prune", "3", "--skeleton", "-i", "none.raw"), 1, WHERE)  # without --swc there is no tree to prune
    check(run("--prune", "3", "--swc-info", files["swc"]), 1, WHERE)
    check(run("--prune-swc", files["swc"], files["out"], "--join", "3"), 1, NOT_WITH)
    check(run("--prune-swc", files["swc"], files["out"], "--distance", files["swc"], files["swc"]), 1, NOT_WITH)
    check(run("--prune-swc", files["swc"], files["out"], "--measure-radius"), 1, NOT_WITH)
    check(run("--prune-swc", files["swc"], "-p", *"2 0 5 0.3 3 2 20 20 2 4 5".split()), 1, NOT_WITH)
    check(run("--prune-swc", files["swc"], "--zscale", "0"), 1, "--zscale: a number, above 0")
    assert not os.path.exists(files["out"])


def test_help_names_the_flags(files):
    r = run("--help")
    assert r.returncode == 0
    for flag in ("--prune L[,K[,M]]", "--prune-swc IN.swc [OUT.swc]", "--prune-length L", "--prune-radius K", "--prune-min-tree M", "#prune=length:L,radius:K,min_tree:M,removed:N,segments:S",
                 "id,keep,height,path,order,seg_id"):
        assert flag in r.stdout, flag


def test_prune_swc_reads_the_file_first_then_creates_the_context(files):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    bad = files["bad"] + ":2: not an SWC line `n type x y z r parent` (3 fields)"
    for extra in ((), ("--prune-length", "3", "--zscale", "2", "--per-node", files["csv"])):
        check(run("--prune-swc", files["bad"], files["out"], *extra), 1, bad)
        check(run("--prune-swc", files["empty"], files["out"], *extra), 1, files["empty"] + ": no nodes")
        check(run("--prune-swc", files["swc"], files["out"], *extra), 1, "pnr_create: " + NO_GPU)
        check(run("--prune-swc", files["swc"], *extra), 1, "pnr_create: " + NO_GPU)  # without OUT: the morphometry alone
    missing = os.path.join(os.path.dirname(files["swc"]), "none.swc")
    check(run("--prune-swc", missing), 1, missing + ": cannot open the file")
    assert not os.path.exists(files["out"]) and not os.path.exists(files["csv"])
