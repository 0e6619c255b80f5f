"""The order in which advantra_cli's tool modes and a tracing run fail, on a machine without a GPU: the stack's loader, the refusal of
--window on an 8-bit stack, the SWC reader and pnr_create report in a fixed order per tool, each with its own exit status and exactly
one line on stderr.  The expected lines are those of the CLI as it was before its host code was split into files."""
import os
import subprocess
import pytest
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pnr_amd", "host", "advantra_cli")
DIMS = "32,24,8"
WINDOW = "--window / --saturate need a 16-bit stack (8-bit input is never windowed)"
NO_GPU = "no HIP device: libpnr_hip has no CPU path (MI355X / gfx950 required)"


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    if not os.path.exists(CLI):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CLI)], check=True)
    d = tmp_path_factory.mktemp("order")
    f = {k: str(d / v) for k, v in (("raw", "s.raw"), ("missing", "none.raw"), ("swc", "t.swc"), ("bad", "bad.swc"), ("empty", "empty.swc"), ("out", "out"))}
    synth.synth(32, 24, 8, seed=1).tofile(f["raw"])
    with open(f["swc"], "w") as fh:
        fh.write("# three nodes\n1 2 4 4 2 1 -1\n2 2 10 6 3 1 1\n3 2 16 9 4 1.5 2\n")
    with open(f["bad"], "w") as fh:
        fh.write("# the second line is short\n1 2 3\n")
    with open(f["empty"], "w") as fh:
        fh.write("# no nodes\n")
    return f


def bad_line(f):
    return f["bad"] + ":2: not an SWC line `n type x y z r parent` (3 fields)"


# per tool: its arguments for a stack and an SWC file, and the file it would write
def tool_args(tool, f, stack, swc):
    out = f["out"]
    return {
        "render": (["--render-swc", swc, "-i", stack, "-d", DIMS, "--mask", out + "_m.raw"], out + "_m.raw"),
        "components": (["--components", "-i", stack, "-d", DIMS, "--labels", out + "_l.raw"], out + "_l.raw"),
        "edt": (["--edt", "-i", stack, "-d", DIMS, "--at", swc, "--per-node", out + "_e.csv", "--edt-out", out + "_e.raw"], out + "_e.raw"),
        "geodesic": (["--geodesic", "-i", stack, "-d", DIMS, "--from", swc, "--geo-out", out + "_g"], out + "_g_d.raw"),
        "trace": (["-d", DIMS, "-f", "advantra_func", "-i", stack, "-p", *"2 0 5 0.3 3 2 20 20 2 4 5".split()], stack + "_Advantra.swc"),
    }[tool]


TOOLS = ("render", "components", "edt", "geodesic", "trace")
WITH_SWC = ("render", "edt", "geodesic")
SWC_FIRST = ("render",)


def check(r, status, line):
    assert (r.returncode, r.stderr) == (status, line + "\n"), (r.returncode, r.stderr)


@pytest.mark.parametrize("tool", TOOLS)
def test_unreadable_stack(files, tool):
    args, out = tool_args(tool, files, files["missing"], files["swc"])
    check(run(*args), 0 if tool == "trace" else 1, "cannot open " + files["missing"])  # the reference's contract: an image message, status 0
    assert not os.path.exists(out)


@pytest.mark.parametrize("tool", TOOLS)
def test_window_on_an_8_bit_stack(files, tool):
    args, out = tool_args(tool, files, files["raw"], files["swc"])
    check(run("--window", "0,100", *args), 1, WINDOW)
    assert not os.path.exists(out)


@pytest.mark.parametrize("tool", WITH_SWC)
def test_malformed_swc(files, tool):
    """alone, and against the two stack messages: --render-swc reads the SWC first, --edt and --geodesic the stack"""
    check(run(*tool_args(tool, files, files["raw"], files["bad"])[0]), 1, bad_line(files))
    first = tool in SWC_FIRST
    check(run(*tool_args(tool, files, files["missing"], files["bad"])[0]), 1, bad_line(files) if first else "cannot open " + files["missing"])
    check(run("--window", "0,100", *tool_args(tool, files, files["raw"], files["bad"])[0]), 1, bad_line(files) if first else WINDOW)


@pytest.mark.parametrize("tool", TOOLS)
def test_valid_input_stops_at_pnr_create(files, tool):
    args, out = tool_args(tool, files, files["raw"], files["swc"])
    check(run(*args), 1, NO_GPU if tool == "trace" else "pnr_create: " + NO_GPU)  # the tracing run prints the bare error
    assert not os.path.exists(out)


def test_swc_tools_fail_before_pnr_create(files):
    """--distance, --join-swc (and the sources of --geodesic): an empty or malformed SWC is reported, not the missing device"""
    out = files["out"] + "_j.swc"
    for swc, line in ((files["bad"], bad_line(files)), (files["empty"], files["empty"] + ": no nodes")):
        check(run("--distance", swc, files["swc"]), 1, line)
        check(run("--distance", files["swc"], swc), 1, line)
        check(run("--join-swc", swc, out), 1, line)
        check(run("--geodesic", "-i", files["raw"], "-d", DIMS, "--from", swc), 1, line)
        assert not os.path.exists(out)
    check(run("--distance", files["swc"], files["swc"]), 1, "pnr_create: " + NO_GPU)
    check(run("--join-swc", files["swc"], out), 1, "pnr_create: " + NO_GPU)
    assert not os.path.exists(out)
