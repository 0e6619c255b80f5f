"""Randomised parity campaign (tests/fuzzcase.py) on the GPU box: random small stacks and parameters, HIP path against the oracle
stage by stage; every comparison is for equality of bytes.
usage: fuzz_parity.py [--images CLASS[,CLASS]] [seconds] [first_case]     FUZZ_DRIVER=persistent  FUZZ_BIG=1 (stacks up to 192 x 160 x 80)
--images: the stacks come from tests/imgclass.py (the named classes in turn; "all": every class) instead of the synthetic tubes"""
import os, sys, time, traceback
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tests'))
import orc, fuzzcase, imgclass

argv = sys.argv[1:]
images = None
if "--images" in argv:
    i = argv.index("--images")
    images = list(imgclass.CLASSES) if argv[i + 1] == "all" else argv[i + 1].split(",")
    assert all(k in imgclass.CLASSES for k in images), f"--images: classes are {imgclass.CLASSES}"
    del argv[i:i + 2]
budget = float(argv[0]) if len(argv) > 0 else 300.0
case = int(argv[1]) if len(argv) > 1 else 0
L = orc.load_oracle()
t_end = time.time() + budget
nbad = ncases = 0
stats = {}
while time.time() < t_end:
    desc = {}
    try:
        fuzzcase.run_case(L, case, stats, desc, driver=os.environ.get("FUZZ_DRIVER"), big=bool(os.environ.get("FUZZ_BIG")), images=images)
    except Exception as e:  # noqa
        nbad += 1
        print("MISMATCH", desc, "->", repr(e)[:300], flush=True)
        if not isinstance(e, AssertionError): traceback.print_exc()
    ncases += 1; case += 1
    if ncases % 10 == 0: print(f"[{ncases} cases, {nbad} bad] {stats}", flush=True)
print(f"done: {ncases} cases, {nbad} mismatches, {stats}, next case {case}")
sys.exit(1 if nbad else 0)
