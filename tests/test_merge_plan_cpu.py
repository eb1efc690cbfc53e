"""reth_amd/csrc/merge_plan.h (the plans of the closed-form account and storage
merges, the position formulas their kernels call, the lcp patch list, the
interval offsets and the 64-bit merged counts) as a plain host executable:
tests/merge_plan_main.cpp, built with the address and undefined-behaviour
sanitizers. It places every row with the shared formulas and compares the
result with a std::map model. No GPU, nothing loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reth_amd", "csrc")


def test_merge_plans_against_map_model(tmp_path):
    exe = str(tmp_path / "merge_plan_check")
    r = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(HERE, "merge_plan_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failed = (int(x) for x in r.stdout.split()[1::2])
    # account scenarios (2,000 random + 7 by hand) x 4 properties, storage
    # scenarios (2,000 random + 5 by hand) x 3, 1,400 rejected deltas, 4 count
    # limits, 200 interval sets, and the 16 named scenarios, each hit at
    # least once
    assert failed == 0 and checked == 2_007 * 4 + 2_005 * 3 + 1_400 + 4 + 200 + 16, \
        r.stdout
