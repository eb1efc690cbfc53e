"""reth_amd/csrc/revert_plan.h (the row decisions of the revert capture and
the positions of its storage rows, which the k_rv_* kernels call) as a
plain host executable: tests/revert_plan_main.cpp, built with the address
and undefined-behaviour sanitizers. It places every revert row with the
shared functions and compares the result with a std::map model; on unsorted
and duplicate deltas it checks that every position stays below the total.
No GPU, nothing loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reth_amd", "csrc")


def test_revert_positions_against_map_model(tmp_path):
    exe = str(tmp_path / "revert_plan_check")
    r = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(HERE, "revert_plan_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failed = (int(x) for x in r.stdout.split()[1::2])
    # valid scenarios (3,000 random + 9 by hand) x 4 properties, 1,500
    # unsorted or duplicate deltas x the bounds, and the 11 named
    # scenarios, each hit at least once
    assert failed == 0 and checked == 3_009 * 4 + 1_500 + 11, r.stdout
