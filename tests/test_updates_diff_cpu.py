"""reth_amd/csrc/updates_diff.h (the TrieUpdates row order, the snapshot
compare and the incremental net diff) as a plain host executable:
tests/updates_diff_main.cpp, built with the address and undefined-behaviour
sanitizers. It checks that row_less and snap_cmp are one order and the net
diff against a std::map model. No GPU, nothing loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reth_amd", "csrc")


def test_order_agreement_and_net_diff_model(tmp_path):
    exe = str(tmp_path / "updates_diff_check")
    r = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(HERE, "updates_diff_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failed = (int(x) for x in r.stdout.split()[1::2])
    # 200,000 row pairs + 2,000 scenarios x 5 properties + the 10 ways a
    # row can go through the merge loop, each taken at least once
    assert failed == 0 and checked == 200_000 + 2_000 * 5 + 10, r.stdout
