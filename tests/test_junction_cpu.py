"""reth_amd/csrc/junction.h (the key compare the storage leaf kernel runs on
its LE-loaded key words) against a byte-wise nibble loop, as a plain host
executable: tests/junction_main.cpp, built with the address and
undefined-behaviour sanitizers. No GPU, nothing loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reth_amd", "csrc")


def test_junction_matches_nibble_loop(tmp_path):
    exe = str(tmp_path / "junction_check")
    r = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(HERE, "junction_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failed = (int(x) for x in r.stdout.split()[1::2])
    # 8 x 65 positions x (2 + 2 + 4 x 64) + 4 + 4 x 64 + 2 x 1M
    assert failed == 0 and checked == 8 * 65 * 260 + 260 + 2_000_000, r.stdout
