"""The host arithmetic of cyc_table_reach (cyclonus_amd/csrc/reach_terms.hpp) on the CPU: tests/native/reach_terms_check.cpp
checks the seed validation and its messages, the seed lists as bitsets against a per-pod tally, the working-set limit and
`levels` from per-hop counters of a search written out pod by pod.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reach_terms(tmp_path):
    exe = str(tmp_path / "reach_terms_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "cyclonus_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "reach_terms_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reach terms: ok" in r.stdout
