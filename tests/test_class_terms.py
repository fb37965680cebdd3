"""The host arithmetic of cyc_table_classes / cyc_table_cells_at (cyclonus_amd/csrc/class_terms.hpp) on the CPU:
tests/native/class_terms_check.cpp drives the grouping, the status key, the election among failed pods over several rounds
and the first-occurrence numbering against a pairwise row comparison, for every hash mask, and checks the messages of
the list checks.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_terms(tmp_path):
    exe = str(tmp_path / "class_terms_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "cyclonus_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "class_terms_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "class terms: ok" in r.stdout
