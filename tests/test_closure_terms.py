"""The host arithmetic of cyc_table_closure / cyc_table_zones (cyclonus_amd/csrc/closure_terms.hpp) on the CPU:
tests/native/closure_terms_check.cpp checks the argument messages, the scratch pitch, the check of the representatives the
zone pass delivers and the canonical zone numbering against zones found pair by pair.  A stand-alone program under
ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closure_terms(tmp_path):
    exe = str(tmp_path / "closure_terms_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "cyclonus_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "closure_terms_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "closure terms: ok" in r.stdout
