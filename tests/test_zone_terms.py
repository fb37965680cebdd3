"""The host arithmetic of cyc_table_zone_graph (cyclonus_amd/csrc/zone_terms.hpp) on the CPU:
tests/native/zone_terms_check.cpp checks the argument and capacity messages, the plane sizes, the zones' smallest pods and
sizes, the check of the edge list the device delivers and the tiers against longest chains on random DAGs, a cycle
included.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zone_terms(tmp_path):
    exe = str(tmp_path / "zone_terms_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "cyclonus_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "zone_terms_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "zone terms: ok" in r.stdout
