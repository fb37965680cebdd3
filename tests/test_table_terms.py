"""The host arithmetic of the device-table entry points (cyclonus_amd/csrc/table_terms.hpp) on the CPU:
tests/native/table_terms_check.cpp builds the counters a kernel pass would deliver cell by cell, runs the terms
functions on them and compares every output with a per-cell tally; GroupTables, find's paging and the group argument
checks on their own.  A stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_terms(tmp_path):
    exe = str(tmp_path / "table_terms_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "cyclonus_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "table_terms_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "table terms: ok" in r.stdout
