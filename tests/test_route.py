"""The path rules (cyclonus_amd/csrc/route.hpp) on the host: tests/native/route_check.cpp holds hand-written
RouteIn cases on both sides of every threshold and the five named workloads' whole routes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_rules(tmp_path):
    exe = str(tmp_path / "route_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cyclonus_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "route_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "route rules: ok" in r.stdout
