"""The C++ unit checks of engine/keyed_table.h (tests/cpp/test_keyed_table.cpp): built with g++ and run, CPU only."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyed_table_mirror(tmp_path):
    exe = str(tmp_path / "test_keyed_table")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(REPO, "cruise-control_amd", "csrc", "engine"),
                    os.path.join(REPO, "tests", "cpp", "test_keyed_table.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "keyed table ok" in r.stdout
