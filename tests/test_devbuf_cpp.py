"""The C++ unit check of engine/devbuf.h (tests/cpp/test_devbuf.cpp): the header every query workspace is owned and laid
out with, built for the host with g++ over allocation functions backed by malloc. Carver: the sizing pass equals the
placing pass, every piece is 256-byte aligned, pieces do not overlap and each owns its size rounded up to 256 bytes, for
counts 0, 1, 63, 64, 65 of 1-, 4-, 8- and 24-byte elements. DevBuf / PinBuf: the growth rule, one free per regrowth, moves,
and an allocator that throws; carve's two passes. CPU only."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_header(tmp_path):
    exe = str(tmp_path / "test_devbuf")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I",
                    os.path.join(REPO, "cruise-control_amd", "csrc", "engine"),
                    os.path.join(REPO, "tests", "cpp", "test_devbuf.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "devbuf ok: " in r.stdout
