"""The C++ unit check of engine/replica_load.h (tests/cpp/test_replica_load.cpp): the header the K18 kernels compile,
built for the host with g++ and run on partitions whose expected loads the oracle's restatement of
MonitorUtils.populatePartitionLoad (oc_ingest_partition, oracle/src/ingest.cpp) recorded. The oracle walks a partition's
replicas over one shared, mutated values object; the header computes every replica on its own. CPU only, bit for bit.

Covered, and asserted on the script: every replica count 1..8 with the leader first, in the middle and last, every
W 1..5, reported and unreported replication-bytes-out, all-zero byte rates (follower CPU 0), and CPU values whose x100
does not survive the round trip through float."""
import ctypes as C
import os
import random
import struct
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU, DISK, LBI, LBO, RBI, RBO = range(6)


def _f32(v):
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _bits(v):
    return "%x" % struct.unpack("<I", struct.pack("<f", v))[0]


def _oracle(oracle_lib, W, flags, lead):
    n = len(flags)
    out = (C.c_float * (n * 6 * W))()
    oracle_lib.oc_ingest_partition.restype = C.c_int32
    oracle_lib.oc_ingest_partition(W, n, (C.c_uint8 * n)(*flags), (C.c_float * len(lead))(*lead), out)
    return list(out)


def _cpu_rounds(v):
    """(float)(v * 100.0) / 100 is not v again: the percentage is not exact in float."""
    return _f32(_f32(v * 100.0) / 100.0) != v


def script(oracle_lib, seed=20262):
    rng = random.Random(seed)
    lines, seen = [], dict(unreported=0, reported=0, idle=0, inexact_cpu=0, positions=set(), windows=set())
    for n in range(1, 9):
        for leader in sorted({0, n // 2, n - 1}):
            for W in range(1, 6):
                for kind in ("reported", "unreported", "idle"):
                    lead = [[_f32(rng.uniform(0.0, 5e4)) for _ in range(W)] for _ in range(6)]
                    lead[CPU] = [_f32(rng.uniform(0.0, 0.9)) for _ in range(W)]
                    if kind == "unreported":
                        lead[RBO] = [0.0] * W
                    if kind == "idle":
                        for m in (LBI, LBO, RBI, RBO):
                            lead[m] = [0.0] * W
                    if rng.random() < 0.2:  # one idle window among busy ones
                        w = rng.randrange(W)
                        for m in (LBI, LBO, RBI, RBO):
                            lead[m][w] = 0.0
                    flat = [x for row in lead for x in row]
                    flags = [1 if i == leader else 0 for i in range(n)]
                    want = _oracle(oracle_lib, W, flags, flat)
                    lines.append("case %d %d %d" % (W, n, leader))
                    lines.append("lead " + " ".join(_bits(x) for x in flat))
                    lines.append("want " + " ".join(_bits(x) for x in want))
                    seen[kind] += 1
                    seen["inexact_cpu"] += sum(1 for v in lead[CPU] if _cpu_rounds(v))
                    seen["windows"].add(W)
                    seen["positions"].add((n, "first" if leader == 0 else "last" if leader == n - 1 else "middle"))
                    if kind == "idle" and n > 1:  # a follower of an idle partition has CPU 0
                        follower = 1 if leader == 0 else 0
                        assert all(want[(follower * 6 + CPU) * W + w] == 0.0 for w in range(W))
                    if kind == "reported" and 0 < leader < n - 1:
                        # the follower before the leader and the one after it differ exactly by the filled value
                        before, after = want[CPU * W:(CPU + 1) * W], want[((n - 1) * 6 + CPU) * W:((n - 1) * 6 + CPU + 1) * W]
                        seen["order_matters"] = seen.get("order_matters", 0) + (before != after)
    return lines, seen


def test_replica_load_header(tmp_path, oracle_lib):
    lines, seen = script(oracle_lib)
    assert seen["windows"] == {1, 2, 3, 4, 5}
    assert {n for n, _ in seen["positions"]} == set(range(1, 9))
    assert all((n, where) in seen["positions"] for n in range(3, 9) for where in ("first", "middle", "last"))
    assert seen["reported"] and seen["unreported"] and seen["idle"] and seen["inexact_cpu"] and seen["order_matters"]
    path = tmp_path / "replica_load_script.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_replica_load")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "cruise-control_amd", "csrc", "engine"),
                    os.path.join(REPO, "tests", "cpp", "test_replica_load.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "replica load ok: %d partitions" % (len(lines) // 3) in r.stdout
