"""The C++ unit check of engine/percentile.h (tests/cpp/test_percentile.cpp): the header the K19 kernels compile, built
for the host with g++ -ffp-contract=off and run on cases the Python restatement (tests/metric_anomaly_support.py)
recorded: the hand-derived percentile cases, seeded random ones (ties, NaNs, infinities, signed zeros, every n up to the
aggregator's 31 windows and a few long ones) and the sufficiency minima. The program compares bit for bit. CPU only."""
import math
import os
import random
import struct
import subprocess

import metric_anomaly_support as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERCENTILES = (0.01, 1.0, 2.0, 5.0, 10.0, 25.0, 50.0, 75.0, 90.0, 95.0, 99.0, 99.99, 100.0)


def _bits(v):
    return "%x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _pct(values, p):
    return "pct %s %d %s %s" % (_bits(p), len(values), " ".join(_bits(v) for v in values),
                                _bits(A.percentile(list(values), p)))


def script(seed):
    rng = random.Random(seed)
    ten = [float(v) for v in range(1, 11)]
    lines = [_pct(ten, 90), _pct(ten, 95), _pct(ten, 5), _pct([1.0, 2.0, 3.0, 4.0], 50), _pct([], 50), _pct([7.0], 1),
             _pct([float("nan")], 50), _pct([float("nan"), 3.0, float("nan"), 1.0], 50),
             _pct([float("nan"), float("nan")], 50), _pct(ten, 100), _pct([0.0, -0.0, 0.0], 50),
             _pct([1.0, math.inf], 50), _pct([-math.inf, math.inf, 0.0], 50)]
    for n in list(range(0, 32)) + [64, 257, 1000]:
        for _ in range(6 if n <= 31 else 2):
            kind = rng.randrange(5)
            if kind == 0:
                vals = [rng.uniform(-1e3, 1e6) for _ in range(n)]
            elif kind == 1:
                vals = [float(rng.randrange(0, 4)) for _ in range(n)]  # ties
            elif kind == 2:
                vals = [rng.choice([float("nan"), rng.uniform(0, 10), 0.0, -0.0]) for _ in range(n)]
            elif kind == 3:
                vals = [float(A.S.f32(rng.uniform(0, 1e5))) for _ in range(n)]  # float32 values, as the rows hold
            else:
                vals = [rng.choice([math.inf, -math.inf, rng.uniform(-1, 1), 1e-310]) for _ in range(n)]
            for p in rng.sample(PERCENTILES, 4):
                lines.append(_pct(vals, p))
    for p in (90.0, 95.0, 50.0, 2.0, 0.0, 100.0, 99.99, 0.01, 50.000001, 33.3, 66.7, 75.0):
        lines.append("min %s %d" % (_bits(p), A.min_num_values(p)))
        for count in (0, 1, 2, 9, 10, 11, 19, 20, 31, 49, 50, 10000, A.INT_MAX):
            other = rng.choice(PERCENTILES[:-1])
            lines.append("suf %d %s %s %d" % (count, _bits(p), _bits(other),
                                              1 if A.is_data_sufficient(count, p, other) else 0))
    return lines


def test_percentile_header(tmp_path):
    path = tmp_path / "percentile_script.txt"
    lines = script(2026)
    path.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_percentile")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "cruise-control_amd", "csrc", "engine"),
                    os.path.join(REPO, "tests", "cpp", "test_percentile.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "percentile ok: %d cases" % len(lines) in r.stdout
