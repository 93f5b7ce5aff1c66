"""The C++ unit check of engine/aggregator_entity.h (tests/cpp/test_aggregator_entity.cpp): the header the K17 kernels
compile, built for the host with g++ and run on scripts the Python restatement recorded. CPU only.

The scripts are the RawMetricValuesTest cases of tests/golden/metric_aggregator_kat.json plus seeded random call
sequences shaped like an aggregator's (samples into any kept window, roll-outs with and without a leap). After every
call the script carries the restatement's counts, bit words and stored floats, and at intervals its aggregate and
isValid; the program compares bit for bit."""
import json
import os
import random
import struct
import subprocess

import metric_aggregator_support as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dbits(v):
    return "%x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _fbits(v):
    return "%x" % int(S.float_bits([v])[0])


def _word(flags):
    return sum(1 << a for a, f in enumerate(flags) if f)


class Recorder:
    def __init__(self, keep, min_samples, fns):
        self.raw = S.RawMetricValues(keep, min_samples, fns)
        self.lines = ["case %d %d %d %s" % (keep, min_samples, len(fns), " ".join(map(str, fns)))]

    def state(self):
        r = self.raw
        self.lines.append("state %s %d %d" % (" ".join(map(str, r.counts)), _word(r.validity), _word(r.extrapolations)))

    def oldest(self, w):
        self.raw.update_oldest_window_index(w)
        self.lines.append("oldest %d" % w)
        self.state()

    def add(self, w, values):
        try:
            self.raw.add_sample(values, w)
        except ValueError:
            pass  # the header drops what the reference refuses with an exception
        self.lines.append("add %d %s" % (w, " ".join(_dbits(v) for v in values)))
        self.state()
        if self.raw.oldest <= w <= self.raw.current_window_index():
            a = self.raw.array_index(w)
            self.lines.append("values %d %s" % (a, " ".join(_fbits(row[a]) for row in self.raw.values)))

    def reset(self, start, n):
        self.raw.reset_window_indices(start, n)
        self.lines.append("reset %d %d" % (start, n))
        self.state()

    def is_valid(self, mx):
        self.lines.append("isvalid %d %d" % (mx, 1 if self.raw.is_valid(mx) else 0))

    def agg(self, windows):
        values, ext = self.raw.aggregate(windows, check_window=False)
        self.lines.append("agg %d %s %s %s" % (len(windows), " ".join(map(str, windows)), " ".join(map(str, ext)),
                                               " ".join(_fbits(v) for row in values for v in row)))


def kat_scripts():
    kat = json.load(open(os.path.join(REPO, "tests", "golden", "metric_aggregator_kat.json")))["raw"]
    lines = []
    for case in kat["cases"]:
        rec = Recorder(case["keep"], case["min_samples"], kat["functions"])
        for op in case["ops"]:
            if op[0] == "oldest":
                rec.oldest(op[1])
            elif op[0] in ("add", "add_refused"):
                rec.add(op[1], op[2:])
            elif op[0] == "reset":
                rec.reset(op[1], op[2])
            elif op[0] == "is_valid":
                rec.is_valid(op[1])
            elif op[0] == "agg":
                rec.agg(op[1])
        keep = case["keep"]
        rec.agg(list(range(rec.raw.oldest, rec.raw.oldest + keep - 1)))
        for mx in range(keep + 1):
            rec.is_valid(mx)
        lines += rec.lines
    return lines


def random_scripts(seed, cases=12, steps=160):
    rng = random.Random(seed)
    lines = []
    for _ in range(cases):
        num_windows = rng.choice([1, 2, 5, 5, 7, 31])
        keep = num_windows + 1
        min_samples = rng.choice([1, 2, 3, 4, 5])
        fns = [rng.randrange(3) for _ in range(rng.choice([1, 3, 9]))]
        rec = Recorder(keep, min_samples, fns)
        oldest = rng.randrange(0, 40)
        current = oldest + rng.randrange(0, keep)  # the aggregator's, at most the raw values' own
        rec.oldest(oldest)
        for _ in range(steps):
            roll = rng.random()
            if roll < 0.12:  # maybeRollOutNewWindow, sometimes with a leap
                w = current + (rng.randrange(1, 3) if rng.random() < 0.8 else rng.randrange(keep, 3 * keep))
                new_oldest = max(1, w - num_windows)
                n_reset = min(keep, new_oldest - oldest)
                if n_reset > 0:
                    rec.oldest(new_oldest)
                    rec.reset(oldest, n_reset)
                    oldest = new_oldest
                current = w
            else:
                w = rng.randrange(oldest, current + 1)
                if rng.random() < 0.6:  # concentrate, so windows fill up
                    w = max(oldest, current - rng.randrange(0, 3))
                vals = [rng.choice([rng.uniform(-50.0, 1e4), float(rng.randrange(0, 100)), 1e-3 * rng.random(), -0.0, 0.0])
                        for _ in fns]
                rec.add(w, vals)
            if rng.random() < 0.25:
                rec.agg(list(range(oldest, oldest + keep)))  # every kept window, the current one too
                rec.is_valid(rng.randrange(0, keep + 1))
        lines += rec.lines
    return lines


def test_aggregator_entity_header(tmp_path):
    script = tmp_path / "aggregator_entity_script.txt"
    lines = kat_scripts() + random_scripts(20261)
    script.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_aggregator_entity")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "cruise-control_amd", "csrc", "engine"),
                    os.path.join(REPO, "tests", "cpp", "test_aggregator_entity.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "aggregator entity ok" in r.stdout
