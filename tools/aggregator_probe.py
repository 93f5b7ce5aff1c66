#!/usr/bin/env python3
"""Times ccmi_aggregator at C2 size: E = 1,000,000 entities in 30,000 groups, M = 9 (KafkaMetricDef's common metrics),
5 windows, 4 samples per window.

Six windows are fed (five stable ones and the current one), each as four batches that hold one sample of every entity
except a random 5 % (so some windows come out short of samples and the extrapolations occur). Timed, as medians over
--repeats calls after a warm-up: one add_samples batch (the C call: the host pass over the timestamps, the copies in,
the four launches, one synchronise; the batches of the feed itself are the repetitions), completeness, aggregate with
all rows, and the capacity = 0 sizing call. A numpy mirror of counts and values is kept while feeding (a batch names an
entity at most once, so the mirror's update is vectorised too); the same aggregate computed from the mirror with
vectorised numpy is the baseline, and before anything is timed it must equal the device's rows bit for bit.

    python tools/aggregator_probe.py [--repeats K] [--entities E] [--groups G]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
import ccmi  # noqa: E402

NUM_WINDOWS, WINDOW_MS, MIN_SAMPLES, PER_WINDOW = 5, 300_000, 4, 4
LONG_MAX = (1 << 63) - 1
f32, f64 = np.float32, np.float64


class Mirror:
    """counts[a][e] and values[a][m][e] as RawMetricValues keeps them, for batches that name an entity once."""

    def __init__(self, num_entities, fns):
        self.L = NUM_WINDOWS + 1
        self.fns = np.asarray(fns)
        self.counts = np.zeros((self.L, num_entities), dtype=np.int32)
        self.values = np.zeros((self.L, len(fns), num_entities), dtype=f32)
        self.current = self.oldest = 0

    def add(self, entities, window, samples):
        if window > self.current:  # maybeRollOutNewWindow
            new_oldest = max(1, window - NUM_WINDOWS)
            for w in range(self.oldest, self.oldest + min(self.L, new_oldest - self.oldest)):
                self.counts[w % self.L] = 0
            self.oldest, self.current = new_oldest, window
        a = window % self.L
        c = self.counts[a, entities]
        for m, fn in enumerate(self.fns):
            old, s = self.values[a, m, entities].astype(f64), samples[:, m]
            new = s if fn == ccmi.AGG_LATEST else np.where(c == 0, s, old + s if fn == ccmi.AGG_AVG else np.maximum(old, s))
            self.values[a, m, entities] = new.astype(f32)
        self.counts[a, entities] = c + 1

    def aggregate(self, windows):
        """RawMetricValues.aggregate over `windows` for every entity: values [E][M][Wv] and codes [E][Wv]."""
        L, counts, values = self.L, self.counts, self.values
        half = max(1, MIN_SAMPLES // 2)
        first, last = self.oldest % L, (self.oldest + L - 2) % L
        avg = (self.fns == ccmi.AGG_AVG)[:, None]
        num_entities = counts.shape[1]
        out = np.zeros((num_entities, len(self.fns), len(windows)), dtype=f32)
        ext = np.zeros((num_entities, len(windows)), dtype=np.uint8)
        for j, w in enumerate(windows):
            a = w % L
            c = counts[a]
            plain = np.where(c == 0, f32(0), np.where(avg, values[a] / np.maximum(c, 1).astype(f32), values[a]))
            enough = c >= half
            if a != first and a != last:
                p, n = (a + L - 1) % L, (a + 1) % L
                adjacent = ~enough & (counts[p] >= MIN_SAMPLES) & (counts[n] >= MIN_SAMPLES)
                total = ((values[p] + np.where(c == 0, f32(0), values[a])) + values[n]).astype(f64)
                adjacent_value = np.where(avg, total / (counts[p] + c + counts[n]).astype(f64),
                                          total / np.where(c > 0, 3.0, 2.0)).astype(f32)
            else:
                adjacent, adjacent_value = np.zeros(num_entities, dtype=bool), f32(0)
            forced = ~enough & ~adjacent & (c > 0)
            out[:, :, j] = np.where(enough | forced, plain, np.where(adjacent, adjacent_value, f32(0))).T
            ext[:, j] = np.where(enough, np.where(c < MIN_SAMPLES, 1, 0), np.where(adjacent, 2, np.where(forced, 3, 4)))
        return out, ext


def median_ms(call, repeats, warmup=3):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(t), 3), ms_min_max=[round(min(t), 3), round(max(t), 3)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=30_000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    E, G = args.entities, args.groups
    rng = np.random.default_rng(1)
    fns = [f for _, f in ccmi.KAFKA_COMMON_METRICS]
    M = len(fns)
    group = rng.integers(0, G, E).astype(np.int32)
    agg = ccmi.MetricSampleAggregator(NUM_WINDOWS, WINDOW_MS, MIN_SAMPLES, fns, group, G, device=args.device)
    mirror = Mirror(E, fns)
    add_ms = []
    for window in range(1, NUM_WINDOWS + 2):
        for k in range(PER_WINDOW):
            ents = rng.permutation(E)[:int(E * 0.95)].astype(np.int32)
            times = np.full(ents.size, (window - 1) * WINDOW_MS + k, dtype=np.int64)
            samples = rng.uniform(0.0, 1e6, (ents.size, M))
            t0 = time.perf_counter()
            accepted = agg.add_samples(ents, times, samples)
            add_ms.append((time.perf_counter() - t0) * 1e3)
            assert accepted.all()
            mirror.add(ents, window, samples)
    options = ccmi.AggregationOptions(0.5, 0.0, 1, NUM_WINDOWS, ccmi.GRANULARITY_ENTITY, True)
    res = agg.aggregate(-1, LONG_MAX, options)
    windows = res.completeness.valid_window_indices.tolist()
    t0 = time.perf_counter()
    want_values, want_ext = mirror.aggregate(windows)
    first_numpy_ms = (time.perf_counter() - t0) * 1e3
    same = bool(res.num_entities == len(res.entities) and
                np.array_equal(res.values.view(np.uint32), want_values[res.entities].view(np.uint32)) and
                np.array_equal(res.extrapolations, want_ext[res.entities]))
    codes = np.bincount(res.extrapolations.reshape(-1), minlength=5).tolist()

    # the C calls on buffers allocated once (the binding adds allocations and slices)
    s, arrays = agg._completeness_struct(np)
    o = options.struct()
    n = C.c_int64(0)
    cap = res.num_entities
    ent, val = np.zeros(cap, dtype=np.int32), np.zeros(cap * M * NUM_WINDOWS, dtype=f32)
    ext, inv = np.zeros(cap * NUM_WINDOWS, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
    L = agg.lib.lib

    def completeness():
        agg.lib.check(L.ccmi_aggregator_completeness_query(agg.handle, -1, LONG_MAX, C.byref(o), None, C.byref(s), None, None))

    def aggregate(capacity):
        agg.lib.check(L.ccmi_aggregator_aggregate(agg.handle, -1, LONG_MAX, C.byref(o), None, C.byref(s), ent.ctypes.data,
                                                  val.ctypes.data, ext.ctypes.data, inv.ctypes.data, capacity, C.byref(n)))

    out = dict(entities=E, groups=G, metrics=M, windows=NUM_WINDOWS, samples_per_window=PER_WINDOW, repeats=args.repeats,
               batch_samples=int(E * 0.95), valid_windows=len(windows), rows=int(res.num_entities),
               extrapolation_counts=codes, out_bytes=int(cap * (M * len(windows) * 4 + len(windows) + 5)),
               same_answer=same,
               add_samples=dict(ms=round(statistics.median(add_ms[1:]), 3), batches=len(add_ms) - 1,
                                ms_min_max=[round(min(add_ms[1:]), 3), round(max(add_ms[1:]), 3)],
                                first_ms=round(add_ms[0], 3)),
               completeness=median_ms(completeness, args.repeats),
               aggregate_all_rows=median_ms(lambda: aggregate(cap), args.repeats),
               aggregate_sizing_call=median_ms(lambda: aggregate(0), args.repeats),
               numpy_aggregate=dict(median_ms(lambda: mirror.aggregate(windows), max(3, args.repeats // 4), warmup=1),
                                    first_ms=round(first_numpy_ms, 3)))
    print(json.dumps(out), flush=True)
    if not same:
        sys.exit("the device's rows differ from the numpy computation over the mirrored counts and values")


if __name__ == "__main__":
    main()
