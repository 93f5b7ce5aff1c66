#!/usr/bin/env python3
"""Times the two metric anomaly finders on the device against the host path a caller had before them.

Shape: 10,000 brokers on 5,000 hosts, M = 32 broker metrics (the order of KafkaMetricDef's broker metric set; the eight
the reference's KafkaMetricAnomalyFinderTest names are interested), 20 history windows and the current one, one sample
per broker and window. About 1 % of the brokers are slow now (log flush time times 4 to 6), 2 % carry negligible
traffic, 1 % have a latency spike.

Measured, as medians over --repeats calls after a warm-up:
  device : MetricSampleAggregator.metric_anomalies (95 / 5 / 0.5 / 0.2) and SlowBrokerFinder.detect (the defaults,
           log flush threshold 150 ms), each one Python call; the rows never leave the device;
  host   : aggregate + peek_current_window copied out (what a caller had to do), then a vectorised numpy restatement
           of the finder over those rows (legacy_percentile below: sort along the window axis, the LEGACY position,
           two gathers). The copy-out and the numpy part are reported separately and summed.
Before anything is timed the two sides must agree: the same records bit for bit, the same reported brokers, scores and
peer bases (from fresh scores on both sides).

    python tools/anomaly_probe.py [--repeats K] [--brokers E] [--metrics M] [--windows W]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
import ccmi  # noqa: E402

WINDOW_MS = 300_000
LONG_MAX = (1 << 63) - 1
FLUSH, IN, REPL, LATENCY = 0, 1, 2, 3
f32, f64 = np.float32, np.float64
INT_MAX = 2 ** 31 - 1


def min_num_values(p):
    den = 100.0 - p if p > 50.0 else p
    return INT_MAX if den == 0.0 else min(INT_MAX, int(np.ceil(100.0 / den)))


def legacy_percentile(ordered, n, p):
    """commons-math3 Percentile (LEGACY) per row: ordered [R][W] ascending with the row's n values first, no NaN."""
    width = ordered.shape[1]
    q = p / 100.0
    nf = n.astype(f64)
    pos = nf if q == 1.0 else q * (nf + 1.0)
    fl = np.floor(pos)
    k = fl.astype(np.int64)

    def take(i):
        return np.take_along_axis(ordered, np.clip(i, 0, width - 1)[:, None], axis=1)[:, 0]

    with np.errstate(invalid="ignore"):
        lo, hi = take(k - 1), take(k)
        mid = lo + (pos - fl) * (hi - lo)
    return np.where(pos < 1.0, ordered[:, 0], np.where(pos >= nf, take(n - 1), mid))


def host_rows(agg):
    res = agg.aggregate(-1, LONG_MAX, ccmi.AggregationOptions(0.0, 0.0, 1, 5, ccmi.GRANULARITY_ENTITY, False))
    ents, values, _, _ = agg.peek_current_window()
    return res, ents, values


def host_percentile(res, cur_ents, cur_values, num_entities, interested, upper, lower, upper_margin, lower_margin):
    wv = res.values.shape[2] if res.num_entities else 0
    if res.num_entities == 0 or wv < max(min_num_values(upper), min_num_values(lower)):
        return np.zeros(0, dtype=ccmi.METRIC_ANOMALY_DTYPE)
    row_of = np.full(num_entities, -1, dtype=np.int64)
    row_of[res.entities] = np.arange(res.num_entities)
    h = row_of[cur_ents]
    with_history = np.flatnonzero(h >= 0)
    metrics = np.flatnonzero(interested)
    hist = res.values[h[with_history]][:, metrics, :].astype(f64)  # [R][Mi][Wv]
    rows, mi = hist.shape[0], metrics.size
    ordered = np.sort(hist.reshape(rows * mi, wv), axis=1)
    n = np.full(rows * mi, wv, dtype=np.int64)
    u = legacy_percentile(ordered, n, upper)
    hi = u * (1.0 + upper_margin)
    lo = legacy_percentile(ordered, n, lower) * lower_margin
    cur = cur_values[with_history][:, metrics].astype(f64).reshape(-1)
    hit = np.flatnonzero(~(u <= 1.0) & ((cur > hi) | (cur < lo)))
    out = np.zeros(hit.size, dtype=ccmi.METRIC_ANOMALY_DTYPE)
    out["entity"] = cur_ents[with_history][hit // mi]
    out["metric"] = metrics[hit % mi]
    out["current"], out["upper_threshold"], out["lower_threshold"] = cur[hit], hi[hit], lo[hit]
    return out


class HostSlowBrokerFinder:
    """SlowBrokerFinder over the copied-out rows, vectorised; the scores are numpy arrays over the brokers."""

    def __init__(self, num_entities, flush_threshold, bytes_threshold=1024.0, hp=90.0, hm=3.0, pp=50.0, pm=3.0,
                 demotion=5, decommission=50, ratio=0.1):
        self.E = num_entities
        self.flush_threshold, self.bytes_threshold = flush_threshold, bytes_threshold
        self.hp, self.hm, self.pp, self.pm = hp, hm, pp, pm
        self.demotion, self.decommission, self.ratio = demotion, decommission, ratio
        self.score = np.zeros(num_entities, dtype=np.int32)
        self.since = np.zeros(num_entities, dtype=np.int64)
        self.has = np.zeros(num_entities, dtype=bool)

    def _history_hits(self, values, keep, cur):
        ordered = np.sort(np.where(keep, values, np.inf), axis=1)
        n = keep.sum(axis=1)
        enough = n >= min_num_values(self.hp)
        return enough & (cur > legacy_percentile(ordered, np.maximum(n, 1), self.hp) * self.hm)

    def _peer_hits(self, cur, active):
        n = int(active.sum())
        if n < min_num_values(self.pp):
            return np.zeros(cur.size, dtype=bool), float("nan")
        ordered = np.sort(cur[active])[None, :]
        base = float(legacy_percentile(ordered, np.array([n]), self.pp)[0])
        return active & (cur > base * self.pm), base

    def detect(self, res, cur_ents, cur_values, time_ms):
        bytes_now = (cur_values[:, IN] + cur_values[:, REPL]).astype(f64)  # a float sum, widened afterwards
        active = ~(bytes_now < self.bytes_threshold)
        flush = cur_values[:, FLUSH].astype(f64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per_byte = flush / bytes_now
        row_of = np.full(self.E, -1, dtype=np.int64)
        row_of[res.entities] = np.arange(res.num_entities)
        h = row_of[cur_ents]
        sel = np.flatnonzero((h >= 0) & active)
        hit_flush, hit_per_byte = np.zeros(cur_ents.size, dtype=bool), np.zeros(cur_ents.size, dtype=bool)
        if sel.size:
            hv = res.values[h[sel]]
            hf = hv[:, FLUSH, :].astype(f64)
            total = hv[:, IN, :].astype(f64) + hv[:, REPL, :].astype(f64)
            hit_flush[sel] = self._history_hits(hf, hf > 5.0, flush[sel])
            with np.errstate(divide="ignore", invalid="ignore"):
                hit_per_byte[sel] = self._history_hits(hf / total, total >= self.bytes_threshold, per_byte[sel])
        peer_flush, base_flush = self._peer_hits(flush, active)
        peer_per_byte, base_per_byte = self._peer_hits(per_byte, active)
        suspect_rows = active & (hit_flush | peer_flush) & (hit_per_byte | peer_per_byte) & (flush > self.flush_threshold)
        suspect = np.zeros(self.E, dtype=bool)
        suspect[cur_ents[suspect_rows]] = True
        fresh = suspect & ~self.has
        self.since[fresh] = time_ms
        self.score = np.where(fresh, 1, np.where(suspect, np.minimum(self.score + 1, self.decommission),
                                                 np.where(self.has, self.score - 1, self.score))).astype(np.int32)
        self.has = suspect | (self.has & (self.score != 0))
        self.score[~self.has] = 0
        self.since[~self.has] = 0
        remove = suspect & (self.score == self.decommission)
        demote = suspect & ~remove & (self.score >= self.demotion)
        reported = np.flatnonzero(remove | demote)
        out = np.zeros(reported.size, dtype=ccmi.SLOW_BROKER_DTYPE)
        out["entity"], out["kind"] = reported, np.where(remove[reported], 2, 1)
        out["score"], out["since_ms"] = self.score[reported], self.since[reported]
        unfixable = reported.size > res.num_entities * self.ratio
        return out, (base_flush, base_per_byte), bool(unfixable), int(active.sum())


def median_ms(call, repeats, warmup=2):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(t), 3), ms_min_max=[round(min(t), 3), round(max(t), 3)])


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--brokers", type=int, default=10_000)
    ap.add_argument("--metrics", type=int, default=32)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    E, M, W = args.brokers, args.metrics, args.windows
    rng = np.random.default_rng(19)
    fns = [ccmi.AGG_AVG] * M
    agg = ccmi.MetricSampleAggregator(W, WINDOW_MS, 1, fns, np.arange(E, dtype=np.int32) // 2, (E + 1) // 2,
                                      device=args.device)
    slow = rng.random(E) < 0.01
    quiet = rng.random(E) < 0.02
    spike = rng.random(E) < 0.01
    ents = np.arange(E, dtype=np.int32)
    for w in range(1, W + 2):
        v = rng.uniform(5.0, 50.0, (E, M))
        v[:, FLUSH] = 100.0 + rng.integers(-25, 26, E)
        v[:, IN] = 4096.0 + rng.integers(-400, 401, E)
        v[:, REPL] = 4096.0 + rng.integers(-400, 401, E)
        v[quiet, IN] = v[quiet, REPL] = 300.0
        if w == W + 1:
            v[slow, FLUSH] *= rng.integers(4, 7, int(slow.sum()))
            v[spike, LATENCY] *= 4.0
        assert agg.add_samples(ents, np.full(E, (w - 1) * WINDOW_MS + 7, dtype=np.int64), v).all()
    interested = np.zeros(M, dtype=np.uint8)
    interested[[FLUSH, LATENCY] + list(range(4, min(M, 10)))] = 1
    config = (95.0, 5.0, 0.5, 0.2)
    finder = ccmi.SlowBrokerFinder(agg, FLUSH, IN, REPL, log_flush_time_threshold_ms=150.0, demotion_score=0)

    # the same answer first, from fresh scores
    got = agg.metric_anomalies(LONG_MAX, interested, *config)
    res, cur_ents, cur_values = host_rows(agg)
    want = host_percentile(res, cur_ents, cur_values, E, interested, *config)
    same_percentile = same_bits(got.records, want) and got.num_anomalies == want.size
    host = HostSlowBrokerFinder(E, 150.0, demotion=0)
    d = finder.detect(1000, to_ms=LONG_MAX)
    want_brokers, want_bases, want_unfixable, want_active = host.detect(res, cur_ents, cur_values, 1000)
    same_slow = (same_bits(d.brokers, want_brokers) and bool(d.summary.unfixable) == want_unfixable and
                 d.summary.num_active == want_active and
                 np.array([d.summary.peer_base_log_flush, d.summary.peer_base_per_byte]).tobytes() ==
                 np.array(want_bases).tobytes())

    def host_percentile_path():
        r, ce, cv = host_rows(agg)
        return host_percentile(r, ce, cv, E, interested, *config)

    def host_slow_path():
        r, ce, cv = host_rows(agg)
        return host.detect(r, ce, cv, 2000)

    repeats = args.repeats
    out = dict(brokers=E, metrics=M, interested_metrics=int(interested.sum()), history_windows=W, repeats=repeats,
               anomalies=int(got.num_anomalies), reported_brokers=int(d.num_brokers), active=int(d.summary.num_active),
               skipped=int(d.summary.num_skipped), same_percentile=bool(same_percentile), same_slow=bool(same_slow),
               device_metric_anomalies=median_ms(lambda: agg.metric_anomalies(LONG_MAX, interested, *config), repeats),
               device_detect=median_ms(lambda: finder.detect(2000, to_ms=LONG_MAX), repeats),
               host_copy_out=median_ms(lambda: host_rows(agg), repeats),
               host_numpy_percentile=median_ms(
                   lambda: host_percentile(res, cur_ents, cur_values, E, interested, *config), repeats),
               host_numpy_detect=median_ms(lambda: host.detect(res, cur_ents, cur_values, 2000), repeats),
               host_metric_anomalies=median_ms(host_percentile_path, repeats),
               host_detect=median_ms(host_slow_path, repeats))
    print(json.dumps(out), flush=True)
    if not (same_percentile and same_slow):
        sys.exit("the device's answer differs from the numpy restatement over the copied-out rows")


if __name__ == "__main__":
    main()
