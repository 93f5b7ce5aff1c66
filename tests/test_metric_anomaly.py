"""ccmi_aggregator_metric_anomalies and ccmi_slow_broker_finder on the device (kernels/anomaly.hip) against the
plain-Python restatement of the reference's finders (tests/metric_anomaly_support.py) over the rows of the aggregator
restatement, both sides fed the same add_samples calls. Integers and masks are compared exactly, doubles as bit
patterns with -0.0 equal to 0.0 (Percentile selects with <). There is no tolerance.
"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import ccmi
import metric_aggregator_support as S
import metric_anomaly_support as A

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "cruise-control_amd", "csrc", "engine", "devtypes.h")) as _f:
    _DEVTYPES = _f.read()
BLOCK = int(re.search(r"constexpr int kAnomBlock = (\d+);", _DEVTYPES).group(1))
TILE = int(re.search(r"constexpr int kAggTile = (\d+);", _DEVTYPES).group(1))
SORT_TILE = int(re.search(r"constexpr int kSegSortTile = (\d+);", _DEVTYPES).group(1))
ALL_TIME = (-1, S.LONG_MAX)
FLUSH, IN, REPL, LATENCY, TINY = range(5)  # the metrics of these scripts; LATENCY ~ 20, TINY <= 1
M = 5
PROFILES = ("normal", "normal", "normal", "slow", "slow", "quiet", "lowflush", "lowbytes", "const", "gap", "nocurrent",
            "spike", "dip", "smallslow", "absent")
SEED = 0  # picked on the CPU so that the coverage asserted in test_shapes (one workgroup + 1) holds on the restatement


class Pair:
    """One device aggregator and the restatement, fed the same calls."""

    def __init__(self, lib, num_entities, num_windows, group=None):
        group = group if group is not None else [e // 2 for e in range(num_entities)]  # two brokers per host
        fns = [S.AVG, S.AVG, S.AVG, S.MAX, S.LATEST]
        self.dev = ccmi.MetricSampleAggregator(num_windows, S.WINDOW_MS, 1, fns, group, lib=lib)
        self.ref = S.MetricSampleAggregator(num_windows, S.WINDOW_MS, 1, fns, group)
        self.E = num_entities

    def add(self, batch):
        ents, times, vals = batch
        if not ents:
            return
        got = self.dev.add_samples(ents, times, vals)
        want = self.ref.add_samples(ents, times, vals)
        assert got.tolist() == [1 if a else 0 for a in want]

    def state(self):
        s = self.dev.state()
        return (s.generation, s.oldest_window_index, s.current_window_index, s.num_samples, s.num_present_entities)


def window_batch(rng, profiles, w, history_windows, slow=None):
    """One sample per entity in window w; w > history_windows is a current window. `slow` overrides the profiles'
    own choice of who is slow now (the rounds of a detect sequence)."""
    current = w > history_windows
    ents, times, vals = [], [], []
    for e, p in enumerate(profiles):
        gap = p == "gap" and w in (history_windows // 2, history_windows // 2 + 1)  # two in a row: no AVG_ADJACENT
        if p == "absent" or gap or (p == "nocurrent" and current):  # absent: never sampled, not in _rawMetrics
            continue
        flush = 100.0 + rng.randint(-25, 25)
        bytes_in, repl = 4096.0 + rng.randint(-400, 400), 4096.0 + rng.randint(-400, 400)
        latency, tiny = 20.0 + rng.randint(-100, 100) / 100.0, rng.random()
        if p == "const":  # equal histories: every order statistic is a tie
            flush, bytes_in, repl, latency = 100.0, 4096.0, 4096.0, 20.0
        if p == "quiet":
            bytes_in, repl = 300.0, 300.0 + rng.randint(0, 500)  # around the threshold of 1024 with the sum
        if p == "lowflush" and not current and w % 3:
            flush = float(rng.randint(0, 5))  # <= 5.0: filtered out of the flush history
        if p == "lowbytes" and not current and w % 4:
            bytes_in, repl = 100.0, 200.0  # below the threshold: filtered out of the per-byte history
        if p == "smallslow":
            flush = 10.0 + rng.randint(-2, 2)  # four times its history is still under the absolute threshold
        is_slow = (e in slow) if slow is not None else p in ("slow", "lowflush", "lowbytes", "smallslow")
        if current and is_slow:
            flush *= rng.choice([4, 5, 6])
        if current and p == "spike":
            latency = 40.0
        if current and p == "dip":
            latency = 2.0
        ents.append(e)
        times.append((w - 1) * S.WINDOW_MS + rng.randrange(S.WINDOW_MS))
        vals.append([flush, bytes_in, repl, latency, tiny])
    order = list(range(len(ents)))
    rng.shuffle(order)
    return [ents[i] for i in order], [times[i] for i in order], [vals[i] for i in order]


def build(lib, rng, num_entities, history_windows, num_windows=None, profiles=None):
    profiles = profiles or [rng.choice(PROFILES) for _ in range(num_entities)]
    p = Pair(lib, num_entities, num_windows or max(history_windows, 1))
    for w in range(1, history_windows + 2):
        p.add(window_batch(rng, profiles, w, history_windows))
    return p, profiles


def dbits(values):
    return [A.double_bits(v) for v in values]


def check_percentile(p, upper, lower, upper_margin, lower_margin, metrics, interested=None, capacity=None, options=None):
    """-> the restatement's anomalies."""
    mask = np.zeros(M, dtype=np.uint8)
    mask[list(metrics)] = 1
    history, current, failure, result = A.row_maps(p.ref, *ALL_TIME, options, interested)
    want = A.PercentileMetricAnomalyFinder(upper, lower, upper_margin, lower_margin, metrics).metric_anomalies(
        history, current)
    before = p.state()
    o = None if options is None else ccmi.AggregationOptions(
        options.min_valid_entity_ratio, options.min_valid_entity_group_ratio, options.min_valid_windows,
        options.max_allowed_extrapolations_per_entity, options.granularity, options.include_invalid_entities)
    got = p.dev.metric_anomalies(ALL_TIME[1], mask, upper, lower, upper_margin, lower_margin, options=o,
                                 interested=interested, capacity=capacity)
    assert p.state() == before
    assert got.completeness.failure == failure and got.current_window_index == p.ref.current
    if result is not None:
        assert got.completeness.valid_window_indices.tolist() == result.completeness.valid_window_indices
        assert got.completeness.num_valid_entities == len(result.entities)
    assert got.num_anomalies == len(want)
    k = len(want) if capacity is None else min(capacity, len(want))
    rec = got.records
    assert len(rec) == k
    assert list(zip(rec["entity"].tolist(), rec["metric"].tolist())) == [(a[0], a[1]) for a in want[:k]]
    for field, i in (("current", 2), ("upper_threshold", 3), ("lower_threshold", 4)):
        assert dbits(rec[field]) == dbits(a[i] for a in want[:k]), field
    return want


class Finders:
    """The device finder and the restatement's, configured alike."""

    def __init__(self, p, **config):
        self.p = p
        self.dev = ccmi.SlowBrokerFinder(p.dev, FLUSH, IN, REPL, **config)
        self.ref = A.SlowBrokerFinder(FLUSH, IN, REPL, **config)

    def check_scores(self):
        got = self.dev.scores()
        assert list(zip(got["entity"].tolist(), got["kind"].tolist(), got["score"].tolist(),
                        got["since_ms"].tolist())) == self.ref.scores()

    def detect(self, time_ms, interested=None, capacity=None):
        """-> the restatement's result."""
        p = self.p
        history, current, failure, _ = A.row_maps(p.ref, *ALL_TIME, None, interested)
        want = self.ref.metric_anomalies(history, current, time_ms)
        before = p.state()
        got = self.dev.detect(time_ms, to_ms=ALL_TIME[1], interested=interested, capacity=capacity, diagnostics=True)
        assert p.state() == before
        s = got.summary
        assert got.completeness.failure == failure and s.current_window_index == p.ref.current
        assert (s.num_current, s.num_skipped, s.num_active, s.cluster_size) == (
            want.num_current, len(want.skipped), want.num_active, want.cluster_size)
        assert dbits([s.peer_base_log_flush, s.peer_base_per_byte]) == dbits(want.peer_base)
        assert (s.num_persistent, s.num_recent, s.num_suspect) == (
            want.num_by_type["PERSISTENT"], want.num_by_type["RECENT"], want.num_by_type["SUSPECT"])
        assert (s.num_to_demote, s.num_to_remove) == (len(want.demote), len(want.remove))
        assert (s.unfixable, s.removal_enabled) == (int(want.unfixable), int(self.ref.removal_enabled))
        assert got.diagnostics.tolist() == [want.diag.get(e, 0) for e in range(p.E)]
        assert got.num_brokers == len(want.brokers)
        k = len(want.brokers) if capacity is None else min(capacity, len(want.brokers))
        b = got.brokers
        assert list(zip(b["entity"].tolist(), b["kind"].tolist(), b["score"].tolist(), b["since_ms"].tolist())) == \
            want.brokers[:k]
        self.check_scores()
        return want


FEATURES = dict(skipped=False, flush_history=False, flush_peers=False, per_byte_history=False, per_byte_peers=False,
                over=False, suspect=False, not_suspect_by_threshold=False, flush_history_cut=False,
                per_byte_history_cut=False, current_without_history=False, history_without_sample=False, absent=False,
                upper_anomaly=False, lower_anomaly=False, insignificant=False, ties=False)


def note_features(f, p, want_slow, want_pct, profiles):
    history, current, _, _ = A.row_maps(p.ref, *ALL_TIME)
    for e, d in want_slow.diag.items():
        f["skipped"] |= d == A.DIAG_SKIPPED
        f["flush_history"] |= bool(d & A.DIAG_FLUSH_HISTORY)
        f["flush_peers"] |= bool(d & A.DIAG_FLUSH_PEERS)
        f["per_byte_history"] |= bool(d & A.DIAG_PER_BYTE_HISTORY)
        f["per_byte_peers"] |= bool(d & A.DIAG_PER_BYTE_PEERS)
        f["over"] |= bool(d & A.DIAG_OVER_THRESHOLD)
        f["suspect"] |= bool(d & A.DIAG_SUSPECT)
        f["not_suspect_by_threshold"] |= bool(d & (A.DIAG_FLUSH_HISTORY | A.DIAG_FLUSH_PEERS)) and \
            bool(d & (A.DIAG_PER_BYTE_HISTORY | A.DIAG_PER_BYTE_PEERS)) and not d & A.DIAG_OVER_THRESHOLD
    for e, h in history.items():
        wv = len(h[FLUSH])
        if e in current and e not in want_slow.skipped and A.is_data_sufficient(wv, 90.0, 90.0):
            kept = sum(1 for v in h[FLUSH] if v > 5.0)
            f["flush_history_cut"] |= not A.is_data_sufficient(kept, 90.0, 90.0)
            kept = sum(1 for a, b in zip(h[IN], h[REPL]) if a + b >= 1024.0)
            f["per_byte_history_cut"] |= not A.is_data_sufficient(kept, 90.0, 90.0)
        f["ties"] |= len(set(h[FLUSH])) == 1 and wv > 1
        f["insignificant"] |= A.percentile([float(v) for v in h[TINY]], 90.0) <= 1.0
    f["current_without_history"] |= any(e not in history for e in current)
    f["history_without_sample"] |= any(profiles[e] == "nocurrent" for e in history)
    f["absent"] |= any(name == "absent" and e not in current and e not in history for e, name in enumerate(profiles))
    f["upper_anomaly"] |= any(a[2] > a[3] for a in want_pct)
    f["lower_anomaly"] |= any(a[2] < a[4] for a in want_pct)


# ---------------------------------------------------------------------------------------------- 1. shapes
SHAPES = [1, 2, 63, 64, 65, BLOCK + 1, 2 * TILE + 1]


@pytest.mark.parametrize("num_entities", SHAPES)
def test_shapes(gpu_lib, num_entities):
    """Ten history windows (the sufficiency edge of the 90th percentile) at every entity count at which a kernel takes
    another path: a lane, a wave and one more, a workgroup and one more, two compaction tiles and one more."""
    rng = random.Random(SEED * 1000 + num_entities)
    p, profiles = build(gpu_lib, rng, num_entities, 10)
    want_pct = check_percentile(p, 90.0, 10.0, 0.5, 0.2, range(M))
    check_percentile(p, 90.0, 10.0, 0.5, 0.2, [LATENCY])
    assert check_percentile(p, 90.0, 10.0, 0.5, 0.2, []) == []
    assert check_percentile(p, 95.0, 5.0, 0.5, 0.2, range(M)) == []  # ten windows are not enough for 95 / 5
    mask = np.array([1 if rng.random() < 0.6 else 0 for _ in range(num_entities)], dtype=np.uint8)
    mask[0] = 1
    mask[[e for e, name in enumerate(profiles) if name == "absent"]] = 1  # interested entities that are absent
    check_percentile(p, 90.0, 10.0, 0.0, 1.0, range(M), interested=mask)
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0)
    want = f.detect(1000)
    f.detect(2000, interested=mask)
    if num_entities == BLOCK + 1:  # asserted on the restatement alone: this script reaches what the comparison is for
        seen = dict(FEATURES)
        note_features(seen, p, want, want_pct, profiles)
        assert all(seen.values()), seen


# ---------------------------------------------------------------------------------------------- 2. history lengths
@pytest.mark.parametrize("history_windows", [0, 1, 9, 10, 11, 31])
def test_history_lengths(gpu_lib, history_windows):
    """No window at all (the failure path: the finders still run), one, the sufficiency edge at p = 90 and the most an
    aggregator keeps."""
    rng = random.Random(100 + history_windows)
    p, _ = build(gpu_lib, rng, 65, history_windows)
    history, _, failure, _ = A.row_maps(p.ref, *ALL_TIME)
    assert (failure != S.FAIL_NONE) == (history_windows == 0) == (not history)
    for upper, lower in ((90.0, 10.0), (95.0, 5.0), (75.0, 50.0), (99.99, 0.01)):
        want = check_percentile(p, upper, lower, 0.5, 0.2, range(M))
        assert bool(want) == A.is_data_sufficient(history_windows, upper, lower), (upper, lower)
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0)
    want = f.detect(500)
    assert want.cluster_size == len(history)
    assert any(d & A.DIAG_FLUSH_HISTORY for d in want.diag.values()) == (history_windows >= 10)
    assert any(d & A.DIAG_FLUSH_PEERS for d in want.diag.values())  # the peer step needs no history
    # percentiles of 0 and 100 are never sufficient: no history hit, no peer base
    g = Finders(p, log_flush_time_threshold_ms=150.0, metric_history_percentile=100.0, peer_metric_percentile=0.0)
    want = g.detect(600)
    assert all(np.isnan(b) for b in want.peer_base) and not want.suspects


def test_no_sample_at_all(gpu_lib):
    """An aggregator that never saw a sample: no history, no current row, and the finders still answer."""
    p = Pair(gpu_lib, 3, 5)
    assert check_percentile(p, 90.0, 10.0, 0.5, 0.2, range(M)) == []
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0)
    want = f.detect(5)
    assert (want.num_current, want.cluster_size, want.brokers) == (0, 0, [])


# ---------------------------------------------------------------------------------------------- 3. peers
@pytest.mark.parametrize("active", [0, 1, 2, 3, SORT_TILE + 1])
def test_active_peer_counts(gpu_lib, active):
    """The peer percentile over no, one, two and three active brokers (two is the sufficiency minimum at p = 50) and
    over one more than the sort's tile, among brokers with negligible traffic."""
    rng = random.Random(active)
    num_entities = active + 3
    profiles = ["normal"] * num_entities
    for e in rng.sample(range(num_entities), 3):
        profiles[e] = "quiet"
    if active >= 3:
        profiles[profiles.index("normal")] = "slow"
    p, _ = build(gpu_lib, rng, num_entities, 2, profiles=profiles)
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0, bytes_in_rate_detection_threshold=2000.0)
    want = f.detect(7)
    assert want.num_active == active and len(want.skipped) == 3
    assert all(np.isnan(b) for b in want.peer_base) == (active < 2)
    assert len(want.brokers) == (1 if active >= 3 else 0)
    # a threshold of zero: nobody is skipped, the quiet brokers join the peers
    g = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0, bytes_in_rate_detection_threshold=0.0)
    assert g.detect(8).num_active == num_entities


# ---------------------------------------------------------------------------------------------- 4. capacity
def test_capacity_convention(gpu_lib):
    rng = random.Random(9)
    p, _ = build(gpu_lib, rng, 65, 10)
    want = check_percentile(p, 90.0, 10.0, 0.5, 0.2, range(M))
    total = len(want)
    assert total >= 3
    for capacity in (0, 2, total):
        check_percentile(p, 90.0, 10.0, 0.5, 0.2, range(M), capacity=capacity)
    lib = p.dev.lib
    s, _arrays = p.dev._completeness_struct(np)
    o = ccmi.AggregationOptions(0.0, 0.0, 1, 5, ccmi.GRANULARITY_ENTITY, False).struct()
    cfg = ccmi.MetricAnomalyConfigStruct(90.0, 10.0, 0.5, 0.2)
    metrics = np.ones(M, dtype=np.uint8)
    n, window = C.c_int64(-1), C.c_int64(-1)
    # the sizing call
    lib.check(lib.lib.ccmi_aggregator_metric_anomalies(p.dev.handle, -1, S.LONG_MAX, C.byref(o), None, C.byref(cfg),
                                                       metrics.ctypes.data, C.byref(s), C.byref(window), None, 0,
                                                       C.byref(n)))
    assert n.value == total and window.value == p.ref.current
    for capacity in (2, total):
        rec = np.full((total + 1) * 32, 0xAB, dtype=np.uint8)
        lib.check(lib.lib.ccmi_aggregator_metric_anomalies(p.dev.handle, -1, S.LONG_MAX, C.byref(o), None,
                                                           C.byref(cfg), metrics.ctypes.data, C.byref(s),
                                                           C.byref(window), rec.ctypes.data, capacity, C.byref(n)))
        assert n.value == total and (rec[capacity * 32:] == 0xAB).all()  # rows beyond the count stay untouched
        assert rec[:capacity * 32].view(ccmi.METRIC_ANOMALY_DTYPE)["entity"].tolist() == [a[0] for a in want[:capacity]]
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0, self_healing_unfixable_ratio=1.0)
    first = f.detect(1)
    assert len(first.brokers) >= 3
    f.detect(2, capacity=0)  # still one round of the score update
    f.detect(3, capacity=2)
    last = f.detect(4, capacity=len(first.brokers))
    assert [b[2] for b in last.brokers] == [4] * len(last.brokers)
    got = f.dev.scores(capacity=1)
    assert len(got) == 1 and got["entity"][0] == f.ref.scores()[0][0]
    f.dev.reset()
    f.ref.score, f.ref.since = {}, {}
    f.check_scores()


# ---------------------------------------------------------------------------------------------- 5. rounds
def test_five_rounds(gpu_lib):
    """Five detection rounds, a new window each: scores rise to demotion and to the decommission clamp, fall, reach
    zero and leave, and a broker comes back with a new since; scores() is compared after every round."""
    rng = random.Random(21)
    num_entities, history_windows = 65, 10
    profiles = ["normal"] * num_entities
    profiles[7], profiles[40] = "quiet", "nocurrent"
    p = Pair(gpu_lib, num_entities, history_windows + 6)
    for w in range(1, history_windows + 1):
        p.add(window_batch(rng, profiles, w, history_windows, slow=set()))
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=2, decommission_score=3,
                self_healing_unfixable_ratio=0.03, removal_enabled=True)
    slow_by_round = [{1, 2, 3, 64}, {1, 2, 64}, {1, 64, 40}, {1, 3}, {3}]
    seen = dict(demote=False, remove=False, clamp=False, left=False, back=False, unfixable=False, fixable=False)
    gone = set()
    for r, slow in enumerate(slow_by_round):
        w = history_windows + 1 + r
        p.add(window_batch(rng, profiles, w, w - 1, slow=slow))
        before = dict(f.ref.score)
        want = f.detect(1000 * (r + 1))
        assert want.suspects == slow - {40}, r  # 40 has no sample in a current window: negligible traffic
        seen["demote"] |= bool(want.demote)
        seen["remove"] |= bool(want.remove)
        seen["clamp"] |= any(before.get(e) == 3 and f.ref.score.get(e) == 3 for e in slow)
        left = set(before) - set(f.ref.score)
        seen["left"] |= bool(left)
        seen["back"] |= bool(gone & set(f.ref.score))
        gone |= left
        seen["unfixable"] |= want.unfixable
        seen["fixable"] |= bool(want.brokers) and not want.unfixable
    assert all(seen.values()), seen


# ---------------------------------------------------------------------------------------------- 6. errors
def test_invalid_arguments_change_nothing(gpu_lib):
    rng = random.Random(3)
    p, _ = build(gpu_lib, rng, 4, 10, profiles=["slow", "normal", "normal", "normal"])
    f = Finders(p, log_flush_time_threshold_ms=150.0, demotion_score=0)
    f.detect(10)
    before, scores = p.state(), f.ref.scores()
    assert scores
    ones = np.ones(M, dtype=np.uint8)
    for kwargs in (dict(upper_percentile=0.0), dict(upper_percentile=100.0), dict(lower_percentile=0.001),
                   dict(lower_percentile=99.995), dict(upper_percentile=float("nan")), dict(upper_margin=-0.1),
                   dict(upper_margin=10.5), dict(lower_margin=-0.1), dict(lower_margin=1.5), dict(capacity=-1),
                   dict(options=ccmi.AggregationOptions(min_valid_windows=0))):
        with pytest.raises(ccmi.IllegalArgumentException):
            p.dev.metric_anomalies(S.LONG_MAX, ones, **kwargs)
    with pytest.raises(ccmi.IllegalArgumentException):
        p.dev.metric_anomalies(S.LONG_MAX, np.ones(M + 1, dtype=np.uint8))
    for kwargs in (dict(bytes_in_rate_detection_threshold=-1.0), dict(log_flush_time_threshold_ms=-0.5),
                   dict(metric_history_percentile=-1.0), dict(metric_history_percentile=100.5),
                   dict(metric_history_margin=0.99), dict(peer_metric_percentile=-0.1),
                   dict(peer_metric_percentile=101.0), dict(peer_metric_margin=0.5), dict(demotion_score=-1),
                   dict(decommission_score=-1), dict(self_healing_unfixable_ratio=-0.1),
                   dict(self_healing_unfixable_ratio=1.1), dict(peer_metric_margin=float("nan"))):
        with pytest.raises(ccmi.IllegalArgumentException):
            ccmi.SlowBrokerFinder(p.dev, FLUSH, IN, REPL, **kwargs)
    for metrics in ((-1, IN, REPL), (FLUSH, M, REPL), (FLUSH, IN, M + 3)):
        with pytest.raises(ccmi.IllegalArgumentException):
            ccmi.SlowBrokerFinder(p.dev, *metrics)
    with pytest.raises(ccmi.IllegalArgumentException):
        f.dev.detect(20, capacity=-1)
    with pytest.raises(ccmi.IllegalArgumentException):
        f.dev.detect(20, options=ccmi.AggregationOptions(min_valid_windows=0))
    with pytest.raises(ccmi.IllegalArgumentException):
        f.dev.scores(capacity=-1)
    lib = p.dev.lib
    with pytest.raises(ccmi.IllegalArgumentException):  # capacity without an array
        s, _arrays = p.dev._completeness_struct(np)
        o = ccmi.AggregationOptions().struct()
        summary, n = ccmi.SlowBrokerSummaryStruct(), C.c_int64(0)
        lib.check(lib.lib.ccmi_slow_broker_finder_detect(f.dev.handle, -1, S.LONG_MAX, C.byref(o), None, 20,
                                                         C.byref(s), C.byref(summary), None, 4, C.byref(n), None))
    assert p.state() == before and f.ref.scores() == scores
    f.check_scores()
    # the percentiles 0 and 100 are legal for the slow broker finder (never sufficient), and the calls still work
    ccmi.SlowBrokerFinder(p.dev, FLUSH, IN, REPL, metric_history_percentile=0.0, peer_metric_percentile=100.0)
    f.detect(30)
