"""Pins tests/metric_anomaly_support.py, the restatement the device finders are compared against: hand-derived
percentile cases, the reference's own unit-test scenarios (SlowBrokerFinderTest, KafkaMetricAnomalyFinderTest, rebuilt
as AnomalyDetectorTestUtils builds them) and multi-round score scripts. CPU only."""
import math
import random

import pytest

import metric_anomaly_support as A

NAN = float("nan")


# ---------------------------------------------------------------------------------------------- the percentile
def test_percentile_by_hand():
    ten = [float(v) for v in range(10, 0, -1)]
    # pos = 0.9 * 11 = 9.9: 9 + 0.9 * (10 - 9), in the doubles the rule produces
    pos = (90 / 100.0) * 11
    assert A.percentile(ten, 90) == 9.0 + (pos - 9.0) * 1.0 and abs(A.percentile(ten, 90) - 9.9) < 1e-12
    assert A.percentile(ten, 95) == 10.0  # pos = 10.45 >= n
    assert A.percentile(ten, 5) == 1.0  # pos = 0.55 < 1
    assert A.percentile([4.0, 1.0, 3.0, 2.0], 50) == 2.5  # pos = 2.5
    assert math.isnan(A.percentile([], 50))
    assert A.percentile([7.0], 1) == 7.0 and math.isnan(A.percentile([NAN], 50))  # n == 1: the value, a NaN too
    assert A.percentile([NAN, 3.0, NAN, 1.0], 50) == 2.0  # NaNs removed: pos = 1.5 over {1, 3}
    assert math.isnan(A.percentile([NAN, NAN], 50))
    assert A.percentile(ten, 100) == 10.0 and A.percentile([2.0, 1.0], 100) == 2.0  # pos is exactly n
    assert A.percentile([5.0, 5.0, 5.0], 50) == 5.0  # ties
    assert A.percentile([1.0, math.inf], 50) == math.inf


def test_sufficiency_minima():
    assert [A.min_num_values(p) for p in (90, 95, 50, 2)] == [10, 20, 2, 50]
    assert A.min_num_values(0) == A.INT_MAX == A.min_num_values(100)  # Java's (int) of +Infinity
    assert A.min_num_values(99.99) == 10000 and A.min_num_values(0.01) == 10000
    assert A.is_data_sufficient(10, 90, 90) and not A.is_data_sufficient(9, 90, 90)
    assert A.is_data_sufficient(20, 95, 5) and not A.is_data_sufficient(19, 95, 5)
    assert A.is_data_sufficient(20, 95, 50) and not A.is_data_sufficient(19, 50, 95)
    assert not A.is_data_sufficient(A.INT_MAX - 1, 0, 50) and not A.is_data_sufficient(10 ** 6, 50, 100)


# ---------------------------------------------------------------------------------------------- the reference's tests
FLUSH, IN, REPL = 0, 1, 2  # the metric ids of these scenarios
NORMAL_BYTES, BYTES_VARIANCE, NORMAL_FLUSH, FLUSH_VARIANCE, SMALL_BYTES = 4096.0, 0.1, 100.0, 0.25, 1024.0
WINDOWS, MULTIPLIER, TIME_MS = 10, 4, 100
SEEDS = range(6)


def values(bytes_in, repl_in, flush):
    return [flush, bytes_in, repl_in]


def slow_finder():  # createSlowBrokerFinder: demotion score 0, log flush threshold 150, the other defaults
    return A.SlowBrokerFinder(FLUSH, IN, REPL, demotion_score=0, log_flush_time_threshold_ms=150.0)


def history_of(rng, base, windows=WINDOWS, scale=1.0):
    return A.test_utils_history(rng, base, values(base[IN] * BYTES_VARIANCE, base[REPL] * BYTES_VARIANCE,
                                                  NORMAL_FLUSH * scale * FLUSH_VARIANCE), windows)


def no_anomaly(finder, r):
    assert r.anomalies == [] and r.brokers == []
    assert finder.num_by_type == dict(PERSISTENT=0, RECENT=0, SUSPECT=0)


def one_recent(finder, r):
    assert len(r.anomalies) == 1 and set(r.anomalies[0][0]) == {0} and r.anomalies[0][0][0] == TIME_MS
    assert finder.num_by_type == dict(PERSISTENT=0, RECENT=1, SUSPECT=0)
    assert r.brokers == [(0, A.DEMOTE, 1, TIME_MS)]


@pytest.mark.parametrize("seed", SEEDS)
def test_detecting_slow_broker_from_history(seed):
    rng = random.Random(seed)
    finder = slow_finder()
    history = {0: history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))}
    current = {0: A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH * MULTIPLIER))}
    r = finder.metric_anomalies(history, current, TIME_MS)
    one_recent(finder, r)
    assert r.diag[0] & A.DIAG_FLUSH_HISTORY and not r.diag[0] & A.DIAG_FLUSH_PEERS  # one broker has no peers


@pytest.mark.parametrize("seed", SEEDS)
def test_detecting_slow_broker_from_peer(seed):
    rng = random.Random(seed)
    finder = slow_finder()
    history = {0: history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH * MULTIPLIER))}
    current = {0: A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH * MULTIPLIER))}
    for i in range(1, 4):
        history[i] = history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))
        current[i] = A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))
    r = finder.metric_anomalies(history, current, TIME_MS)
    one_recent(finder, r)
    assert r.diag[0] & A.DIAG_FLUSH_PEERS and r.diag[0] & A.DIAG_PER_BYTE_PEERS
    assert r.peer_base[0] == 100.0 and r.unfixable  # 1 > 4 * 0.1: still one anomaly, reported as not fixable


@pytest.mark.parametrize("seed", SEEDS)
def test_excluding_small_traffic_broker(seed):
    rng = random.Random(seed)
    finder = slow_finder()
    # SMALL_BYTES_IN_RATE on both metrics sums to 2048 >= 1024: the broker is not skipped, it is simply normal
    history = {0: history_of(rng, values(SMALL_BYTES, SMALL_BYTES, NORMAL_FLUSH))}
    current = {0: A.test_utils_current(values(SMALL_BYTES, SMALL_BYTES, NORMAL_FLUSH))}
    for i in range(1, 4):
        # the reference puts every one of these histories under broker 0 (its test's own slip): later ones replace it
        history[0] = history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))
        current[i] = A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))
    no_anomaly(finder, finder.metric_anomalies(history, current, TIME_MS))


@pytest.mark.parametrize("seed", SEEDS)
def test_insufficient_data(seed):
    rng = random.Random(seed)
    finder = slow_finder()
    history = {0: history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH), WINDOWS // 2)}
    current = {0: A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH * MULTIPLIER))}
    r = finder.metric_anomalies(history, current, TIME_MS)
    no_anomaly(finder, r)
    assert r.diag[0] == A.DIAG_OVER_THRESHOLD


@pytest.mark.parametrize("seed", SEEDS)
def test_no_false_positive_due_to_traffic_fluctuation(seed):
    rng = random.Random(seed)
    finder = slow_finder()
    history = {0: history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))}
    current = {0: A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, NORMAL_FLUSH))}
    no_anomaly(finder, finder.metric_anomalies(history, current, TIME_MS))


@pytest.mark.parametrize("seed", SEEDS)
def test_no_false_positive_on_small_log_flush_time(seed):
    rng = random.Random(seed)
    finder = slow_finder()
    small = NORMAL_FLUSH / 10
    history = {0: history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, small * MULTIPLIER), scale=0.1)}
    current = {0: A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, small * MULTIPLIER))}
    for i in range(1, 4):
        history[i] = history_of(rng, values(NORMAL_BYTES, NORMAL_BYTES, small), scale=0.1)
        current[i] = A.test_utils_current(values(NORMAL_BYTES, NORMAL_BYTES, small))
    r = finder.metric_anomalies(history, current, TIME_MS)
    no_anomaly(finder, r)
    assert r.diag[0] & A.DIAG_FLUSH_PEERS and not r.diag[0] & A.DIAG_OVER_THRESHOLD  # 40 ms: above its peers, not slow


def percentile_finder():  # createKafkaMetricAnomalyFinder: 95 / 5 / 0.5 / 0.2
    return A.PercentileMetricAnomalyFinder(95.0, 5.0, 0.5, 0.2, {0})


@pytest.mark.parametrize("seed", SEEDS)
def test_kafka_metric_anomalies(seed):
    rng = random.Random(seed)
    finder = percentile_finder()
    history = {0: A.test_utils_history(rng, [20.0], [1.0], 20)}
    got = finder.metric_anomalies(history, {0: [40.0]})
    assert len(got) == 1 and finder.num_recent == 1
    entity, metric, cur, upper, lower = got[0]
    assert (entity, metric, cur) == (0, 0, 40.0) and 19.0 * 1.5 <= upper <= 21.0 * 1.5 < cur and lower <= 21.0 * 0.2


@pytest.mark.parametrize("seed", SEEDS)
def test_kafka_metric_insufficient_data(seed):
    rng = random.Random(seed)
    finder = percentile_finder()
    history = {0: A.test_utils_history(rng, [20.0], [1.0], 19)}
    assert finder.metric_anomalies(history, {0: [20.0]}) == [] and finder.num_recent == 0
    # and with enough windows the value is inside the range
    history = {0: A.test_utils_history(rng, [20.0], [1.0], 20)}
    assert finder.metric_anomalies(history, {0: [20.0]}) == []
    # no history at all, an entity without history, a metric that is not interested, an insignificant value
    assert finder.metric_anomalies({}, {0: [40.0]}) == []
    assert finder.metric_anomalies(history, {1: [40.0]}) == []
    assert A.PercentileMetricAnomalyFinder(95.0, 5.0, 0.5, 0.2, set()).metric_anomalies(history, {0: [40.0]}) == []
    assert finder.metric_anomalies({0: [[1.0] * 20]}, {0: [40.0]}) == []  # u <= 1
    low = finder.metric_anomalies(history, {0: [2.0]})  # below lower * 0.2
    assert len(low) == 1 and low[0][2] < low[0][4]


# ---------------------------------------------------------------------------------------------- score scripts
def steady_history(n, flush=100.0):
    return [[flush] * n, [4096.0] * n, [4096.0] * n]


def round_of(finder, slow, time_ms, brokers=4, history=True):
    hist = {e: steady_history(10) for e in range(brokers)} if history else {}
    cur = {e: [400.0 if e in slow else 100.0, 4096.0, 4096.0] for e in range(brokers)}
    return finder.metric_anomalies(hist, cur, time_ms)


def test_score_rises_to_demotion_and_clamps_at_decommission():
    f = A.SlowBrokerFinder(FLUSH, IN, REPL, log_flush_time_threshold_ms=150.0, demotion_score=3, decommission_score=5,
                           self_healing_unfixable_ratio=1.0)
    seen = []
    for t in range(1, 9):
        r = round_of(f, {0}, 1000 * t)
        seen.append((f.scores(), r.brokers, dict(f.num_by_type)))
    assert [s[0] for s in seen] == [[(0, 0, min(t, 5), 1000)] for t in range(1, 9)]  # since stays, the score clamps
    assert [s[1] for s in seen[:2]] == [[], []] and seen[0][2] == dict(PERSISTENT=0, RECENT=0, SUSPECT=1)
    assert seen[2][1] == [(0, A.DEMOTE, 3, 1000)] and seen[3][1] == [(0, A.DEMOTE, 4, 1000)]
    assert all(s[1] == [(0, A.REMOVE, 5, 1000)] for s in seen[4:])
    assert seen[7][2] == dict(PERSISTENT=1, RECENT=0, SUSPECT=0)
    assert r.anomalies == [({0: 1000}, False, True)]  # removal is not enabled: reported, not fixable


def test_recovery_to_zero_leaves_both_maps():
    f = A.SlowBrokerFinder(FLUSH, IN, REPL, log_flush_time_threshold_ms=150.0, demotion_score=2, decommission_score=5,
                           self_healing_unfixable_ratio=1.0)
    round_of(f, {1, 2}, 10)
    round_of(f, {1}, 20)
    assert f.scores() == [(1, 0, 2, 10)] and 2 not in f.since  # 2 went 1 -> 0 and left
    r = round_of(f, set(), 30)
    assert f.scores() == [(1, 0, 1, 10)] and r.brokers == [] and f.num_by_type["SUSPECT"] == 1
    round_of(f, set(), 40)
    assert f.scores() == [] and f.since == {} and f.num_by_type == dict(PERSISTENT=0, RECENT=0, SUSPECT=0)
    r = round_of(f, {1}, 50)  # a new since
    assert f.scores() == [(1, 0, 1, 50)]
    # an entity that is no longer current still recovers
    f.metric_anomalies({}, {}, 60)
    assert f.scores() == []


def test_unfixable_crossing():
    f = A.SlowBrokerFinder(FLUSH, IN, REPL, log_flush_time_threshold_ms=150.0, demotion_score=1, decommission_score=9,
                           self_healing_unfixable_ratio=0.25, removal_enabled=True)
    r = round_of(f, {0}, 1, brokers=8)  # 1 > 8 * 0.25 is false
    assert not r.unfixable and r.anomalies == [({0: 1}, True, False)]
    r = round_of(f, {0, 1}, 2, brokers=8)  # 2 > 2.0 is false
    assert not r.unfixable and r.cluster_size == 8
    r = round_of(f, {0, 1, 2}, 3, brokers=8)  # 3 > 2.0
    assert r.unfixable and r.anomalies == [({0: 1, 1: 2, 2: 3}, False, False)]
    assert [b[:2] for b in r.brokers] == [(0, A.DEMOTE), (1, A.DEMOTE), (2, A.DEMOTE)]


def test_empty_history_with_a_peer_hit():
    f = A.SlowBrokerFinder(FLUSH, IN, REPL, log_flush_time_threshold_ms=150.0, demotion_score=0)
    r = round_of(f, {3}, 7, history=False)
    assert r.cluster_size == 0 and r.brokers == [(3, A.DEMOTE, 1, 7)]
    assert r.unfixable  # 1 > 0 * 0.1
    assert r.diag[3] == A.DIAG_FLUSH_PEERS | A.DIAG_PER_BYTE_PEERS | A.DIAG_OVER_THRESHOLD | A.DIAG_SUSPECT
    assert r.peer_base == [100.0, 100.0 / 8192.0]


def test_skipped_brokers_and_filters():
    f = A.SlowBrokerFinder(FLUSH, IN, REPL, log_flush_time_threshold_ms=150.0, demotion_score=0)
    hist = {0: [[400.0] * 10, [100.0] * 10, [100.0] * 10],  # history bytes below the threshold: per-byte history empty
            1: [[4.0] * 10, [4096.0] * 10, [4096.0] * 10]}  # history flush <= 5: flush history empty
    cur = {0: [400.0, 4096.0, 4096.0], 1: [400.0, 4096.0, 4096.0], 2: [400.0, 500.0, 500.0]}
    r = f.metric_anomalies(hist, cur, 5)
    assert r.skipped == {2} and r.num_active == 2 and r.diag[2] == A.DIAG_SKIPPED
    assert r.diag[0] == A.DIAG_OVER_THRESHOLD and r.diag[1] == A.DIAG_PER_BYTE_HISTORY | A.DIAG_OVER_THRESHOLD
    assert r.brokers == []
