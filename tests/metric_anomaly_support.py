"""A plain-Python restatement of the reference's two metric anomaly finders, the yardstick of
ccmi_aggregator_metric_anomalies and ccmi_slow_broker_finder.

Written from cruise-control-core detector/metricanomaly/{PercentileMetricAnomalyFinder, PercentileMetricAnomalyFinderUtils}
.java and cruise-control detector/SlowBrokerFinder.java, method by method, and from the rule of commons-math3 3.6.1's
stat.descriptive.rank.Percentile with its defaults (LEGACY estimation, NaNStrategy.REMOVED). It is not derived from the
HIP code. The finders work over two maps as MetricAnomalyDetector.run hands them over: history {entity: values[m][i]},
newest window first, and current {entity: values[m]}, both holding float32 values as Python floats (row_maps builds
them from the aggregator restatement of metric_aggregator_support). A Java double is a Python float; MetricValues
.latest() returns a Java float, so latest() + latest() is a float sum (f32), while doubleArray() widens first.
"""
import math
import random
import struct

import numpy as np

import metric_aggregator_support as S

INT_MAX = 2 ** 31 - 1
SIGNIFICANT_METRIC_VALUE_THRESHOLD = 1.0
DEMOTE, REMOVE = 1, 2
(DIAG_SKIPPED, DIAG_FLUSH_HISTORY, DIAG_FLUSH_PEERS, DIAG_PER_BYTE_HISTORY, DIAG_PER_BYTE_PEERS, DIAG_OVER_THRESHOLD,
 DIAG_SUSPECT) = 1, 2, 4, 8, 16, 32, 64
NAN = float("nan")


def double_bits(v):
    """The bit pattern of a double with every NaN canonical and -0.0 as 0.0 (the order statistics of Percentile are
    selected with <, so the sign of a zero is not determined)."""
    v = float(v)
    if v != v:
        return 0x7FF8000000000000
    if v == 0.0:
        return 0
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def jdiv(a, b):
    """Java's double a / b."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def percentile(values, p):
    """Percentile.evaluate(p) over the doubles `values`, p in (0, 100]."""
    n = len(values)
    if n == 0:
        return NAN
    if n == 1:
        return values[0]
    work = sorted(v for v in values if v == v)  # NaNStrategy.REMOVED
    n = len(work)
    if n == 0:
        return NAN
    q = p / 100.0
    pos = float(n) if q == 1.0 else q * (n + 1)
    if pos < 1:
        return work[0]
    if pos >= n:
        return work[n - 1]
    fpos = math.floor(pos)
    k, d = int(fpos), pos - fpos
    lower, upper = work[k - 1], work[k]
    return lower + d * (upper - lower)


def min_num_values(p):
    """(int) Math.ceil(100 / (p > 50.0 ? 100 - p : p))"""
    q = jdiv(100.0, (100.0 - p) if p > 50.0 else p)
    if q != q:
        return 0
    if q >= INT_MAX:
        return INT_MAX
    if q <= -INT_MAX - 1:
        return -INT_MAX - 1
    return int(math.ceil(q))


def is_data_sufficient(sample_count, upper_percentile, lower_percentile):
    return sample_count >= max(min_num_values(upper_percentile), min_num_values(lower_percentile))


class PercentileMetricAnomalyFinder:
    def __init__(self, upper_percentile, lower_percentile, upper_margin, lower_margin, interested_metrics):
        self.upper, self.lower = float(upper_percentile), float(lower_percentile)
        self.upper_margin, self.lower_margin = float(upper_margin), float(lower_margin)
        self.interested = set(interested_metrics)  # metric ids
        self.num_recent = 0

    def _anomaly_for_metric(self, entity, m, history, current):
        data = [float(v) for v in history[m]]  # doubleArray()
        u = percentile(data, self.upper)
        if u <= SIGNIFICANT_METRIC_VALUE_THRESHOLD:
            return None
        upper_threshold = u * (1 + self.upper_margin)
        lower_threshold = percentile(data, self.lower) * self.lower_margin
        cur = float(current[m])
        if cur > upper_threshold or cur < lower_threshold:
            return (entity, m, cur, upper_threshold, lower_threshold)
        return None

    def metric_anomalies(self, history, current):
        """-> [(entity, metric, current, upper_threshold, lower_threshold)] in ascending (entity, metric) order."""
        if not history or not is_data_sufficient(len(next(iter(history.values()))[0]), self.upper, self.lower):
            return []
        out = []
        for entity in sorted(current):
            h = history.get(entity)
            if h is None:
                continue
            for m in range(len(current[entity])):
                if m in self.interested:
                    a = self._anomaly_for_metric(entity, m, h, current[entity])
                    if a is not None:
                        out.append(a)
        self.num_recent = len(out)
        return out


class SlowBrokerResult:
    pass


class SlowBrokerFinder:
    def __init__(self, log_flush_metric, leader_bytes_in_metric, replication_bytes_in_metric,
                 bytes_in_rate_detection_threshold=1024.0, log_flush_time_threshold_ms=1000.0,
                 metric_history_percentile=90.0, metric_history_margin=3.0, peer_metric_percentile=50.0,
                 peer_metric_margin=3.0, demotion_score=5, decommission_score=50, self_healing_unfixable_ratio=0.1,
                 removal_enabled=False):
        self.m_flush, self.m_in, self.m_repl = log_flush_metric, leader_bytes_in_metric, replication_bytes_in_metric
        self.bytes_threshold = float(bytes_in_rate_detection_threshold)
        self.flush_threshold = float(log_flush_time_threshold_ms)
        self.history_percentile, self.history_margin = float(metric_history_percentile), float(metric_history_margin)
        self.peer_percentile, self.peer_margin = float(peer_metric_percentile), float(peer_metric_margin)
        self.demotion_score, self.decommission_score = int(demotion_score), int(decommission_score)
        self.unfixable_ratio = float(self_healing_unfixable_ratio)
        self.removal_enabled = bool(removal_enabled)
        self.score = {}  # _brokerSlownessScore
        self.since = {}  # _detectedSlowBrokers
        self.num_by_type = dict(PERSISTENT=0, RECENT=0, SUSPECT=0)

    # ---- detectMetricAnomalies
    def _from_history(self, historical, current, detected):
        for e, cur in current.items():
            h = historical.get(e)
            if h is not None and is_data_sufficient(len(h), self.history_percentile, self.history_percentile):
                if cur > percentile(h, self.history_percentile) * self.history_margin:
                    detected.add(e)

    def _from_peers(self, current, detected):
        if is_data_sufficient(len(current), self.peer_percentile, self.peer_percentile):
            base = percentile(list(current.values()), self.peer_percentile)
            for e, cur in current.items():
                if cur > base * self.peer_margin:
                    detected.add(e)
            return base
        return NAN

    def metric_anomalies(self, history, current, time_ms):
        r = SlowBrokerResult()
        hist_flush, cur_flush, hist_per_byte, cur_per_byte = {}, {}, {}, {}
        r.skipped = set()
        for e in sorted(current):
            cv = current[e]
            latest_bytes = S.f32(cv[self.m_in] + cv[self.m_repl])  # float latest() + float latest()
            if latest_bytes < self.bytes_threshold:
                r.skipped.add(e)
                continue
            flush = float(cv[self.m_flush])
            cur_flush[e] = flush
            cur_per_byte[e] = jdiv(flush, latest_bytes)
            h = history.get(e)
            if h is not None:
                hist_flush[e] = [float(v) for v in h[self.m_flush] if float(v) > 5.0]
                kept = []
                for i in range(len(h[self.m_in])):
                    total = float(h[self.m_in][i]) + float(h[self.m_repl][i])
                    if total >= self.bytes_threshold:
                        kept.append(jdiv(float(h[self.m_flush][i]), total))
                hist_per_byte[e] = kept
        sets = []
        r.peer_base = []
        for historical, cur in ((hist_flush, cur_flush), (hist_per_byte, cur_per_byte)):
            from_history, from_peers = set(), set()
            self._from_history(historical, cur, from_history)
            r.peer_base.append(self._from_peers(cur, from_peers))
            sets.append((from_history, from_peers))
        over = set(e for e, v in cur_flush.items() if v > self.flush_threshold)
        suspects = (sets[0][0] | sets[0][1]) & (sets[1][0] | sets[1][1]) & over
        r.num_current, r.num_active = len(current), len(cur_flush)
        r.diag = {}
        for e in current:
            if e in r.skipped:
                r.diag[e] = DIAG_SKIPPED
                continue
            r.diag[e] = ((DIAG_FLUSH_HISTORY if e in sets[0][0] else 0) | (DIAG_FLUSH_PEERS if e in sets[0][1] else 0) |
                         (DIAG_PER_BYTE_HISTORY if e in sets[1][0] else 0) |
                         (DIAG_PER_BYTE_PEERS if e in sets[1][1] else 0) | (DIAG_OVER_THRESHOLD if e in over else 0) |
                         (DIAG_SUSPECT if e in suspects else 0))
        r.suspects = suspects
        # ---- updateBrokerSlownessScore
        for e in suspects:
            self.since.setdefault(e, time_ms)
            v = self.score.get(e)
            self.score[e] = 1 if v is None else min(v + 1, self.decommission_score)
        recovered = set()
        for e in list(self.score):
            if e not in suspects:
                score = self.score[e] - 1
                if score == 0:
                    recovered.add(e)
                else:
                    self.score[e] = score
        for e in recovered:
            del self.score[e]
            del self.since[e]
        # ---- createSlowBrokerAnomalies
        cluster_size = len(history)
        demote, remove = {}, {}
        for e in suspects:
            score = self.score[e]
            if score == self.decommission_score:
                remove[e] = self.since[e]
            elif score >= self.demotion_score:
                demote[e] = self.since[e]
        both = len(demote) + len(remove)
        self.num_by_type = dict(PERSISTENT=len(remove), RECENT=len(demote), SUSPECT=len(self.since) - both)
        r.cluster_size, r.demote, r.remove = cluster_size, demote, remove
        r.unfixable = both > cluster_size * self.unfixable_ratio
        r.num_by_type = dict(self.num_by_type)
        # the reference's anomalies: (brokers, fixable, remove)
        r.anomalies = []
        if r.unfixable:
            merged = dict(demote)
            merged.update(remove)
            r.anomalies.append((merged, False, False))
        else:
            if demote:
                r.anomalies.append((demote, True, False))
            if remove:
                r.anomalies.append((remove, self.removal_enabled, True))
        r.brokers = sorted([(e, DEMOTE, self.score[e], t) for e, t in demote.items()] +
                           [(e, REMOVE, self.score[e], t) for e, t in remove.items()])
        return r

    def scores(self):
        return sorted((e, 0, s, self.since[e]) for e, s in self.score.items())


BROKER_OPTIONS = dict(min_valid_entity_ratio=0.0, min_valid_entity_group_ratio=0.0, min_valid_windows=1,
                      max_allowed_extrapolations_per_entity=5, granularity=S.ENTITY, include_invalid_entities=False)


def broker_options():
    """KafkaBrokerMetricSampleAggregator.aggregate's AggregationOptions."""
    return S.AggregationOptions(**BROKER_OPTIONS)


def row_maps(ref, frm, to, options=None, interested=None):
    """loadMonitor().brokerMetrics().valuesAndExtrapolations() and currentBrokerMetricValues() over the aggregator
    restatement `ref`: -> (history map, current map, failure code, the AggregationResult or None)."""
    options = options or broker_options()
    ids = None if interested is None else [e for e, f in enumerate(interested) if f]
    history, failure, result = {}, S.FAIL_NONE, None
    try:
        result = ref.aggregate(frm, to, options, ids)
        for row, e in enumerate(result.entities.tolist()):
            history[e] = [[float(v) for v in result.values[row][m]] for m in range(len(ref.fn))]
    except S.NotEnoughValidWindowsException as ex:  # the reference returns an empty map
        failure = ex.failure
    ents, values, _ = ref.peek_current_window()
    current = {e: [float(v) for v in values[row]] for row, e in enumerate(ents.tolist())}
    return history, current, failure, result


# ------------------------------------------------------------------------------------------------ the reference's tests
def test_utils_history(rng, value_by_metric, fluctuation_by_metric, num_windows):
    """AnomalyDetectorTestUtils.createHistory for one broker: value + (randint(0, 200) - 100) * fluctuation / 100 per
    window, stored as floats."""
    return [[S.f32(value_by_metric[m] + (rng.randint(0, 200) - 100) * fluctuation_by_metric[m] / 100)
             for _ in range(num_windows)] for m in range(len(value_by_metric))]


def test_utils_current(value_by_metric):
    return [S.f32(v) for v in value_by_metric]


test_utils_history.__test__ = False
test_utils_current.__test__ = False
