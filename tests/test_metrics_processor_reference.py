"""Pins the plain-Python restatement of CruiseControlMetricsProcessor (tests/metrics_processor_support.py), the reference
of the K20 GPU tests: the scenarios of CruiseControlMetricsProcessorTest fed in several shuffled arrival orders,
hand-derived cases, the HashMap model against jsem.h's JHashSet (tests/cpp/hashset_order.cpp), and the known answers of
tests/golden/metrics_processor_kat.json. CPU only."""
import json
import os
import random
import struct

import pytest

import metrics_processor_support as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(REPO, "tests", "golden", "metrics_processor_kat.json")))
DELTA = 0.001
W = (0.7, 0.15, 0.15)


def hx(d):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(d)))[0]


def unhx(h):
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def process(records, partitions=S.BASIC_PARTITIONS, nodes=S.BASIC_NODES, cores=(32.0, 32.0), seed=None, **kw):
    records = list(records)
    if seed is not None:
        random.Random(seed).shuffle(records)
    p = S.Processor()
    p.add(records)
    return p, p.process(partitions, list(nodes), list(cores), **kw)


@pytest.mark.parametrize("seed", [None, 0, 1, 2, 3])
def test_basic(seed):
    p, o = process(S.basic_records(), seed=seed)
    assert p.cached_cores == {0: 32.0, 1: 32.0}
    assert o["num_partition_samples"] == 4 and o["num_broker_samples"] == 2 and o["max_metric_timestamp"] == 102
    b0 = lambda p_in, p_out: 32.0 * S.estimate_cpu_per_core(W, 50.0, 820.0, 1380.0 + 20.0 + 800.0, 500.0, p_in, p_out)
    expected = [(b0(20.0, 80.0 + 20.0), 20.0, 80.0, 100.0),
                (32.0 * S.estimate_cpu_per_core(W, 30.0, 500.0, 500.0 + 500.0, 20.0 + 800.0, 500.0, 500.0 + 500.0),
                 500.0, 500.0, 300.0),
                (b0(800.0 / 2, (1300.0 + 800.0) / 2), 400.0, 650.0, 200.0),
                (b0(800.0 / 2, (1300.0 + 800.0) / 2), 400.0, 650.0, 500.0)]
    for row, (cpu, bytes_in, bytes_out, disk) in zip(o["partition_values"], expected):
        assert abs(row[0] - cpu) < DELTA and abs(row[2] - bytes_in) < DELTA
        assert abs(row[3] - bytes_out) < DELTA and abs(row[1] - disk) < DELTA
    assert [row[0] for row in o["broker_values"]] == [50.0, 30.0]
    assert abs(o["broker_values"][0][7] - 500.0) < DELTA and abs(o["broker_values"][1][7] - (20.0 + 800.0)) < DELTA
    assert o["broker_version"] == [4, 4]


@pytest.mark.parametrize("seed", [None, 4, 5])
@pytest.mark.parametrize("drop, partitions, brokers", [
    (lambda r: r[0] == 5 and r[1] == 0, 1, 1),                       # testMissingBrokerCpuUtilization
    (lambda r: r[0] == 36 and r[1] == 0, 4, 1),                      # testMissingOtherBrokerMetrics
    (lambda r: r[0] == 4 and r[4] == "topic1" and r[5] == 0, 3, 2),  # testMissingPartitionSizeMetric
])
def test_missing_metrics(seed, drop, partitions, brokers):
    _, o = process([r for r in S.basic_records() if not drop(r)], seed=seed)
    assert (o["num_partition_samples"], o["num_broker_samples"]) == (partitions, brokers)


@pytest.mark.parametrize("seed", [None, 6])
def test_missing_topic_bytes_in(seed):
    records = [r for r in S.basic_records() if not (r[0] in (2, 3, 11, 12) and r[1] == 0 and r[4] == "topic1")]
    _, o = process(records, seed=seed)
    assert (o["num_partition_samples"], o["num_broker_samples"]) == (4, 2)
    assert o["partition_values"][0][:4] == [0.0, 100.0, 0.0, 0.0]  # T1P0: no IO, no CPU


def test_cpu_capacity_estimation():
    nan = float("nan")
    p, o = process(S.basic_records(), cores=(nan, nan))
    assert p.cached_cores == {} and o["num_partition_samples"] == 0 and o["partition_skip"] == [3, 3, 3, 3]
    p, o = process(S.basic_records(), cores=(32.0, nan))
    assert p.cached_cores == {0: 32.0} and o["partition_skip"] == [0, 3, 0, 0]
    p.clear()
    p.add(S.basic_records(300))
    o = p.process(S.BASIC_PARTITIONS, [0, 1], [nan, 8.0])  # a cached value survives clear and a later NaN
    assert p.cached_cores == {0: 32.0, 1: 8.0} and o["num_partition_samples"] == 4


def test_estimated_cpu_util_produce_only():
    assert abs(S.estimate_cpu_per_core(W, 50.0, 1000.0, 0.0, 2000.0, 1000.0, 0.0 + 0.0) - 35.0) < 0.01


def test_avg_adds_in_arrival_order_and_latest_keeps_the_first_of_equal_times():
    for order, want in (((1e16, 1.0, -1e16), 0.0), ((1e16, -1e16, 1.0), 1.0 / 3)):
        records = [r for r in S.basic_records() if not (r[0] == 19 and r[1] == 0)]
        records += [(19, 0, 100, v, None, -1) for v in order]
        _, o = process(records)
        assert o["broker_values"][0][S.metric_def_of(19)] == want
    records = S.basic_records() + [(4, 0, 100, 111.0 * S.MB, "topic1", 0), (4, 0, 101, 7.0 * S.MB, "topic2", 0),
                                   (4, 0, 101, 8.0 * S.MB, "topic2", 0)]
    _, o = process(records)
    assert o["partition_values"][0][1] == 100.0 and o["partition_values"][2][1] == 7.0


def test_dotted_topic_and_a_broker_that_leads_nothing():
    partitions = S.BASIC_PARTITIONS + [("a.b", 0, 1, 1), ("a_b", 0, 1, 1)]
    records = S.basic_records() + [(4, 1, 100, 3.0 * S.MB, "a_b", 0), (2, 1, 100, 4096.0, "a_b", -1)]
    records += [(t, 9, 100, 1.0, None, -1) for t in S.BROKER_TYPES]
    _, o = process(records, partitions, [0, 1, 9], (32.0, 32.0, 32.0))
    # "a.b" and "a_b" are one metric topic but two topics of the leader distribution: one leader each
    assert o["partition_values"][4][2] == 4.0 and o["partition_values"][5][2] == 4.0
    assert o["broker_skip"] == [0, 0, 0] and o["broker_version"] == [4, 4, 5]  # broker 9 leads nothing: enough metrics
    assert o["broker_values"][2][1] == 0.0


def test_versions_and_the_follower_fetch_rule():
    v4 = [t for t in S.BROKER_TYPES if S.version_since(t) == 4]
    for types, nrep, version, skip in ((S.BROKER_TYPES, 2, 5, 0), (v4, 2, 4, 0), (v4 + [43], 2, 4, 0),
                                       ([t for t in S.BROKER_TYPES if t != 18], 2, -1, 2),
                                       ([t for t in S.BROKER_TYPES if t != 18], 1, 5, 0),
                                       ([t for t in S.BROKER_TYPES if t != 22], 1, -1, 2),
                                       ([t for t in S.BROKER_TYPES if t not in S.ALLOWED_MISSING], 1, 5, 0)):
        records = [(t, 3, 10, 2.0, None, -1) for t in types] + [(4, 3, 10, 1.0, "x", 0)]
        _, o = process(records, [("x", 0, 3, nrep)], [3], (4.0,))
        assert o["broker_skip"] == [skip], types
        assert o["broker_version"] == ([version] if skip == 0 else [])
        if skip == 0 and version == 4:
            assert o["broker_values"][0][S.metric_def_of(43)] == 0.0  # nullable: reset even when it was reported


def test_list_bin_order_against_jhashset():
    rng = random.Random(1)
    for n in (1, 5, 12, 13, 24, 25, 48, 49, 100, 300):
        names = ["topic-%d" % rng.randrange(10 ** 7) for _ in range(n)]
        names = list(dict.fromkeys(names))
        hashes = [S.string_hash(x) for x in names]
        keys = S.OrderedKeys(True)
        for x, h in zip(names, hashes):
            keys.add(x, h)
        assert keys.order() == [names[i] for i in S.hashset_order(names, hashes, True)], n
        pairs = [(x, rng.randrange(50)) for x in names]
        hashes = [S.topic_partition_hash(t, p) for t, p in pairs]
        keys = S.OrderedKeys(False)
        for k, h in zip(pairs, hashes):
            keys.add(k, h)
        assert keys.order() == [pairs[i] for i in S.hashset_order(["-"] * len(pairs), hashes, False)], n


def test_tree_bin_takes_the_emulated_order():
    names = [""]
    for _ in range(4):
        names = [x + blk for x in names for blk in ("Aa", "BB")]
    keys = S.OrderedKeys(True)
    for x in names:
        keys.add(x, S.string_hash(x))
    assert keys.tree and keys.early_resize_or_tree() and sorted(keys.order()) == sorted(names)
    with pytest.raises(S.TreeBin):
        m = S.JHashMap()
        for x in names:
            m.put_if_absent(x, S.string_hash(x), lambda: None)


def test_known_answers():
    for c in KAT["avg"]:
        h = S.Holder(False)
        for v in c["values"]:
            h.record(unhx(v), 0)
        assert hx(h.get()) == c["result"]
    for c in KAT["latest"]:
        h = S.Holder(True)
        for t, v in c["records"]:
            h.record(unhx(v), t)
        assert hx(h.get()) == c["result"]
    for c in KAT["cpu"]:
        r = S.estimate_cpu_per_core([unhx(x) for x in c["weights"]], *[unhx(x) for x in c["args"]])
        assert (None if r is None else hx(r)) == c["result"]
    for c in KAT["tphash"]:
        assert S.string_hash(c["topic"]) == c["topic_hash"] and S.topic_partition_hash(c["topic"], c["partition"]) == c["result"]
    b = KAT["basic_round"]
    p = S.Processor()
    p.add([(t, br, tm, unhx(v), topic, part) for t, br, tm, v, topic, part in b["records"]])
    o = p.process(S.BASIC_PARTITIONS, S.BASIC_NODES, [32.0, 32.0])
    assert [[hx(v) for v in row] for row in o["partition_values"]] == b["partition_values"]
    assert [[hx(v) for v in row] for row in o["broker_values"]] == b["broker_values"]
    assert o["broker_version"] == b["broker_version"] and o["partition_skip"] == b["partition_skip"]
