"""ccmi_metrics_processor on the device (kernels/metrics_processor.hip) against the plain-Python restatement of
CruiseControlMetricsProcessor (tests/metrics_processor_support.py), both fed the same records in the same arrival order.
Doubles are compared as bit patterns with NaN canonical, skip tables and counts exactly. There is no tolerance.
"""
import os
import random
import re

import numpy as np
import pytest

import ccmi
import metrics_processor_support as S

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "cruise-control_amd", "csrc", "engine", "metrics_processor.h")) as _f:
    _HDR = _f.read()
BLOCK = int(re.search(r"constexpr int kMpBlock = (\d+);", _HDR).group(1))
SORT_TILE = int(re.search(r"constexpr int kMpSortTile = (\d+);", _HDR).group(1))
HASH_SEED = 0  # picked on the CPU: test_hash_order asserts what it was picked for


def run_both(lib, records, partitions, node_ids, cores, interested=None, mode=0, batches=2, dev=None, ref=None):
    """One round on the device and on the restatement, compared; -> (device result, restatement dict)"""
    dev = dev or ccmi.MetricsProcessor(lib=lib)
    ref = ref or S.Processor()
    step = max(1, (len(records) + batches - 1) // batches)
    for i in range(0, len(records), step):
        dev.add_metrics(*S.record_columns(records[i:i + step]))
    ref.add(records)
    got = dev.process(*S.cluster_columns(partitions), node_ids, cores, interested=interested, sampling_mode=mode)
    want = ref.process(partitions, node_ids, cores, interested=interested, mode=mode)
    S.assert_same(got, want)
    return got, want


def shuffled(records, seed):
    r = list(records)
    random.Random(seed).shuffle(r)
    return r


# ------------------------------------------------------------------------------------------ reference scenarios
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_basic(gpu_lib, seed):
    got, _ = run_both(gpu_lib, shuffled(S.basic_records(), seed), S.BASIC_PARTITIONS, S.BASIC_NODES, [32.0, 32.0])
    assert got.num_partition_samples == 4 and got.num_broker_samples == 2 and got.max_metric_timestamp == 102
    cpu_b0 = lambda p_in, p_out: 32.0 * S.estimate_cpu_per_core((0.7, 0.15, 0.15), 50.0, 820.0, 1380.0 + 20.0 + 800.0,
                                                                500.0, p_in, p_out)
    expected = {0: (cpu_b0(20.0, 100.0), 20.0, 80.0, 100.0),
                1: (32.0 * S.estimate_cpu_per_core((0.7, 0.15, 0.15), 30.0, 500.0, 1000.0, 820.0, 500.0, 1000.0),
                    500.0, 500.0, 300.0),
                2: (cpu_b0(400.0, 1050.0), 400.0, 650.0, 200.0), 3: (cpu_b0(400.0, 1050.0), 400.0, 650.0, 500.0)}
    for e, row in zip(got.partition_entity.tolist(), got.partition_values):
        cpu, bytes_in, bytes_out, disk = expected[e]
        assert abs(row[0] - cpu) < 0.001 and abs(row[2] - bytes_in) < 0.001
        assert abs(row[3] - bytes_out) < 0.001 and abs(row[1] - disk) < 0.001
    assert abs(got.broker_values[0][7] - 500.0) < 0.001 and abs(got.broker_values[1][7] - 820.0) < 0.001


@pytest.mark.parametrize("drop, partitions, brokers", [
    (lambda r: r[0] == 5 and r[1] == 0, 1, 1),                       # testMissingBrokerCpuUtilization
    (lambda r: r[0] == 36 and r[1] == 0, 4, 1),                      # testMissingOtherBrokerMetrics
    (lambda r: r[0] == 4 and r[4] == "topic1" and r[5] == 0, 3, 2),  # testMissingPartitionSizeMetric
])
def test_missing_metrics(gpu_lib, drop, partitions, brokers):
    records = [r for r in S.basic_records() if not drop(r)]
    got, _ = run_both(gpu_lib, shuffled(records, 5), S.BASIC_PARTITIONS, S.BASIC_NODES, [32.0, 32.0])
    assert (got.num_partition_samples, got.num_broker_samples) == (partitions, brokers)


def test_missing_topic_bytes_in(gpu_lib):
    records = [r for r in S.basic_records() if not (r[0] in (2, 3, 11, 12) and r[1] == 0 and r[4] == "topic1")]
    got, _ = run_both(gpu_lib, shuffled(records, 6), S.BASIC_PARTITIONS, S.BASIC_NODES, [32.0, 32.0])
    assert (got.num_partition_samples, got.num_broker_samples) == (4, 2)
    assert got.partition_values[0].tolist()[:4] == [0.0, 100.0, 0.0, 0.0]


@pytest.mark.parametrize("cores, cached", [([np.nan, np.nan], (None, None)), ([32.0, np.nan], (32.0, None))])
def test_cpu_capacity_resolution(gpu_lib, cores, cached):
    dev = ccmi.MetricsProcessor(lib=gpu_lib)
    got, _ = run_both(gpu_lib, S.basic_records(), S.BASIC_PARTITIONS, S.BASIC_NODES, cores, dev=dev)
    assert (dev.cached_num_cores(0), dev.cached_num_cores(1)) == cached
    assert got.num_partition_samples == (0 if cached[0] is None else 3)


def test_cached_cores_survive_clear_and_nan(gpu_lib):
    dev, ref = ccmi.MetricsProcessor(lib=gpu_lib), S.Processor()
    run_both(gpu_lib, S.basic_records(), S.BASIC_PARTITIONS, S.BASIC_NODES, [16.0, 8.0], dev=dev, ref=ref)
    dev.clear()
    ref.clear()
    got, _ = run_both(gpu_lib, S.basic_records(200), S.BASIC_PARTITIONS, S.BASIC_NODES, [np.nan, 4.0], dev=dev, ref=ref)
    assert (dev.cached_num_cores(0), dev.cached_num_cores(1), dev.cached_num_cores(7)) == (16.0, 8.0, None)
    assert got.num_partition_samples == 4 and got.max_metric_timestamp == 202


# ------------------------------------------------------------------------------------------ generated rounds
def mixed(rng):
    return rng.uniform(0.1, 1.0) * 10.0 ** rng.randint(0, 15)


def generate(rng, num_nodes, num_topics, num_partitions, rf=2, repeats=(1, 3), value=mixed, dotted=True):
    """A round: every node reports its broker types, the topic types and partition sizes of the replicas it hosts"""
    node_ids = rng.sample(range(1000), num_nodes)
    topics = [("t.%d" if dotted and i % 3 == 0 else "t%d") % i for i in range(num_topics)]
    partitions, hosted = [], {}
    for p in range(num_partitions):
        topic, number = topics[p % num_topics], p // num_topics
        replicas = rng.sample(node_ids, min(rf, num_nodes))
        partitions.append((topic, number, replicas[0], len(replicas)))
        for b in replicas:
            hosted.setdefault(b, []).append((S.replace_dots(topic), number))
    records = []
    for b in node_ids:
        v5 = rng.random() < 0.7
        for t in S.BROKER_TYPES:
            if S.version_since(t) == 5 and not v5:
                continue
            if t in S.ALLOWED_MISSING and rng.random() < 0.2:
                continue
            for _ in range(rng.randint(*repeats)):
                records.append((t, b, rng.randint(0, 1000), value(rng), None, -1))
        for topic in sorted({tp[0] for tp in hosted.get(b, [])}):
            for t in S.TOPIC_TYPES:
                if rng.random() < 0.15:
                    continue
                for _ in range(rng.randint(*repeats)):
                    records.append((t, b, rng.randint(0, 1000), value(rng), topic, -1))
        for topic, number in hosted.get(b, []):
            for _ in range(rng.randint(*repeats)):
                records.append((4, b, rng.choice((5, 5, 9, 700)), value(rng), topic, number))
    rng.shuffle(records)
    return records, partitions, node_ids


def test_wave_and_block_edges(gpu_lib):
    rng = random.Random(11)
    num_partitions = 3 * BLOCK + 5
    records, partitions, node_ids = generate(rng, 70, 40, num_partitions)
    # one holder whose run in the sorted records is longer than a workgroup, so it straddles a block boundary
    records += [(19, node_ids[33], 10 + i, mixed(rng), None, -1) for i in range(BLOCK + 7)]
    rng.shuffle(records)
    assert len(records) > 2 * SORT_TILE  # more than one radix tile
    cores = [float(rng.choice((8, 16, 32))) for _ in node_ids]
    got, _ = run_both(gpu_lib, records, partitions, node_ids, cores, batches=3)
    assert got.num_partition_samples > BLOCK and got.num_broker_samples > 0


def hash_order_round(seed):
    """Three brokers with 13, 25 and 49 reported topics (one, two and three resizes), values of mixed magnitude"""
    rng = random.Random(seed)
    node_ids, records, partitions = [7, 3, 11], [], []
    for b, count in zip(node_ids, (13, 25, 49)):
        for t in S.BROKER_TYPES:
            records.append((t, b, 10, mixed(rng), None, -1))
        for i in range(count):
            topic = "b%d_topic_%d" % (b, rng.randrange(10 ** 6))
            partitions.append((topic, 0, b, 1))
            for t in S.TOPIC_TYPES:
                records.append((t, b, 10, mixed(rng), topic, -1))
            records.append((4, b, 10, mixed(rng), topic, 0))
    rng.shuffle(records)
    return records, partitions, node_ids


def test_hash_order(gpu_lib):
    records, partitions, node_ids = hash_order_round(HASH_SEED)
    got, want = run_both(gpu_lib, records, partitions, node_ids, [8.0] * 3)
    assert got.num_broker_samples == 3 and got.num_hash_fallback_brokers == 0
    # the seed's property: some summed type and diskUsage differ in their bits from the sums in two convenient orders
    first = {}
    for t, b, _, v, topic, part in records:
        if t == 4:
            first.setdefault(b, []).append((topic, v))
    differs_sum = differs_disk = False
    for s, b in enumerate(node_ids):
        by_arrival = [topic for topic, _ in first[b]]
        by_index = [p[0] for p in partitions if p[2] == b]
        value = {(t, topic): v for t, bb, _, v, topic, _ in records if bb == b and topic is not None}
        for order in (by_arrival, by_index):
            for t in S.SUM_TARGET:
                total = 0.0
                for topic in order:
                    total += value[(t, topic)]
                reported = S.convert_unit(total, S.SUM_TARGET[t])
                other = want["broker_values"][s][S.metric_def_of(S.SUM_TARGET[t])]
                differs_sum |= S.bits([reported])[0] != S.bits([other])[0]
            total = 0.0
            for topic in order:
                total += value[(4, topic)]
            differs_disk |= S.bits([total / (1024 * 1024)])[0] != S.bits([want["broker_values"][s][1]])[0]
    assert differs_sum and differs_disk


def equal_hash_names():
    names = [""]
    for _ in range(4):
        names = [n + blk for n in names for blk in ("Aa", "BB")]
    assert len({S.string_hash(n) for n in names}) == 1 and len(names) == 16
    return names


def test_tree_bin(gpu_lib):
    records, partitions, node_ids = hash_order_round(HASH_SEED + 100)
    rng = random.Random(4)
    b = 21
    node_ids.append(b)
    for t in S.BROKER_TYPES:
        records.append((t, b, 10, mixed(rng), None, -1))
    for topic in equal_hash_names():
        partitions.append((topic, 0, b, 1))
        for t in S.TOPIC_TYPES:
            records.append((t, b, 10, mixed(rng), topic, -1))
        records.append((4, b, 10, mixed(rng), topic, 0))
    rng.shuffle(records)
    got, want = run_both(gpu_lib, records, partitions, node_ids, [8.0] * 4)
    assert got.num_hash_fallback_brokers == 1 and got.num_broker_samples == 4


def skip_code_round():
    rng = random.Random(2)
    records, partitions, node_ids = generate(rng, 6, 5, 40, value=lambda r: r.uniform(1.0, 100.0), dotted=True)
    a, b, c, d, e, f = node_ids
    records = [r for r in records if not (r[1] == a and r[0] == 5)]            # code 2: no BROKER_CPU_UTIL
    records = [r for r in records if r[1] != b]                                # code 2 / broker skip 1: no load
    cores = [8.0, 8.0, float("nan"), 8.0, 8.0, 8.0]                            # code 3 on c
    led_d = [p for p in partitions if p[2] == d]
    gone_topic = S.replace_dots(led_d[0][0])
    records = [r for r in records if not (r[1] == d and r[0] == 4 and r[4] == gone_topic)]       # code 4
    led_e = [p for p in partitions if p[2] == e]
    records = [r for r in records if not (r[1] == e and r[0] == 4 and r[4] == S.replace_dots(led_e[0][0])
                                          and r[5] == led_e[0][1])]                              # code 5 (maybe 4)
    # code 7: a partition whose bytes in exceed the broker's total: f reports one huge topic value, but the sums are
    # not taken because f misses a led topic's partition sizes (not enough metrics), so its reported totals stay
    led_f = [p for p in partitions if p[2] == f]
    topics_f = sorted({S.replace_dots(p[0]) for p in led_f})
    miss = topics_f[-1]
    records = [r for r in records if not (r[1] == f and r[0] == 4 and r[4] == miss)]
    huge = topics_f[0]
    assert huge != miss
    records = [r for r in records if not (r[1] == f and r[0] in (0, 2) and (r[4] is None or r[4] == huge))]
    records += [(0, f, 10, 1e6, None, -1), (2, f, 999, 1e12, huge, -1)]
    # code 6: g reports no ALL_TOPIC_BYTES_IN and, missing a topic like f, never gets the sums
    g = 2000
    node_ids.append(g)
    cores.append(8.0)
    for t in S.BROKER_TYPES:
        if t != 0:
            records.append((t, g, 10, 5.0, None, -1))
    partitions += [("gt1", 0, g, 1), ("gt2", 0, g, 1)]
    records += [(4, g, 10, 7.0, "gt1", 0), (2, g, 10, 3.0, "gt1", -1)]
    partitions += [("orphan", 0, -1, 1), ("orphan", 1, 4242, 1)]              # codes 1 and 8
    records += [(5, 4242, 50, 1.0, None, -1), (4, 4242, 5000, 1.0, "orphan", 1)]  # a broker that is not a node
    rng.shuffle(records)
    return records, partitions, node_ids, cores


def test_every_skip_code(gpu_lib):
    records, partitions, node_ids, cores = skip_code_round()
    got, want = run_both(gpu_lib, records, partitions, node_ids, cores)
    assert set(got.partition_skip.tolist()) == set(range(9))
    assert {1, 2} <= set(got.broker_skip.tolist()) and got.num_dropped_records == 2
    assert got.max_metric_timestamp == 5000 and got.skipped_by_node[-1] >= 3
    # interested masks and the restricted sampling modes, each a round of its own
    mask = [i % 3 != 0 for i in range(len(partitions))]
    run_both(gpu_lib, records, partitions, node_ids, cores, interested=mask)
    for mode in (ccmi.SAMPLING_BROKER_METRICS_ONLY, ccmi.SAMPLING_PARTITION_METRICS_ONLY,
                 ccmi.SAMPLING_ONGOING_EXECUTION):
        got, _ = run_both(gpu_lib, records, partitions, node_ids, cores, mode=mode)
        assert (got.num_partition_samples == 0) == (mode == ccmi.SAMPLING_BROKER_METRICS_ONLY)
        assert (got.num_broker_samples == 0) == (mode == ccmi.SAMPLING_PARTITION_METRICS_ONLY)


def test_holder_rules(gpu_lib):
    """AVG adds in arrival order, LATEST keeps the first of equal times, a dotted topic, a broker that leads nothing"""
    for order in ((1e16, 1.0, -1e16), (1e16, -1e16, 1.0)):
        records = [r for r in S.basic_records() if not (r[0] == 19 and r[1] == 0)]
        records += [(19, 0, 100, v, None, -1) for v in order]
        records += [(4, 0, 100, 111.0 * S.MB, "topic1", 0), (4, 0, 300, 5.0 * S.MB, "topic1", 1),
                    (4, 0, 300, 6.0 * S.MB, "topic1", 1)]
        partitions = S.BASIC_PARTITIONS + [("a.b", 0, 1, 1)]
        records += [(4, 1, 100, 3.0 * S.MB, "a_b", 0), (2, 1, 100, 2048.0, "a_b", -1), (5, 9, 100, 1.0, None, -1)]
        got, want = run_both(gpu_lib, records, partitions, [0, 1, 9], [32.0, 32.0, 32.0])
        assert got.broker_values[0][12] == ((order[0] + order[1]) + order[2]) / 3
        assert got.partition_values[0][1] == 100.0  # the earlier record of equal times stays
        assert got.partition_entity.tolist()[-1] == 4 and got.partition_values[-1][2] == 2.0
        # broker 9 leads nothing, so it has enough topic metrics, but it reported one type only: version -1
        assert got.broker_node.tolist() == [0, 1] and got.broker_skip.tolist() == [0, 0, 2]


def test_state_and_errors(gpu_lib):
    dev = ccmi.MetricsProcessor(lib=gpu_lib)
    cols = S.record_columns(S.basic_records())
    cluster = S.cluster_columns(S.BASIC_PARTITIONS)
    bad = lambda **kw: [kw.get(k, c) for k, c in zip(("types", "brokers", "times", "values", "topics", "parts", "names"),
                                                     ([5], [0], [1], [1.0], [-1], [-1], ["x"]))]
    for args in (bad(types=[63]), bad(topics=[0]), bad(parts=[0]), bad(types=[2]), bad(types=[4], topics=[0]),
                 bad(times=[-1]), bad(names=["x", "x"]), bad(types=[2], topics=[1])):
        with pytest.raises(ccmi.IllegalArgumentException):
            dev.add_metrics(*args)
    dev.add_metrics(*cols)
    with pytest.raises(ccmi.IllegalArgumentException):
        dev.process(*cluster, [0, 0], [32.0, 32.0])  # duplicate node ids
    with pytest.raises(ccmi.IllegalArgumentException):
        dev.process(*cluster, [0, 1], [32.0, 32.0], sampling_mode=9)
    got = dev.process(*cluster, [0, 1], [32.0, 32.0])
    assert got.num_partition_samples == 4
    with pytest.raises(ccmi.IllegalStateException):
        dev.process(*cluster, [0, 1], [32.0, 32.0])
    with pytest.raises(ccmi.IllegalStateException):
        dev.add_metrics(*cols)
    dev.clear()
    assert dev.process(*cluster, [0, 1], [32.0, 32.0]).num_partition_samples == 0  # nothing buffered
    dev.clear()
    dev.add_metrics(*cols)
    got = dev.process(*cluster, [0, 1], [32.0, 32.0], partition_capacity=2, broker_capacity=1)
    assert (got.num_partition_samples, len(got.partition_entity), len(got.broker_node)) == (4, 2, 1)


# ------------------------------------------------------------------------------------------ process_into
def test_process_into(gpu_lib):
    """process + add_samples against process_into: the aggregators end bit for bit the same, over two rounds in
    different windows with a clear between them"""
    rng = random.Random(9)
    base, partitions, node_ids = generate(rng, 6, 5, 40)
    cores = [8.0] * len(node_ids)
    cluster = S.cluster_columns(partitions)
    fns9 = [f for _, f in ccmi.KAFKA_COMMON_METRICS]
    fns56 = fns9 + [ccmi.AGG_AVG] * 47
    sides = []
    for _ in range(2):
        sides.append((ccmi.MetricsProcessor(lib=gpu_lib),
                      ccmi.MetricSampleAggregator(8, 1000, 1, fns9, cluster[1], lib=gpu_lib),
                      ccmi.MetricSampleAggregator(8, 1000, 1, fns56, list(range(len(node_ids))), lib=gpu_lib)))
    for shift in (0, 5000):
        records = [(t, b, time + shift, v, topic, part) for t, b, time, v, topic, part in base]
        cols = S.record_columns(records)
        (mp_a, part_a, brok_a), (mp_b, part_b, brok_b) = sides
        mp_a.add_metrics(*cols)
        s = mp_a.process(*cluster, node_ids, cores)
        assert s.num_partition_samples > 10 and s.num_broker_samples > 0
        part_a.add_samples(s.partition_entity, [s.max_metric_timestamp] * len(s.partition_entity), s.partition_values)
        brok_a.add_samples(s.broker_node, [s.max_metric_timestamp] * len(s.broker_node), s.broker_values)
        mp_b.add_metrics(*cols)
        t = mp_b.process_into(*cluster, node_ids, cores, part_b, brok_b)
        assert (t.num_partition_samples, t.num_broker_samples, t.max_metric_timestamp) == \
               (s.num_partition_samples, s.num_broker_samples, s.max_metric_timestamp)
        assert t.partition_skip.tolist() == s.partition_skip.tolist() and len(t.partition_entity) == 0
        assert t.broker_skip.tolist() == s.broker_skip.tolist()
        assert t.skipped_by_node.tolist() == s.skipped_by_node.tolist()
        with pytest.raises(ccmi.IllegalStateException):
            mp_b.process_into(*cluster, node_ids, cores, part_b, brok_b)
        mp_a.clear()
        mp_b.clear()
    options = ccmi.AggregationOptions(0.0, 0.0, 1, 5, ccmi.GRANULARITY_ENTITY, True)
    for a, b in ((sides[0][1], sides[1][1]), (sides[0][2], sides[1][2])):
        sa, sb = a.state(), b.state()
        for field, _ in ccmi.AggregatorStateStruct._fields_:
            assert getattr(sa, field) == getattr(sb, field), field
        assert sa.num_samples > 0 and sa.current_window_index > 5
        ca, cb = a.completeness(-1, 10 ** 9, options), b.completeness(-1, 10 ** 9, options)
        for name in ("generation", "failure", "valid_entity_ratio", "valid_entity_group_ratio"):
            assert getattr(ca, name) == getattr(cb, name), name
        for name in ("windows", "included", "valid_entity_ratio_by_window", "extrapolated_entity_ratio_by_window"):
            assert np.array_equal(getattr(ca, name), getattr(cb, name)), name
        ra, rb = a.aggregate(-1, 10 ** 9, options), b.aggregate(-1, 10 ** 9, options)
        assert ra.num_entities == rb.num_entities > 0 and np.array_equal(ra.entities, rb.entities)
        assert np.array_equal(ra.values.view(np.uint32), rb.values.view(np.uint32))
        assert np.array_equal(ra.extrapolations, rb.extrapolations) and np.array_equal(ra.invalid, rb.invalid)
    # an aggregator that does not fit is refused before anything changes
    small = ccmi.MetricSampleAggregator(3, 1000, 1, fns9, [0, 0], lib=gpu_lib)
    mp = sides[0][0]
    mp.add_metrics(*S.record_columns(base))
    with pytest.raises(ccmi.IllegalArgumentException):
        mp.process_into(*cluster, node_ids, cores, small, None)
    with pytest.raises(ccmi.IllegalArgumentException):
        mp.process_into(*cluster, node_ids, cores, None, sides[0][1])
    assert mp.process_into(*cluster, node_ids, cores, None, None).num_partition_samples > 10
