"""ccmi_builder_populate_from_aggregator (K18, kernels/load_model.hip): the bulk model load against the parent path on the
same device aggregator, aggregate() followed by one ccmi_builder_populate_partition per returned row in ascending entity
order (tests/test_ingest.py pins that loop to the oracle). Every desc field, the broker ids and the topic names are
compared exactly and replica_load as bit patterns; the random cases also check every partition's loads against the
oracle's oc_ingest_partition. There is no tolerance.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ccmi
import load_model_support as L
import metric_aggregator_support as S
from parity import check_desc_against_oracle, constraint
from test_ingest import CAP as KAT_CAP, _leader_util, _two_node_model

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "cruise-control_amd", "csrc", "engine", "devtypes.h")) as _f:
    _DEVTYPES = _f.read()
BLOCK = int(re.search(r"constexpr int kAggBlock = (\d+);", _DEVTYPES).group(1))
MAX_BLOCKS = int(re.search(r"constexpr int kAggMaxBlocks = (\d+);", _DEVTYPES).group(1))
TILE = int(re.search(r"constexpr int kAggTile = (\d+);", _DEVTYPES).group(1))
ALL_TIME = L.ALL_TIME
# (rows, W, largest RF, seed): seeds picked on the CPU so that Case.features() holds what test_random_topologies asserts
RANDOM_CASES = [(1, 3, 8, 47), (TILE - 1, 1, 8, 1), (TILE, 3, 8, 1), (TILE + 1, 5, 8, 1),
                (BLOCK * MAX_BLOCKS + 1, 1, 3, 1)]
EVERY_FEATURE = ("rows_are_the_sampled", "not_a_row", "empty_range", "offline", "follower_before_leader",
                 "follower_after_leader", "zero_bytes", "topic_first_kept_is_not_its_first")


def parent(lib, case, agg, topo, calls, model=None):
    """aggregate() and the per-row loop for every (options, interested) of `calls`, on a fresh model unless given."""
    m = model or L.new_model(lib, case.W)
    results = []
    for o, interested in calls:
        res = agg.aggregate(*ALL_TIME, o, interested)
        L.populate_per_row(m, res, topo)
        results.append(res)
    return m, results


def bulk(lib, case, agg, topo, calls, model=None):
    m = model or L.new_model(lib, case.W)
    outs = [m.populate_from_aggregator(agg, *ALL_TIME, o, topo, interested) for o, interested in calls]
    return m, outs


def check_completeness(got, want):
    assert (got.failure, got.generation) == (want.failure, want.generation)
    assert got.windows.tolist() == want.windows.tolist() and got.included.tolist() == want.included.tolist()
    assert (got.num_interested_entities, got.num_interested_groups, got.num_valid_entities, got.num_valid_groups) == \
        (want.num_interested_entities, want.num_interested_groups, want.num_valid_entities, want.num_valid_groups)
    for name in ("valid_entity_ratio_by_window", "valid_entity_ratio_with_group_granularity_by_window",
                 "valid_entity_group_ratio_by_window", "extrapolated_entity_ratio_by_window"):
        assert S.float_bits(getattr(got, name)).tolist() == S.float_bits(getattr(want, name)).tolist(), name
    assert S.float_bits([got.valid_entity_ratio, got.valid_entity_group_ratio]).tolist() == \
        S.float_bits([want.valid_entity_ratio, want.valid_entity_group_ratio]).tolist()


def check_against_oracle(oracle_lib, case, model, res):
    """Every populated partition's loads against oc_ingest_partition on the row's six leader metrics."""
    W = case.W
    loads = L.loads_of(model)
    lead = np.ascontiguousarray(res.values[:, L.PICK, :], dtype=np.float32)
    fn = oracle_lib.oc_ingest_partition
    fn.restype = C.c_int32
    out = np.zeros(8 * 6 * W, dtype=np.float32)
    r = 0
    for row, e in enumerate(res.entities.tolist()):
        if not case.kept(e):
            continue
        reps = case.replicas(e)
        n = len(reps)
        flags = (C.c_uint8 * n)(*[1 if b == case.leader_broker_id[e] else 0 for b in reps])
        fn(W, n, flags, lead[row].ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
        assert np.array_equal(loads[r * 6 * W:(r + n) * 6 * W].view(np.uint32), out[:n * 6 * W].view(np.uint32)), e
        r += n
    assert r * 6 * W == loads.size


# ---------------------------------------------------------------------------------------------- 1. the KAT
def test_load_monitor_two_node_kat(gpu_lib):
    """LoadMonitorTest.testBasicClusterModel from samples: window i, sample j records i * 10 + j for every metric
    (CPU / 100), four samples a window, through the device aggregator and the bulk call: the partition leader's
    utilization over windows 0 and 1 is CPU 6.5, NW_IN / NW_OUT / DISK 13."""
    window_ms, parts = 1000, [("topic0", 0), ("topic0", 1), ("topic1", 0), ("topic1", 1)]
    agg = ccmi.MetricSampleAggregator(2, window_ms, 4, L.FNS, [0, 0, 1, 1], lib=gpu_lib)
    ents, times, vals = [], [], []
    for i in range(3):  # the third window is the current one and is not aggregated
        for j in range(4):
            for e in range(4):
                ents.append(e)
                times.append(i * window_ms + j)
                vals.append([(i * 10 + j) / 100.0] + [float(i * 10 + j)] * 8)
    agg.add_samples(ents, times, vals)
    topo = ccmi.PartitionTopology(["topic0", "topic1"], [0, 0, 1, 1], [0, 1, 0, 1], [0, 2, 4, 6, 8], [0, 1] * 4, [0] * 4)
    o = ccmi.AggregationOptions(0.0, 0.0, 1, 0, ccmi.GRANULARITY_ENTITY, False)
    m = _two_node_model(gpu_lib, 2)
    c = m.populate_from_aggregator(agg, *ALL_TIME, o, topo)
    assert (c.num_rows, c.num_populated, c.failure) == (4, 4, ccmi.AGG_FAILURE_NONE)
    for p in range(4):
        assert _leader_util(m, p) == {"CPU": 6.5, "NW_IN": 13.0, "NW_OUT": 13.0, "DISK": 13.0}
    want = _two_node_model(gpu_lib, 2)
    res = agg.aggregate(*ALL_TIME, o)
    for row, (t, p) in enumerate(parts):
        res.populate_partition(want, row, t, p, [0, 1], 0)
    L.assert_same(L.snapshot(m), L.snapshot(want))
    assert KAT_CAP["CPU"] == 100.0


# ---------------------------------------------------------------------------------------------- 2. seeded topologies
@pytest.mark.parametrize("rows,W,max_rf,seed", RANDOM_CASES, ids=["rows%d-W%d" % (c[0], c[1]) for c in RANDOM_CASES])
def test_random_topologies(gpu_lib, oracle_lib, rows, W, max_rf, seed):
    """B = 12 with two brokers created dead, per-replica offline flags, two JBOD brokers, RF 1..8. Row counts: 1, around
    the compaction tile, and one more than a grid-stride pass has lanes. One row cannot be an empty-range, an offline
    and a populated partition at once, so the one-row case asserts what one row can hold."""
    case = L.Case(seed, rows, W, max_rf=max_rf)
    f = case.features()
    assert (f["rows"], f["windows"]) == (rows, W)
    if rows == 1:
        assert f["rows_are_the_sampled"] and f["not_a_row"] and f["follower_before_leader"] and f["follower_after_leader"]
    else:
        assert all(f[k] for k in EVERY_FEATURE), f
    agg, topo = case.aggregator(gpu_lib), case.topology()
    calls = [(L.options(), None)]
    want, (res,) = parent(gpu_lib, case, agg, topo, calls)
    got, (c,) = bulk(gpu_lib, case, agg, topo, calls)
    assert res.entities.tolist() == case.row_entities
    assert c.num_rows == rows and c.num_populated == sum(1 for e in case.row_entities if case.kept(e))
    check_completeness(c, res.completeness)
    L.assert_same(L.snapshot(L.finish_model(got)), L.snapshot(L.finish_model(want)))
    check_against_oracle(oracle_lib, case, got, res)


# ---------------------------------------------------------------------------------------------- 3. zero rows
def test_include_invalid_entities(gpu_lib):
    """Under include_invalid_entities the interested entities are the rows: the absent ones and the ones without a
    valid window come with zeros and become zero-load partitions, as in the per-row loop."""
    case = L.Case(3, 40, 3)
    agg, topo = case.aggregator(gpu_lib), case.topology()
    everyone = np.ones(case.E, dtype=np.uint8)
    calls = [(L.options(include_invalid=True), everyone)]
    want, (res,) = parent(gpu_lib, case, agg, topo, calls)
    got, (c,) = bulk(gpu_lib, case, agg, topo, calls)
    assert c.num_rows == case.E == len(res.entities)
    absent_kept = [e for e in case.absent + case.late if case.kept(e)]
    assert absent_kept, "the seed leaves no absent entity to populate"
    snap = L.snapshot(got)
    L.assert_same(snap, L.snapshot(want))
    d, loads = got.desc(), L.loads_of(got).reshape(-1, 6, case.W)
    kept = [e for e in range(case.E) if case.kept(e)]
    assert c.num_populated == len(kept)
    for e in case.absent:
        if case.kept(e):
            p = kept.index(e)
            assert not loads[d.partition_offset[p]:d.partition_offset[p + 1]].any()


# ---------------------------------------------------------------------------------------------- 4. two calls
def test_two_calls_append(gpu_lib):
    case = L.Case(4, 300, 3)
    agg, topo = case.aggregator(gpu_lib), case.topology()
    odd = (np.arange(case.E) % 2).astype(np.uint8)
    calls = [(L.options(), odd), (L.options(), 1 - odd)]
    want, results = parent(gpu_lib, case, agg, topo, calls)
    got, outs = bulk(gpu_lib, case, agg, topo, calls)
    assert [c.num_rows for c in outs] == [len(r.entities) for r in results] and all(c.num_rows > 100 for c in outs)
    snap = L.snapshot(got)
    L.assert_same(snap, L.snapshot(want))
    # the topics are in first-appearance order of the populated partitions, across the two calls
    order = []
    for r in results:
        for e in r.entities.tolist():
            if case.kept(e) and case.topic_names[case.partition_topic[e]] not in order:
                order.append(case.topic_names[case.partition_topic[e]])
    assert snap["topic_names"] == order and order != sorted(order)
    # a mask selecting nothing means every present entity
    nothing = np.zeros(case.E, dtype=np.uint8)
    a, (ca,) = bulk(gpu_lib, case, agg, topo, [(L.options(), nothing)])
    b, (cb,) = bulk(gpu_lib, case, agg, topo, [(L.options(), None)])
    assert ca.num_rows == cb.num_rows == case.rows
    L.assert_same(L.snapshot(a), L.snapshot(b))


# ---------------------------------------------------------------------------------------------- 5. failure outcomes
def test_failure_outcomes(gpu_lib):
    case = L.Case(5, 30, 3)
    agg, topo = case.aggregator(gpu_lib), case.topology()
    m, _ = bulk(gpu_lib, case, agg, topo, [(L.options(), None)])
    before = L.snapshot(m)
    c = m.populate_from_aggregator(agg, *ALL_TIME, L.options(min_valid_windows=4), topo)
    assert c.failure == ccmi.AGG_FAILURE_NOT_ENOUGH_VALID_WINDOWS and (c.num_rows, c.num_populated) == (0, 0)
    c = m.populate_from_aggregator(agg, 50_000, 90_000, L.options(), topo)
    assert c.failure == ccmi.AGG_FAILURE_NO_WINDOW_IN_RANGE and (c.num_rows, c.num_populated) == (0, 0)
    L.assert_same(L.snapshot(m), before)
    two = L.new_model(gpu_lib, 2)  # the aggregate has three valid windows
    empty = L.snapshot(two)
    with pytest.raises(ccmi.IllegalArgumentException, match="3 valid windows"):
        two.populate_from_aggregator(agg, *ALL_TIME, L.options(), topo)
    L.assert_same(L.snapshot(two), empty)
    with pytest.raises(ccmi.IllegalArgumentException):
        m.populate_from_aggregator(agg, *ALL_TIME, L.options(min_valid_windows=0), topo)
    with pytest.raises(ccmi.IllegalArgumentException, match="metric_of"):
        m.populate_from_aggregator(agg, *ALL_TIME, L.options(), topo, metric_of=[0, 1, 2, 3, 7, 9])
    L.assert_same(L.snapshot(m), before)


# ---------------------------------------------------------------------------------------------- 6. errors
def _per_row_message(lib, case, agg, topo):
    with pytest.raises(ccmi.IllegalArgumentException) as info:
        parent(lib, case, agg, topo, [(L.options(), None)])
    return str(info.value)


def test_errors_leave_the_builder_unchanged(gpu_lib):
    case = L.Case(6, 2 * TILE + 100, 1)
    agg, good = case.aggregator(gpu_lib), case.topology()
    m, _ = bulk(gpu_lib, case, agg, good, [(L.options(), None)])
    before = L.snapshot(m)
    assert before["num_partitions"] > TILE
    # row entities with at least three replicas that are populated, one per compaction tile
    rich = [e for e in case.row_entities if case.kept(e) and len(case.replicas(e)) >= 3]
    low = next(e for e in rich if e < TILE // 2)
    high = next(e for e in rich if e > 2 * TILE)

    def refused(topo, text):
        with pytest.raises(ccmi.IllegalArgumentException) as info:
            m.populate_from_aggregator(agg, *ALL_TIME, L.options(), topo)
        assert text in str(info.value), str(info.value)
        L.assert_same(L.snapshot(m), before)
        return str(info.value)

    def not_leader(e):
        return next(b for b in range(L.NUM_BROKERS) if b not in case.replicas(e))

    # each complaint in the per-row call's words
    for edit, text in (({("replica", low): 77}, "replica on unknown broker 77 (create it first"),
                       ({("replica", low): case.replicas(low)[1]}, "duplicate replica broker"),
                       ({("leader", low): not_leader(low)}, "is not one of its replica brokers")):
        topo = broken_from(case, edit)
        assert refused(topo, text) == _per_row_message(gpu_lib, case, agg, topo)
    # two bad partitions two tiles apart: the lower entity's complaint, whichever kind it is
    topo = broken_from(case, {("replica", low): 77, ("leader", high): not_leader(high)})
    refused(topo, "replica on unknown broker 77")
    topo = broken_from(case, {("leader", low): not_leader(low), ("replica", high): 77})
    msg = refused(topo, "is not one of its replica brokers")
    assert "partition %s-%d:" % (case.topic_names[case.partition_topic[low]], case.partition_number[low]) in msg
    # an offline partition is still checked for unknown and duplicate brokers
    offline = next(e for e in case.row_entities if case.replicas(e) and case.leader_broker_id[e] < 0)
    refused(broken_from(case, {("replica", offline): 77}), "replica on unknown broker 77")
    # a bad partition that is not a row of the aggregate is no error
    outsider = next(e for e in case.late + case.absent if case.replicas(e))
    again = L.new_model(gpu_lib, case.W)
    c = again.populate_from_aggregator(agg, *ALL_TIME, L.options(), broken_from(case, {("replica", outsider): 77}))
    assert c.num_populated == before["num_partitions"]
    # the shape of the topology
    nine = list(case.replica_offset)
    e9 = next(e for e in range(case.E) if len(case.replicas(e)) == 8 and len(case.replicas(e + 1)) >= 1)
    nine[e9 + 1] += 1
    refused(case.topology(replica_offset=nine), "at most 8")
    down = list(case.replica_offset)
    down[5] = down[4] - 1 if down[4] > 0 else down[6] + 1
    refused(case.topology(replica_offset=down), "replica_offset decreases")
    topics = list(case.partition_topic)
    topics[low] = len(case.topic_names)
    refused(case.topology(partition_topic=topics), "topic index out of range")
    logdirs = list(case.replica_logdir)
    logdirs[0] = len(L.LOGDIRS)
    refused(case.topology(replica_logdir=logdirs), "logdir index out of range")
    short = L.Case(6, 10, 1)
    refused(short.topology(), "partitions, the aggregator")
    with pytest.raises(ccmi.IllegalArgumentException):
        gpu_lib.check(gpu_lib.lib.ccmi_builder_populate_from_aggregator(m.handle, agg.handle, -1, 1, None, None, None,
                                                                        None, None, None, None))
    L.assert_same(L.snapshot(m), before)


def broken_from(case, edits):
    brokers, leaders = list(case.replica_broker_id), list(case.leader_broker_id)
    for (kind, e), value in edits.items():
        if kind == "replica":
            brokers[case.replica_offset[e]] = value
        else:
            leaders[e] = value
    return case.topology(replica_broker_id=brokers, leader_broker_id=leaders)


# ---------------------------------------------------------------------------------------------- 7. end to end
def test_bulk_loaded_model_matches_oracle(gpu_lib, oracle_lib):
    """A B = 12, 160-partition model built by the bulk call runs the default goals bit-exactly against the oracle, with
    brokers 4 and 9 dead and brokers 2 and 5 on BAD_DISKS with offline replicas, as in test_ingest's INGEST_CASES."""
    m = e2e_model(gpu_lib, lambda case: case.aggregator(gpu_lib), bulk_load)
    assert m.desc().num_partitions == 160
    cm, res, _ = check_desc_against_oracle(gpu_lib, m.desc(), m, list(ccmi.DEFAULT_GOALS), constraint(1.05, 3000))
    assert res is not None and len(cm.actions()) > 0  # the goals ran and moved replicas; nothing ended in an exception


E2E_BAD = (2, 5)


def e2e_case():
    case = L.Case(7, 160, 3, max_rf=4, extra=0, topics=20, p_skip=0.0)  # every partition is populated
    rng = np.random.default_rng(7)
    assert all(case.kept(e) for e in range(case.E))
    # replicas are offline on BAD_DISKS brokers only
    case.replica_offline = [1 if b in E2E_BAD and rng.random() < 0.5 else 0 for b in case.replica_broker_id]
    return case


def bulk_load(m, case, agg):
    c = m.populate_from_aggregator(agg, *ALL_TIME, L.options(), case.topology(replica_logdir=None, logdir_names=()))
    assert c.num_populated == case.E


def e2e_model(lib, make_agg, load):
    case = e2e_case()
    m = ccmi.LoadMonitorModel(num_windows=case.W, lib=lib)
    for b in range(L.NUM_BROKERS):
        m.create_broker("rack%d" % (b % 4), "h%d" % b, b, KAT_CAP, alive=b not in L.DEAD)  # RF 4 needs four racks
    load(m, case, make_agg(case))
    for b in L.DEAD:
        m.set_broker_state(b, "DEAD")
    for b in E2E_BAD:
        m.set_broker_state(b, "BAD_DISKS")
    return m
