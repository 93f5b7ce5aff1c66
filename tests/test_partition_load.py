"""ccmi_partition_load: the partition load response keyed, sorted and gathered on the device
(kernels/partition_load.hip).

The reference of every test is partition_load_support.Restatement: per-replica float32 windows and double running sums
from the desc, the oracle's action log replayed on them in the operations of loadops.h, the value rules of
Load.expectedUtilizationFor and Python's sorted on (-key, rank, partition). test_partition_load_reference.py pins it to
the oracle. The product's records are compared with its records byte for byte: order, the four values, the brokers.
"""
import random
import re

import numpy as np
import pytest

import ccmi
from acceptance_support import DEFAULT_GOALS, ChainCase, props
from oracle_binding import ArrayDesc, desc_arrays
from parity import constraint
from partition_load_support import (AVG, CPU, DEFAULT, DISK, LEADERSHIP, MAX, MODES, MOVE, NW_IN, NW_OUT, Restatement,
                                    assert_same)
from test_hosts import SHARED, _model as hosts_model
from test_ingest import _random_cluster_via_builder

pytestmark = pytest.mark.gpu

RES = ccmi.RESOURCES  # CPU, NW_IN, NW_OUT, DISK
ALL = 2 ** 31 - 1
TILE = 2048  # kPlSortTile: entries per workgroup of a sort pass
JSON_KEYS = {"topic", "partition", "leader", "followers", "cpu", "networkInbound", "networkOutbound", "disk"}


def check_all(cm, rs, tie_rank=None, combos=None):
    """Every (resource, mode), no selection, all entries; returns the expected orders."""
    orders = {}
    for res, mode in combos or [(r, m) for r in range(4) for m in (DEFAULT, MAX, AVG)]:
        want, n = rs.expected(res, mode, tie_rank)
        assert_same(cm.partition_load(RES[res], tie_rank=tie_rank, **MODES[mode]), want, n)
        assert n == rs.P
        orders[(res, mode)] = want.tobytes()
    return orders


@pytest.fixture(scope="module")
def chained(gpu_lib, oracle_lib):
    """props(20) after the default goals: the session, and the restatement with the log replayed."""
    c = ChainCase.random(gpu_lib, **props(20))
    c.optimize(DEFAULT_GOALS, constraint(1.05, max_replicas=3000))
    return c, Restatement(c.desc).apply(c.oc.actions())


# ------------------------------------------------------------------------------------------------ T1
@pytest.mark.parametrize("num_brokers", [20, 130], ids=["b20", "b130"])
def test_fresh_and_after_the_default_goals(gpu_lib, oracle_lib, num_brokers):
    """4 resources x 3 modes, no selection, every record, on the fresh session and after the chain (its action log
    equal to the oracle's, ChainCase). The chain relocates leaderships, so a stale rLoad or pLeader would not pass."""
    c = ChainCase.random(gpu_lib, **props(num_brokers))
    rs = Restatement(c.desc)
    launches = c.cm.perf().stats_launches
    fresh = check_all(c.cm, rs)
    assert c.cm.perf().stats_launches > launches
    c.optimize(DEFAULT_GOALS, constraint(1.05, max_replicas=3000))
    actions = c.oc.actions()
    assert sum(1 for a in actions if a[0] == LEADERSHIP) >= 1
    rs.apply(actions)
    after = check_all(c.cm, rs)
    assert all(after[k] != fresh[k] for k in fresh)
    p = c.cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)  # not an acceptance call


# ------------------------------------------------------------------------------------------------ T2
def test_three_windows_through_the_builder(gpu_lib, oracle_lib):
    """num_windows = 3 (test_ingest's builder model with two dead brokers): the three modes read different things —
    the mean of the windows, their maximum, the latest one for DISK. The model has replication factor 4 on 3 racks, so
    the chain is the default goals without RackAwareGoal, which fails there before it moves anything."""
    m, _ = _random_cluster_via_builder(gpu_lib, seed=2, dead=(4, 9))
    c = ChainCase(gpu_lib, m.desc(), m)
    assert c.desc.num_windows == 3
    rs = Restatement(c.desc)
    for stage in ("fresh", "chained"):
        if stage == "chained":
            c.optimize([g for g in DEFAULT_GOALS if g != "RackAwareGoal"], constraint(1.05, 3000))
            rs.apply(c.oc.actions())
        check_all(c.cm, rs)
        for res in range(4):
            default, mx, avg = (rs.keys(res, mode) for mode in (DEFAULT, MAX, AVG))
            assert default != mx and avg != mx, (stage, res)
            # without the max flag only DISK tells the modes apart: latest against avg
            assert (default != avg) == (res == DISK), (stage, res)


# ------------------------------------------------------------------------------------------------ T3
def _ties_model(gpu_lib):
    """A random desc (5,020 partitions: three sort tiles, the last one partial) with three edits: partitions
    [1980, 2121), 141 of them (more than two wavefronts) across the boundary of the first sort tile at 2048, get one and
    the same leader load; partitions [3000, 3070) all-zero leader loads; five leaders (two of them, 2047 and 2048,
    inside the tied range and on either side of the tile boundary) and two followers get no load at all
    (num_replica_loads < R)."""
    base = ccmi.RandomCluster.generate(gpu_lib, num_racks=5, num_brokers=20, num_replicas=15000, num_topics=300)
    a = {k: list(v) if not isinstance(v, int) else v for k, v in desc_arrays(base.desc).items()}
    R, P = len(a["replica_partition"]), len(a["partition_topic"])
    assert P > 2 * TILE and P % TILE != 0
    leader = {a["replica_partition"][r]: r for r in range(R) if a["is_leader"][r]}
    tied, zero = list(range(1980, 2121)), list(range(3000, 3070))
    proto = a["load"][leader[tied[0]] * 6:leader[tied[0]] * 6 + 6]
    for p in tied:
        a["load"][leader[p] * 6:leader[p] * 6 + 6] = proto
    for p in zero:
        a["load"][leader[p] * 6:leader[p] * 6 + 6] = [0.0] * 6
    empty = [4000, 4001, 4002, 2047, 2048]
    followers = [r for r in range(R) if not a["is_leader"][r]][:2]
    unloaded = {leader[p] for p in empty} | set(followers)
    tied = [p for p in tied if p not in empty]  # 139 stay tied, on both sides of the two emptied ones at the boundary
    assert len(tied) >= 130
    a["load_order"] = [r for r in range(R) if r not in unloaded]
    flat = ArrayDesc(a)
    flat.desc.num_replica_loads = len(a["load_order"])
    assert flat.desc.num_replica_loads == R - 7 < R
    return flat, base, tied, zero, empty


def test_ties_zeros_and_empty_loads(gpu_lib):
    flat, base, tied, zero, empty = _ties_model(gpu_lib)
    cm = ccmi.ClusterModel(flat.desc, lib=gpu_lib, keepalive=(flat, base))
    rs = Restatement(flat.desc)
    P = rs.P
    rng = np.random.default_rng(20261020)
    some = [(DISK, DEFAULT), (CPU, MAX), (NW_OUT, AVG), (NW_IN, MAX)]
    by_index = check_all(cm, rs)
    permuted = check_all(cm, rs, rng.permutation(P).astype(np.int32), some)
    repeated = check_all(cm, rs, rng.integers(-3, 3, P).astype(np.int32), some)  # duplicates, and negative ranks
    for k in some:  # the rank decided among the equal keys
        assert by_index[k] != permuted[k] and by_index[k] != repeated[k] and permuted[k] != repeated[k]
    # the equal keys sit next to each other, in index order without ranks
    full = cm.partition_load("DISK").records
    at = {int(p): i for i, p in enumerate(full["partition"])}
    assert [at[p] for p in tied] == list(range(at[tied[0]], at[tied[0]] + len(tied)))
    # max mode: a leader whose windows are all zero reports Float.MIN_VALUE per metric, an empty load 0.0, and the
    # zeros sort before the empties
    mx = cm.partition_load("CPU", max_load=True)
    at = {int(p): i for i, p in enumerate(mx.records["partition"])}
    for p in zero:
        u = mx.records["util"][at[p]]
        assert (u[CPU], u[NW_OUT], u[NW_IN], u[DISK]) == (2.0 ** -149, 2.0 ** -148, 2.0 ** -148, 2.0 ** -149)
    for p in empty:
        assert list(mx.records["util"][at[p]]) == [0.0] * 4
    assert max(at[p] for p in zero) < min(at[p] for p in empty)
    assert sorted(at[p] for p in zero + empty) == list(range(P - len(zero) - len(empty), P))
    js = {(e["topic"], e["partition"]): e for e in mx.get_json_structure()["records"]}
    names = cm.topic_names()
    e = js[(names[flat.desc.partition_topic[zero[0]]], flat.desc.partition_number[zero[0]])]
    assert e["cpu"] == 2.0 ** -149 and e["networkOutbound"] == 2.0 ** -148
    # default mode: both groups are 0.0 and come in index order
    dflt = cm.partition_load("CPU").records
    assert list(dflt["partition"][P - len(zero) - len(empty):]) == sorted(zero + empty)


# ------------------------------------------------------------------------------------------------ T4
def test_selection_and_entries(chained):
    """Topic regex, partition bounds, broker ids (after the chain: the current brokers decide) and combinations, each
    with the entries cuts around a wavefront and around the selected count: the answer is the matching subsequence of
    the full list, cut."""
    c, rs = chained
    names, ids = c.cm.topic_names(), c.cm.broker_ids()
    full, _ = rs.expected(DISK, DEFAULT)
    assert_same(c.cm.partition_load("DISK"), full, rs.P)
    some_brokers = [3, 11]
    moved_in = [p for p in range(rs.P)
                if any(rs.broker[r] in some_brokers for r in rs.slots[p])
                != any(c.desc.replica_broker[r] in some_brokers for r in rs.slots[p])]
    assert moved_in  # the desc's brokers would select other partitions
    selections = [dict(topic=r".*[0-4]"), dict(topic=re.escape(names[1])), dict(partition_range=(1, 4)),
                  dict(partition_range=(2, 2)), dict(broker_index=some_brokers),
                  dict(topic=r".*[0-4]", partition_range=(0, 5), broker_index=some_brokers),
                  dict(topic="no such topic")]
    for sel in selections:
        keep = set(rs.selected(**sel))
        want = full[np.array([int(p) in keep for p in full["partition"]], dtype=bool)]
        n = len(want)
        assert n == len(keep) and (n > 0) == (sel.get("topic") != "no such topic")
        kwargs = {k: v for k, v in sel.items() if k != "broker_index"}
        if "broker_index" in sel:
            kwargs["broker_ids"] = [ids[b] for b in sel["broker_index"]]
        for entries in sorted({0, 1, 63, 64, 65, n, n + 1, ALL}):
            got = c.cm.partition_load("DISK", entries=entries, **kwargs)
            assert_same(got, want[:entries], n)
    assert len(rs.selected(topic=re.escape(names[1]))) < len(rs.selected(topic=r".*"))
    # another resource and mode under a selection, against the restatement's own selection and sort
    want, n = rs.expected(NW_OUT, MAX, topic=r".*[5-9]", partition_range=(0, 3))
    assert 0 < n < rs.P
    assert_same(c.cm.partition_load("NW_OUT", max_load=True, topic=r".*[5-9]", partition_range=(0, 3)), want, n)
    empty = c.cm.partition_load("DISK", partition_range=(5, 4))  # lower > upper
    assert len(empty.records) == 0 and empty.num_selected == 0



# ------------------------------------------------------------------------------------------------ T5
def test_pending_rows_and_loads_reach_the_device_first(gpu_lib, oracle_lib):
    """ccmi_session_apply leaves dirty rows and dirty chain loads on the host; partition_load right after it, with
    nothing in between, must see them (the entry point flushes both lists and the launcher sends them first)."""
    bc = constraint(1.05, max_replicas=3000)
    c = ChainCase.random(gpu_lib, **props(20))
    c.optimize(DEFAULT_GOALS, bc)
    rs = Restatement(c.desc).apply(c.oc.actions())
    before = c.cm.partition_load("NW_OUT").records
    d = c.desc
    off = list(d.partition_offset[:d.num_partitions + 1])
    dist, leaders = c.oc.replica_distribution(), c.oc.leader_distribution()
    rnd = random.Random(7)
    actions, touched, led = [], set(), []
    for p in rnd.sample(range(d.num_partitions), d.num_partitions):
        here = dist[off[p]:off[p + 1]]
        free = [b for b in range(d.num_brokers) if b not in here and b not in touched]
        src = [b for b in here if b not in touched]
        if len(actions) < 3 and free and src:
            actions.append((MOVE, p, src[0], free[0], -1, -1, -1))
            touched |= {src[0], free[0]}
        elif 3 <= len(actions) < 5 and len(here) > 1:
            followers = [b for b in here if b != leaders[p]]
            actions.append((LEADERSHIP, p, leaders[p], followers[0], -1, -1, -1))
            led.append(p)
        if len(actions) == 5:
            break
    assert [a[0] for a in actions] == [MOVE, MOVE, MOVE, LEADERSHIP, LEADERSHIP]
    assert c.cm.apply(actions) == 5
    got = c.cm.partition_load("NW_OUT")  # nothing between apply and the call
    c.oc.apply(actions)
    assert c.cm.actions() == c.oc.actions()
    rs.apply(actions)
    want, n = rs.expected(NW_OUT, DEFAULT)
    assert_same(got, want, n)
    old = {int(r["partition"]): r.tobytes() for r in before}
    new = {int(r["partition"]): r.tobytes() for r in got.records}
    changed = {p for p in old if old[p] != new[p]}
    assert set(led) <= changed and {a[1] for a in actions} == changed


# ------------------------------------------------------------------------------------------------ T6
def test_many_partitions_and_fewer_than_a_wavefront(gpu_lib):
    """About 20K partitions on a fresh session: at least three sort tiles, the last one partial (the count is no
    multiple of the tile). And test_hosts.SHARED, a builder model whose partitions do not fill one wavefront."""
    buf = ccmi.RandomCluster.generate(gpu_lib, num_racks=5, num_brokers=50, num_replicas=60003, num_topics=3000)
    P = buf.desc.num_partitions  # 20,051: nine whole tiles and one of 1,619
    assert P >= 3 * TILE and P % TILE != 0
    cm = ccmi.ClusterModel.from_buffers(buf)
    rs = Restatement(buf.desc)
    rank = np.random.default_rng(5).integers(0, 1 << 30, P).astype(np.int32)
    check_all(cm, rs, combos=[(DISK, DEFAULT), (NW_IN, AVG), (CPU, MAX)])
    check_all(cm, rs, rank, combos=[(NW_OUT, DEFAULT)])
    want, n = rs.expected(DISK, DEFAULT, entries=100, partition_range=(0, 2))
    assert_same(cm.partition_load("DISK", entries=100, partition_range=(0, 2)), want, n)
    cm.close()
    flat = hosts_model(SHARED)
    small = ccmi.ClusterModel(flat.desc, lib=gpu_lib, keepalive=flat)
    assert 0 < flat.desc.num_partitions < 64
    check_all(small, Restatement(flat.desc))


# ------------------------------------------------------------------------------------------------ T7
def test_repeats_errors_and_json(chained):
    c, rs = chained
    log = c.cm.actions()
    first = c.cm.partition_load("NW_IN", avg_load=True, entries=500)
    again = c.cm.partition_load("NW_IN", avg_load=True, entries=500)
    assert first == again and first.records.tobytes() == again.records.tobytes() and len(first.records) == 500
    assert c.cm.actions() == log == c.oc.actions()  # reading changed nothing
    with pytest.raises(ccmi.IllegalArgumentException):
        c.cm.partition_load("DISK", max_load=True, avg_load=True)
    with pytest.raises(ccmi.IllegalArgumentException):
        c.cm.partition_load(4)
    with pytest.raises(ccmi.IllegalArgumentException):
        c.cm.partition_load(-1)
    with pytest.raises(ccmi.IllegalArgumentException):
        c.cm.partition_load("DISK", entries=-1)
    with pytest.raises(ccmi.IllegalArgumentException):
        c.cm.partition_load("DISK", tie_rank=[0, 1, 2])
    import ctypes as C
    q = ccmi.PartitionLoadQueryStruct()
    q.resource, q.entries = DISK, 5
    q.partition_lower, q.partition_upper = -2 ** 31, 2 ** 31 - 1
    n = C.c_int64(0)
    lib = c.cm.lib.lib
    for args in ((None, C.byref(q), None, C.byref(n), None), (c.cm.handle, None, None, C.byref(n), None),
                 (c.cm.handle, C.byref(q), None, None, None), (c.cm.handle, C.byref(q), None, C.byref(n), None)):
        assert lib.ccmi_partition_load(*args) == 1  # CCMI_E_INVALID: a NULL s, q, num_records, records
    q.entries = 0
    assert lib.ccmi_partition_load(c.cm.handle, C.byref(q), None, C.byref(n), None) == 0 and n.value == 0
    assert c.cm.partition_load("NW_IN", avg_load=True, entries=500) == first  # and the errors changed nothing
    js = first.get_json_structure()
    assert set(js) == {"version", "records"} and js["version"] == 1 and len(js["records"]) == 500
    names, ids = c.cm.topic_names(), c.cm.broker_ids()
    for e, r in zip(js["records"], first.records):
        assert set(e) == JSON_KEYS  # no msg_in
        p = int(r["partition"])
        assert e["topic"] == names[c.desc.partition_topic[p]] and e["partition"] == c.desc.partition_number[p]
        brokers = rs.brokers(p)
        assert e["leader"] == ids[brokers[0]] and e["followers"] == [ids[b] for b in brokers[1:]]
        assert (e["cpu"], e["networkInbound"], e["networkOutbound"], e["disk"]) == tuple(float(x) for x in r["util"])
        assert isinstance(e["leader"], int) and isinstance(e["disk"], float)
