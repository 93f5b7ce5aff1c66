"""The remove-disks operation (RemoveDisksRunnable): ccmi_session_mark_disks_for_removal, goal kind 24
(IntraBrokerDiskCapacityGoal(true)) and ClusterModel.remove_disks against the restatement in remove_disks_support.py.

Every case runs on the CPU emulation (emu) and on the device (gpu): the action log, the final replica_disks, the
proposals with logdirs and the outcome (success, or the failure's message and recommendation) must equal the
yardstick's; after a mark, the queries must answer as a fresh session created with those disk capacities 0.0 (stats
within 1e-9 relative, the project's stats bar; broker stats, which only the device library has, row for row).
Deck parameters are chosen with the yardstick alone and asserted on it, never on the code under test.
"""
import ctypes as C
import functools
import math

import pytest

import ccmi
from remove_disks_support import (LOGDIR0, LOGDIR1, REMOVE_DISKS_TEST_ROWS, Yardstick, ZeroedDesc, assert_matches,
                                  product_outcome, remove_disks_test_model)

FOUR_LOGDIRS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=200, rack_aware=1, jbod=2,
                    num_logdirs=4, logdir_capacity=[75000.0] * 4)  # the four-logdirs deck of test_jbod.py
# one broker with more selected entries than the kernel's LDS snapshots (2,048) and sort tile (512) hold
BIG_BROKER = dict(num_racks=4, num_brokers=4, num_replicas=12000, num_topics=100, jbod=2, num_logdirs=4,
                  logdir_capacity=[600000.0] * 4)
CAP16, CAP24 = "IntraBrokerDiskCapacityGoal", ccmi.REMOVE_DISKS_GOAL


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue(request.param + "_lib")


def constraint(thr):
    bc = ccmi.BalancingConstraint()
    bc.set_capacity_threshold(thr)
    return bc


def session(lib, desc, keep):
    return ccmi.ClusterModel(desc, lib=lib, keepalive=keep)


def logdirs_of(y, disks):
    out = {}
    for d in disks:
        out.setdefault(y.ids[y.disk_broker[d]], []).append(y.logdir[d])
    return out


def fullest_removable(y, thr):
    """Each broker's fullest logdir, for the brokers that pass checkCanRemoveDisks on their own."""
    picks = [max(y.disks_of[b], key=lambda d: y.util[d]) for b in range(y.B) if y.broker_alive[b]]
    return [d for d in picks if y.can_remove([d], thr)]


def close(a, b):
    if isinstance(a, float) or isinstance(b, float):
        return a == b or (a != a and b != b) or math.isclose(a, b, rel_tol=1e-9, abs_tol=0.0)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(close(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(close(x, y) for x, y in zip(a, b))
    return a == b


def same_queries(lib, cm, fresh, bc):
    """Mark-then-query against the fresh zero-capacity session."""
    assert close(cm.cluster_stats(bc), fresh.cluster_stats(bc))
    if lib.has_broker_stats:
        assert cm.broker_stats() == fresh.broker_stats()


@functools.lru_cache(maxsize=None)
def generated(lib, **props):
    return ccmi.RandomCluster.generate(lib, **{k: list(v) if isinstance(v, tuple) else v for k, v in props.items()})


def deck(lib, props):
    return generated(lib, **{k: tuple(v) if isinstance(v, list) else v for k, v in props.items()})


def run_remove(lib, desc, keep, y, disks, thr, options=None):
    """check + mark + kind 24 on the product and on the yardstick `y` (fresh); returns the session."""
    y.check_can_remove(disks, thr)
    y.mark(disks)
    want = y.outcome(thr)
    cm = session(lib, desc, keep)
    got = product_outcome(cm, lambda: cm.remove_disks(logdirs_of(y, disks), constraint(thr), options))
    assert_matches(cm, y, got, want)
    return cm, want


# ------------------------------------------------------------------------------------------ (a) RemoveDisksTest
@pytest.mark.parametrize("name,load,optimizes", REMOVE_DISKS_TEST_ROWS, ids=[r[0] for r in REMOVE_DISKS_TEST_ROWS])
def test_remove_disks_test_rows(lib, name, load, optimizes):
    flat = remove_disks_test_model(load)
    y = Yardstick(flat.desc)
    cm, want = run_remove(lib, flat.desc, flat, y, y.disks_named({0: [LOGDIR0]}), 0.8)
    assert (want[0] == "ok") == optimizes
    if optimizes:
        (p,) = cm.proposals()
        assert [y.logdir[d] for d in p.old_disks] == [LOGDIR0] and [y.logdir[d] for d in p.new_disks] == [LOGDIR1]
        assert p.new_replicas == [0]
        assert cm.actions()[0][0] == 3  # INTRA_BROKER_REPLICA_MOVEMENT
    else:
        assert cm.actions() == []


def test_goal_name_and_kind(lib):
    (g,) = ccmi.goals_from_names([CAP24])
    assert g.kind == 24 and g.name() == CAP16 and g.is_hard_goal()
    flat = remove_disks_test_model(75000.0)
    cm = session(lib, flat.desc, flat)
    res = cm.remove_disks({0: [LOGDIR0]})
    assert [r.name for r in res.goal_results] == [CAP16] and res.goal_results[0].succeeded
    # an intra-broker kind wherever 16 is one: no chain with inter-broker goals, kind 16's acceptance as a prior
    with pytest.raises(ccmi.IllegalArgumentException, match="cannot be optimized together with inter-broker goals"):
        ccmi.GoalOptimizer().optimizations(session(lib, flat.desc, flat),
                                           ccmi.goals_from_names(["RackAwareGoal", CAP24]))
    d0, d1 = 0, 1  # broker 0's /mnt/i00 and /mnt/i01 in desc order
    # the replica (75000) is on /mnt/i01 now: moving it back to the zero-capacity disk is rejected, as kind 16 would
    assert cm.action_acceptance_by_goal(CAP24, 3, 0, 0, 0, -1, d1, d0) == "REPLICA_REJECT"
    assert cm.action_acceptance_by_goal(CAP24, 1, 0, 0, 0, -1, d1, d1) == "ACCEPT"  # a leadership movement
    if lib.has_moves_acceptance_mask:
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.moves_acceptance_mask([CAP24], [(0, 0, 0)])


# ------------------------------------------------------------------------------------------ the mark call
def test_check_messages(lib):
    flat = remove_disks_test_model(75000.0)
    cm = session(lib, flat.desc, flat)
    before = cm.cluster_stats()
    rows = cm.broker_stats().disks.tobytes() if lib.has_broker_stats else None
    with pytest.raises(ccmi.IllegalArgumentException, match=r"^Invalid log dirs provided for broker 1\.$"):
        cm.mark_disks_for_removal({1: ["/mnt/i07"]}, 0.8)
    with pytest.raises(ccmi.IllegalArgumentException, match=r"^Invalid log dirs provided for broker 9\.$"):
        cm.mark_disks_for_removal({9: [LOGDIR0]}, 0.8)
    # all or nothing: broker 0's request is fine, broker 2's is not
    with pytest.raises(ccmi.IllegalArgumentException,
                       match=r"^No log dir remaining to move replicas to for broker 2\.$"):
        cm.mark_disks_for_removal({0: [LOGDIR0], 2: [LOGDIR0, LOGDIR1]}, 0.8)
    with pytest.raises(ccmi.IllegalArgumentException,
                       match=r"^Not enough remaining capacity to move replicas to for broker 0\.$"):
        cm.mark_disks_for_removal({1: [LOGDIR1], 0: [LOGDIR0]}, 0.4)  # 75000 / 150000 > 0.4
    # a disk index out of range names its position; duplicates are harmless
    bad = C.c_int32(7)
    arr = (C.c_int32 * 3)(0, 0, 6)
    assert lib.lib.ccmi_session_mark_disks_for_removal(cm.handle, arr, 3, 0.8, C.byref(bad)) == 1  # CCMI_E_INVALID
    assert bad.value == 2
    assert close(cm.cluster_stats(), before)
    if rows is not None:
        assert cm.broker_stats().disks.tobytes() == rows
    # nothing was marked: kind 16 on this session equals kind 16 on a fresh one, and 0.5 passes (the test is >)
    fresh = session(lib, flat.desc, flat)
    same_queries(lib, cm, fresh, constraint(0.8))
    assert lib.lib.ccmi_session_mark_disks_for_removal(cm.handle, arr, 2, 0.5, C.byref(bad)) == 0
    assert bad.value == -1
    zero = ZeroedDesc(flat.desc, [0])
    same_queries(lib, cm, session(lib, zero.desc, (flat, zero)), constraint(0.8))


def test_no_disks_and_state(lib):
    buf = deck(lib, dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300))
    cm = ccmi.ClusterModel.from_buffers(buf)
    arr = (C.c_int32 * 1)(0)
    assert lib.lib.ccmi_session_mark_disks_for_removal(cm.handle, arr, 1, 0.8, None) == 1  # no disks: CCMI_E_INVALID
    flat = remove_disks_test_model(75000.0)
    cm = session(lib, flat.desc, flat)
    ccmi.GoalOptimizer().optimizations(cm, ccmi.goals_from_names([CAP16]))
    with pytest.raises(ccmi.IllegalStateException):
        cm.mark_disks_for_removal({0: [LOGDIR0]}, 0.8)
    cm = session(lib, flat.desc, flat)
    cm.apply([(3, 0, 0, 0, -1, 0, 1)])
    with pytest.raises(ccmi.IllegalStateException):
        cm.mark_disks_for_removal({0: [LOGDIR1]}, 0.8)


def test_mark_then_query_equals_a_fresh_zero_capacity_session(lib):
    buf = deck(lib, FOUR_LOGDIRS)
    y = Yardstick(buf.desc)
    disks = fullest_removable(y, 0.8)
    assert len(disks) == 20
    bc = constraint(0.8)
    zero = ZeroedDesc(buf.desc, disks)
    for goals in ([CAP16], list(ccmi.INTRA_BROKER_GOALS)):
        cm, fresh = ccmi.ClusterModel.from_buffers(buf), session(lib, zero.desc, (buf, zero))
        cm.mark_disks_for_removal(logdirs_of(y, disks), 0.8)
        same_queries(lib, cm, fresh, bc)
        outs = [product_outcome(m, lambda m=m: ccmi.GoalOptimizer(bc).optimizations(m, ccmi.goals_from_names(goals)))
                for m in (cm, fresh)]
        assert outs[0] == outs[1]
        assert cm.actions() == fresh.actions() and len(cm.actions()) > 0
        assert cm.replica_disks() == fresh.replica_disks()
        same_queries(lib, cm, fresh, bc)


# ------------------------------------------------------------------------------------------ (b), (c): four logdirs
def test_four_logdirs_drained(lib):
    """Threshold 0.15: 12 brokers pass the check and are drained; the other 8 are over it and do kind 16's work."""
    thr = 0.15
    buf = deck(lib, FOUR_LOGDIRS)
    y = Yardstick(buf.desc)
    disks = fullest_removable(y, thr)
    marked_brokers = {y.disk_broker[d] for d in disks}
    assert 10 <= len(disks) < 20
    cm, want = run_remove(lib, buf.desc, buf, y, disks, thr)
    assert want == ("ok",) and all(not y.members[d] for d in disks)
    assert sum(len(y.members[d]) for d in range(y.D)) == y.R
    # the brokers without a marked disk: exactly kind 16's records on the unmarked desc
    plain = ccmi.ClusterModel.from_buffers(buf)
    product_outcome(plain, lambda: ccmi.GoalOptimizer(constraint(thr)).optimizations(
        plain, ccmi.goals_from_names([CAP16])))
    others = [a for a in cm.actions() if a[2] not in marked_brokers]
    assert others == [a for a in plain.actions() if a[2] not in marked_brokers] and len(others) > 0
    zero = ZeroedDesc(buf.desc, disks)
    after = session(lib, zero.desc, (buf, zero))
    after.apply(cm.actions())
    same_queries(lib, cm, after, constraint(thr))


def test_four_logdirs_a_disk_that_cannot_be_emptied(lib):
    """The threshold at which the fullest broker's utilization equals its remaining limit: it passes the check (>) and
    cannot place its last replicas (<), so its drained disk stays over the limit."""
    buf = deck(lib, FOUR_LOGDIRS)
    y = Yardstick(buf.desc)
    top = max(range(y.D), key=lambda d: y.util[d])
    thr = y.util[top] / (3 * 75000.0)
    disks = fullest_removable(y, thr)
    assert top in disks and len(disks) == 20
    cm, want = run_remove(lib, buf.desc, buf, y, disks, thr)
    assert want[0] == "fail" and want[2] == 1 and "is above capacity limit" in want[1]
    stuck = [d for d in disks if y.members[d]]
    assert stuck and f"logdir={y.logdir[stuck[0]]}," in want[1] and want[1].endswith(
        f"on broker {y.ids[y.disk_broker[stuck[0]]]} is above capacity limit.")


# ------------------------------------------------------------------------------------------ (d): a large broker
def test_broker_over_the_lds_snapshot(lib):
    buf = deck(lib, BIG_BROKER)
    y = Yardstick(buf.desc)
    selected = [sum(y.selected[r] for d in y.disks_of[b] for r in y.members[d]) for b in range(y.B)]
    b = max(range(y.B), key=lambda b: selected[b])
    d = max(y.disks_of[b], key=lambda d: len(y.members[d]))
    assert selected[b] > 2048 and len(y.members[d]) > 2048
    cm, want = run_remove(lib, buf.desc, buf, y, [d], 0.8)
    assert want == ("ok",) and not y.members[d] and len(cm.actions()) > 2048


# ------------------------------------------------------------------------------------------ (e), (f): scripted
def scripted(replicas, capacity=150000.0, dead_d0=False):
    """Two brokers with /d0 and /d1; `replicas` = (topic, partition, DISK load) on broker 0 /d0, in this order.
    dead_d0: broker 0's /d0 is a dead disk (negative capacity) and its replicas are offline."""
    bld = ccmi.ClusterModelBuilder()
    cap = {"CPU": 100.0, "DISK": 2 * capacity, "NW_IN": 300000.0, "NW_OUT": 200000.0}
    for broker, rack in ((0, "r0"), (1, "r1")):
        bld.create_broker(rack, broker, cap, {"/d0": -1.0 if dead_d0 and broker == 0 else capacity, "/d1": capacity})
    for topic, partition, load in replicas:
        bld.create_replica("r0", 0, topic, partition, 0, True, dead_d0, "/d0")
        bld.set_replica_load("r0", 0, topic, partition, 1.0, 1.0, 1.0, load)
    return bld.build()


def test_zero_load_replica_moves_only_with_the_flag(lib):
    flat = scripted([("normal", 0, 0.0)])
    y = Yardstick(flat.desc)
    (d0,), (d1,) = y.disks_named({0: ["/d0"]}), y.disks_named({0: ["/d1"]})
    cm, want = run_remove(lib, flat.desc, flat, y, [d0], 0.8)
    assert want == ("ok",) and cm.actions() == [(3, 0, 0, 0, -1, d0, d1)]
    other = session(lib, flat.desc, flat)  # kind 16 on the marked model: the empty replica stays
    other.mark_disks_for_removal({0: ["/d0"]}, 0.8)
    res = ccmi.GoalOptimizer(constraint(0.8)).optimizations(other, ccmi.goals_from_names([CAP16]))
    assert res.goal_results[0].succeeded and other.actions() == []
    assert other.replica_disks() == [d0]


def test_excluded_topic_replica_cannot_leave(lib):
    flat = scripted([("excluded", 0, 0.0)])
    t = flat.topics.index("excluded")
    y = Yardstick(flat.desc, excluded_topics=[t])
    cm, want = run_remove(lib, flat.desc, flat, y, y.disks_named({0: ["/d0"]}), 0.8,
                          options=ccmi.OptimizationOptions(excluded_topics=[t]))
    # isUtilizationOverLimit (:270-275) is true for an alive zero-capacity disk that holds any replica, so the
    # over-limit throw of updateGoalState (:235-242) comes before "Could not move all replicas" (:243-246)
    assert want == ("fail", "[IntraBrokerDiskCapacityGoal] Utilization (0.00) for disk Disk[logdir=/d0,state=ALIVE,"
                    "capacity=0.000000,replicaCount=1] on broker 0 is above capacity limit.", 1, 0.0)
    assert cm.actions() == []


def test_marked_dead_disk_keeps_its_replica(lib):
    """The throw that is not behind disk.isAlive(): a dead disk marked for removal (capacity 0, still dead) whose
    offline replica no intra-broker move can take away. No provision recommendation."""
    flat = scripted([("t", 0, 10.0)], dead_d0=True)
    y = Yardstick(flat.desc)
    (d0,) = y.disks_named({0: ["/d0"]})
    assert not y.alive[d0] and y.cap[d0] == -1.0
    cm, want = run_remove(lib, flat.desc, flat, y, [d0], 0.8)
    assert want == ("fail", "[IntraBrokerDiskCapacityGoal] Could not move all replicas from disk /d0 on broker 0",
                    None, None)
    assert cm.actions() == [] and y.cap[d0] == 0.0


@pytest.mark.parametrize("small,sign", [(1e-3, 1), (5e-3, -1)], ids=["positive-residue", "negative-residue"])
def test_drained_disk_residue(lib, small, sign):
    """Disk._utilization is not clamped: 0 + 1e9 + s - 1e9 - s in doubles (the larger replica leaves first) is a
    residue of a few 1e-8. Positive: the empty disk is still over its limit ("Utilization (0.00)"); negative: not."""
    flat = scripted([("t", 0, 1e9), ("t", 1, small)], capacity=4e9)
    y = Yardstick(flat.desc)
    (d0,) = y.disks_named({0: ["/d0"]})
    cm, want = run_remove(lib, flat.desc, flat, y, [d0], 0.8)
    assert not y.members[d0] and y.util[d0] != 0 and (y.util[d0] > 0) == (sign > 0) and abs(y.util[d0]) < 1e-6
    assert [a[1] for a in y.actions] == [0, 1]
    if sign > 0:
        assert want[0] == "fail" and "Utilization (0.00) for disk Disk[logdir=/d0,state=ALIVE,capacity=0.000000," \
            "replicaCount=0] on broker 0 is above capacity limit." in want[1]
        assert want[2] == 1 and want[3] == y.util[d0] / 0.8
    else:
        assert want == ("ok",)
