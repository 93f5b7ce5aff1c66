"""ccmi_proposal_diff: the ExecutionProposals of the current model and their movement statistics, diffed, compacted and
summed on the device (kernels/proposal_diff.hip).

The reference is the oracle (proposal_diff_support): OracleCluster.proposals() where the oracle ran the chain, the
restated getDiff over the oracle's distributions where actions were applied from outside, and a restatement of
getMovementStats over either. The records are compared field by field, in order; the host path cm.proposals() and each
record's flags and counts are compared too (proposal_diff_support.check).
"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import ccmi
from acceptance_support import DEFAULT_GOALS, LEADERSHIP, MOVE, REPO, ChainCase, props
from parity import constraint
from proposal_diff_support import (RECORD, SENTINEL, OracleState, check, classify, expected_summary, movement_stats,
                                   raw_call, restated_diff, summary_tuple)
from test_hosts import SHARED, _model as hosts_model
from test_jbod import INTRA, JBOD_BASE, rebalance_constraint

pytestmark = pytest.mark.gpu

with open(os.path.join(REPO, "cruise-control_amd", "csrc", "engine", "devtypes.h")) as _f:
    TILE = int(re.search(r"constexpr int kPdTile = (\d+);", _f.read()).group(1))  # partitions per workgroup
assert TILE <= 2048 and TILE % 256 == 0
# the 15,000-replica cluster of test_partition_load._ties_model, without its edits: 5,020 partitions
TIES_PROPS = dict(num_racks=5, num_brokers=20, num_replicas=15000, num_topics=300)
UNTOUCHED = bytes([SENTINEL]) * RECORD.itemsize
# OracleCluster.proposals() after the default goals, computed on the CPU: partitions, proposals, inter-broker
# movements, leadership movements
CHAIN_COUNTS = {20: (2020, 1191, 1041, 150), 130: (2130, 1713, 1493, 220)}


def chain_case(gpu_lib, num_brokers):
    """(case, its initial OracleState) on props(num_brokers), nothing run yet."""
    c = ChainCase.random(gpu_lib, **props(num_brokers))
    return c, OracleState(c.oc)


def run_default_chain(c, init):
    """The default goals on both sides; the oracle's proposals, which also pin the restated getDiff."""
    c.optimize(DEFAULT_GOALS, constraint(1.05, max_replicas=3000))
    want = c.oc.proposals()
    assert restated_diff(c.desc, init, c.oc) == want
    return want


@pytest.fixture(scope="module")
def chained(gpu_lib, oracle_lib):
    """props(20) after the default goals: the case, its initial state, the expected proposals, the full answer."""
    c, init = chain_case(gpu_lib, 20)
    want = run_default_chain(c, init)
    return c, init, want, check(c.cm, want)


def assert_fresh(cm):
    st, buf, n, summary = raw_call(cm, 16)
    assert (st, n) == (0, 0) and buf == UNTOUCHED * 16
    assert summary_tuple(summary) == (0, 0, 0, 0, 0, 0)
    diff = cm.proposal_diff()
    assert len(diff.records) == 0 and diff.proposals == [] and diff.movement_stats() == [0] * 5
    assert cm.proposals() == []


# ------------------------------------------------------------------------------------------------ T1
@pytest.mark.parametrize("num_brokers", [20, 130], ids=["b20", "b130"])
def test_fresh_and_after_the_default_goals(gpu_lib, oracle_lib, num_brokers):
    """A fresh session has no proposal and leaves the buffer alone; after the default goals (action logs equal,
    ChainCase) the records and the summary equal the oracle's proposals. Replication factors 2 and 3."""
    c, init = chain_case(gpu_lib, num_brokers)
    launches = c.cm.perf().stats_launches
    assert_fresh(c.cm)
    assert c.cm.perf().stats_launches > launches
    want = run_default_chain(c, init)
    diff = check(c.cm, want)
    stats = movement_stats(want)
    assert (c.desc.num_partitions, len(want), stats[0], stats[4]) == CHAIN_COUNTS[num_brokers]
    assert stats[0] > 0 and stats[4] > 0 and stats[2] == 0  # both kinds, no disks
    assert {len(p.old_replicas) for p in want} == {2, 3}
    assert set(diff.records["old_leader_disk"]) == {-1} and set(diff.records["new_disks"].ravel()) == {-1}
    p = c.cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)  # not an acceptance call


# ------------------------------------------------------------------------------------------------ T2
def test_jbod_between_disk_moves(gpu_lib, oracle_lib):
    """The two intra-broker goals on a JBOD model: every proposal moves replicas between disks of a broker, some of
    them two, so the intra-broker sums and the disk columns carry the answer."""
    c = ChainCase.random(gpu_lib, **props(20, **JBOD_BASE))
    init = OracleState(c.oc)
    assert_fresh(c.cm)
    c.optimize(INTRA, rebalance_constraint())
    want = c.oc.proposals()
    assert restated_diff(c.desc, init, c.oc) == want
    diff = check(c.cm, want)
    s = diff.summary
    assert (len(want), s.num_intra_broker_replica_movements) == (245, 270)
    assert s.num_intra_broker_replica_movements > s.num_proposals
    assert s.num_inter_broker_replica_movements == 0 and s.num_leadership_movements == 0
    assert s.intra_broker_data_to_move_mb > 0
    assert 2 in set(diff.records["num_between_disks"])
    for r in diff.records:
        n = int(r["num_replicas"])
        assert int(r["old_leader_disk"]) >= 0
        assert min(r["old_disks"][:n]) >= 0 and min(r["new_disks"][:n]) >= 0


# ------------------------------------------------------------------------------------------------ T3
def _leadership(p, dist, leaders, off):
    """The leadership of partition p to its first follower, or None for a single replica."""
    followers = [b for b in dist[off[p]:off[p + 1]] if b != leaders[p]]
    return (LEADERSHIP, p, leaders[p], followers[0], -1, -1, -1) if followers else None


def test_tiles_and_wavefronts(gpu_lib, oracle_lib):
    """5,020 partitions: four whole tiles and a partial one. Leadership moves change the partitions of
    [TILE - 70, TILE + 70) (more than two wavefronts across a tile boundary), partition 0 and partition P - 1, and
    nothing else: two whole tiles have no changed partition, the partial one has one. Then three replica moves, one on
    a partition whose leadership moved (both flags)."""
    c = ChainCase.random(gpu_lib, **TIES_PROPS)
    desc = c.desc
    init = OracleState(c.oc)
    P, B = desc.num_partitions, desc.num_brokers
    tiles = (P + TILE - 1) // TILE
    assert P == 5020 and tiles > 2 and P % TILE != 0
    off = list(desc.partition_offset[:P + 1])
    boundary = range(TILE - 70, TILE + 70)
    actions = [a for a in (_leadership(p, init.dist, init.leaders, off) for p in [0, *boundary, P - 1]) if a]
    led = [a[1] for a in actions]
    assert led[0] == 0 and led[-1] == P - 1 and sum(1 for p in led if p in boundary) >= 130
    assert c.cm.apply(actions) == len(actions)
    c.oc.apply(actions)
    assert c.cm.actions() == c.oc.actions()
    want = restated_diff(desc, init, c.oc)
    assert [p.partition for p in want] == led
    changed_tiles = {p // TILE for p in led}
    assert changed_tiles == {0, 1, tiles - 1} and tiles - len(changed_tiles) >= 1
    assert sum(1 for p in led if p // TILE == tiles - 1) == 1
    diff = check(c.cm, want)
    assert diff.movement_stats() == [0, 0, 0, 0, len(led)] and set(diff.records["flags"]) == {2}
    # three replica moves: the old leader of a led partition, and a replica of two untouched partitions
    now = OracleState(c.oc)
    replicated = [p for p in range(2 * TILE, 3 * TILE) if off[p + 1] - off[p] >= 2]  # a tile without changes so far
    moves = []
    for p in (led[len(led) // 2], replicated[17], replicated[-1]):
        here = now.dist[off[p]:off[p + 1]]
        src = init.leaders[p] if p in led else here[-1]  # a follower either way
        moves.append((MOVE, p, src, next(b for b in range(B) if b not in here), -1, -1, -1))
    assert c.cm.apply(moves) == 3
    c.oc.apply(moves)
    want = restated_diff(desc, init, c.oc)
    assert len(want) == len(led) + 2
    diff = check(c.cm, want)
    both = {int(r["partition"]): int(r["flags"]) for r in diff.records}
    assert both[moves[0][1]] == 3 and both[moves[1][1]] == 1
    assert diff.movement_stats()[0] == 3 and diff.movement_stats()[4] == len(led) - 1


# ------------------------------------------------------------------------------------------------ T4
def test_capacity_cuts(chained):
    """The records of a cut call are the prefix of the full answer, nothing past them is written, and the summary does
    not depend on the capacity."""
    c, _, want, full = chained
    n = len(want)
    whole = full.records.tobytes()
    size = RECORD.itemsize
    summary = expected_summary(want)
    for capacity in (0, 1, 63, 64, 65, n - 1, n, n + 1):
        st, buf, got, s = raw_call(c.cm, capacity, room=capacity + 2)
        keep = min(capacity, n)
        assert (st, got) == (0, keep), capacity
        assert buf[:keep * size] == whole[:keep * size], capacity
        assert buf[keep * size:] == UNTOUCHED * (capacity + 2 - keep), capacity
        assert summary_tuple(s) == summary, capacity
        cut = c.cm.proposal_diff(capacity=capacity)
        assert cut.records.tobytes() == whole[:keep * size] and summary_tuple(cut.summary) == summary
    only = c.cm.proposal_diff(summary_only=True)
    assert len(only.records) == 0 and summary_tuple(only.summary) == summary_tuple(full.summary) == summary


# ------------------------------------------------------------------------------------------------ T5
def test_pending_rows_reach_the_device_first(gpu_lib, oracle_lib):
    """ccmi_session_apply leaves dirty rows, slot orders and leaders on the host; proposal_diff right after it, with
    nothing in between, must see them, and exactly the touched partitions' records differ from the call before."""
    c, init = chain_case(gpu_lib, 20)
    before = check(c.cm, run_default_chain(c, init))
    d = c.desc
    off = list(d.partition_offset[:d.num_partitions + 1])
    dist, leaders = c.oc.replica_distribution(), c.oc.leader_distribution()
    rnd = random.Random(7)
    actions, touched = [], set()
    for p in rnd.sample(range(d.num_partitions), d.num_partitions):
        here = dist[off[p]:off[p + 1]]
        free = [b for b in range(d.num_brokers) if b not in here and b not in touched]
        src = [b for b in here if b not in touched]
        if len(actions) < 3 and free and src:
            actions.append((MOVE, p, src[0], free[0], -1, -1, -1))
            touched |= {src[0], free[0]}
        elif 3 <= len(actions) < 5 and len(here) > 1:
            actions.append(_leadership(p, dist, leaders, off))
        if len(actions) == 5:
            break
    assert [a[0] for a in actions] == [MOVE, MOVE, MOVE, LEADERSHIP, LEADERSHIP]
    assert c.cm.apply(actions) == 5
    got = c.cm.proposal_diff()  # nothing between apply and the call
    c.oc.apply(actions)
    assert c.cm.actions() == c.oc.actions()
    want = restated_diff(d, init, c.oc)
    assert got.proposals == want and summary_tuple(got.summary) == expected_summary(want)
    check(c.cm, want)
    old = {int(r["partition"]): r.tobytes() for r in before.records}
    new = {int(r["partition"]): r.tobytes() for r in got.records}
    assert {p for p in set(old) | set(new) if old.get(p) != new.get(p)} == {a[1] for a in actions}


# ------------------------------------------------------------------------------------------------ T6
def _wide_model(rf=8, brokers=10):
    b = ccmi.ClusterModelBuilder()
    cap = {"CPU": 100.0, "DISK": 300000.0, "NW_IN": 300000.0, "NW_OUT": 200000.0}
    for bid in range(brokers):
        b.create_broker(f"r{bid % 5}", bid, cap)
    for i in range(rf):
        b.create_replica(f"r{(i + 1) % 5}", i + 1, "T", 0, i, i == 0)
        b.set_replica_load(f"r{(i + 1) % 5}", i + 1, "T", 0, 2.0, 10.0, 5.0 if i == 0 else 0.0, 1234.75)
    return b.build()


def test_small_and_wide(gpu_lib, oracle_lib):
    """test_hosts.SHARED: fewer partitions than a wavefront. And one partition of replication factor 8, the widest a
    record holds, with the leadership moved to its last replica: all eight slots are written and the new list differs
    from the old one in slots 0 and 7 only."""
    flat = hosts_model(SHARED)
    c = ChainCase(gpu_lib, flat.desc, flat)
    init = OracleState(c.oc)
    P = flat.desc.num_partitions
    assert 0 < P < 64
    assert_fresh(c.cm)
    off = list(flat.desc.partition_offset[:P + 1])
    actions = [_leadership(p, init.dist, init.leaders, off) for p in (0, 5, P - 1)]
    actions.append((MOVE, 7, init.dist[off[7] + 1], next(b for b in range(6) if b not in init.dist[off[7]:off[8]]),
                    -1, -1, -1))
    assert c.cm.apply(actions) == 4
    c.oc.apply(actions)
    want = restated_diff(flat.desc, init, c.oc)
    assert [p.partition for p in want] == [0, 5, 7, P - 1]
    check(c.cm, want)

    wide = _wide_model()
    w = ChainCase(gpu_lib, wide.desc, wide)
    init = OracleState(w.oc)
    assert wide.desc.num_partitions == 1 and init.dist == list(range(1, 9)) and init.leaders == [1]
    assert_fresh(w.cm)
    move = [(LEADERSHIP, 0, 1, 8, -1, -1, -1)]
    assert w.cm.apply(move) == 1
    w.oc.apply(move)
    want = restated_diff(wide.desc, init, w.oc)
    diff = check(w.cm, want)
    r = diff.records[0]
    assert int(r["num_replicas"]) == 8 and int(r["size"]) == 1234 and int(r["flags"]) == 2
    assert list(r["old_replicas"]) == [1, 2, 3, 4, 5, 6, 7, 8] and list(r["new_replicas"]) == [8, 2, 3, 4, 5, 6, 7, 1]
    assert diff.movement_stats() == [0, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------------------ T7
def test_repeats_and_errors(chained):
    c, _, want, full = chained
    log, host = c.cm.actions(), c.cm.proposals()
    again = c.cm.proposal_diff()
    assert again.records.tobytes() == full.records.tobytes() and bytes(again.summary) == bytes(full.summary)
    assert c.cm.actions() == log == c.oc.actions() and c.cm.proposals() == host == want  # reading changed nothing
    lib, h = c.cm.lib.lib, c.cm.handle
    n, s = C.c_int64(0), ccmi.ProposalSummaryStruct()
    room = np.zeros(4, dtype=RECORD)
    for args in ((None, room.ctypes.data, 4, C.byref(n), C.byref(s)),  # a NULL s
                 (h, room.ctypes.data, 4, None, C.byref(s)),           # a NULL num_records
                 (h, room.ctypes.data, -1, C.byref(n), C.byref(s)),    # a negative capacity
                 (h, None, 4, C.byref(n), C.byref(s))):                # NULL records with capacity > 0
        assert lib.ccmi_proposal_diff(*args) == 1  # CCMI_E_INVALID
    with pytest.raises(ccmi.IllegalArgumentException):
        c.cm.proposal_diff(capacity=-1)
    st, buf, got, _ = raw_call(c.cm, 4, with_summary=False)  # summary = NULL is accepted
    assert (st, got) == (0, 4) and buf == full.records.tobytes()[:4 * RECORD.itemsize]
    assert lib.ccmi_proposal_diff(h, None, 0, C.byref(n), None) == 0 and n.value == 0
    after = c.cm.proposal_diff()  # and the errors changed nothing
    assert after.records.tobytes() == full.records.tobytes() and bytes(after.summary) == bytes(full.summary)
    assert [classify(p)[0] for p in want] == [int(f) for f in after.records["flags"]]
