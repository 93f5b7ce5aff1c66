"""ccmi_actions_acceptance (ABI v13): Goal.actionAcceptance of many optimized goals for a batch of actions in one
device call (kernels/accept.hip), against the oracle cell by cell and against the product's own single call.

The reference is OracleCluster.action_acceptance_by_goal on an oracle cluster that ran the same chain (and, for the
state-tracking test, applied the same external actions). Every comparison is exact: the verdicts are small integers.
"""
import numpy as np
import pytest

import ccmi
from acceptance_support import (ACCEPT, BROKER_REJECT, CAPACITY_GOALS, CAPACITY_MIXED, CAPACITY_THRESHOLDS, DEFAULT_GOALS,
                                LEADERSHIP, MOVE, REPLICA_REJECT, SEED, SWAP, ChainCase, Placement,
                                directed_capacity_actions, props, run_in_fresh_process, status_of)
from parity import constraint

PROPS = props(20)
PER_TYPE = 700
# goals that both accept and reject some action of the random sample (checked on the oracle's matrix)
MIXED_GOALS = ["RackAwareGoal", "ReplicaDistributionGoal", "DiskUsageDistributionGoal",
               "NetworkInboundUsageDistributionGoal", "NetworkOutboundUsageDistributionGoal", "CpuUsageDistributionGoal",
               "TopicReplicaDistributionGoal", "LeaderReplicaDistributionGoal", "LeaderBytesInDistributionGoal"]
# the verdicts each action type draws from the 16 default goals on this sample (the oracle's counts): only a replica
# move or a swap can be a BROKER_REJECT (AbstractRackAwareGoal.java:100-106)
VERDICTS_BY_TYPE = {MOVE: {ACCEPT, REPLICA_REJECT, BROKER_REJECT}, LEADERSHIP: {ACCEPT, REPLICA_REJECT},
                    SWAP: {ACCEPT, REPLICA_REJECT, BROKER_REJECT}}


# ------------------------------------------------------------------------------------------------ samples
def random_actions(pl, rs, per_type):
    """per_type replica moves (a random replica to a broker not hosting the partition), leadership moves (the leader to a
    random follower) and swaps (two replicas of different partitions on different brokers, neither broker hosting the
    other's partition), interleaved by type so every run of consecutive actions mixes the three."""
    moves, leads, swaps = [], [], []
    R, P = len(pl.dist), len(pl.off) - 1
    while len(moves) < per_type:
        i = int(rs.randint(R))
        p = int(pl.slot_part[i])
        dst = int(rs.randint(pl.B))
        if dst not in pl.brokers(p):
            moves.append((MOVE, p, pl.dist[i], dst, -1, -1, -1))
    while len(leads) < per_type:
        p = int(rs.randint(P))
        followers = [b for b in pl.brokers(p) if b != pl.leaders[p]]
        if followers:
            leads.append((LEADERSHIP, p, pl.leaders[p], followers[int(rs.randint(len(followers)))], -1, -1, -1))
    while len(swaps) < per_type:
        i, j = int(rs.randint(R)), int(rs.randint(R))
        p, q = int(pl.slot_part[i]), int(pl.slot_part[j])
        sb, db = pl.dist[i], pl.dist[j]
        if p != q and sb != db and db not in pl.brokers(p) and sb not in pl.brokers(q):
            swaps.append((SWAP, p, sb, db, q, -1, -1))
    return [a for triple in zip(moves, leads, swaps) for a in triple]


def oracle_matrix(oc, goals, actions):
    """The reference: one OracleCluster.action_acceptance_by_goal per cell."""
    out = np.zeros((len(actions), len(goals)), dtype=np.int8)
    for i, a in enumerate(actions):
        for g, name in enumerate(goals):
            out[i, g] = ccmi.ACCEPTANCE.index(oc.action_acceptance_by_goal(name, a[0], a[1], a[2], a[3], a[4]))
    return out


def single_calls(cm, goals, actions):
    """The product's own per-cell path (ccmi_action_acceptance_by_kind)."""
    out = np.zeros((len(actions), len(goals)), dtype=np.int8)
    for i, a in enumerate(actions):
        for g, name in enumerate(goals):
            out[i, g] = ccmi.ACCEPTANCE.index(cm.action_acceptance_by_goal(name, *a))
    return out


class Case(ChainCase):
    """A product session and an oracle cluster after the same chain, a random sample and the oracle's matrix of it."""

    def __init__(self, lib, max_replicas):
        buf = ccmi.RandomCluster.generate(lib, **PROPS)
        super().__init__(lib, buf.desc, buf)
        self.optimize(DEFAULT_GOALS, constraint(1.05, max_replicas=max_replicas))
        self.sample = random_actions(self.placement(), np.random.RandomState(SEED), PER_TYPE)
        self.expected = oracle_matrix(self.oc, DEFAULT_GOALS, self.sample)
        self.expected.setflags(write=False)


@pytest.fixture(scope="module")
def cases(gpu_lib, oracle_lib):
    made = {}

    def get(max_replicas):
        if max_replicas not in made:
            made[max_replicas] = Case(gpu_lib, max_replicas)
        return made[max_replicas]
    return get


def check_sample_is_not_degenerate(expected, sample):
    """Asserted on the oracle's matrix alone, so a sample that exercises nothing cannot pass."""
    assert set(np.unique(expected)) == {ACCEPT, REPLICA_REJECT, BROKER_REJECT}
    for name in MIXED_GOALS:
        col = expected[:, DEFAULT_GOALS.index(name)]
        assert (col == ACCEPT).any() and (col != ACCEPT).any(), name
    types = np.array([a[0] for a in sample])
    for typ, verdicts in VERDICTS_BY_TYPE.items():
        assert set(np.unique(expected[types == typ])) == verdicts, typ


# ------------------------------------------------------------------------------------------------ 1. matrix parity
@pytest.mark.gpu
@pytest.mark.parametrize("max_replicas", [3000, 302])
def test_gpu_matrix_matches_oracle(cases, max_replicas):
    c = cases(max_replicas)
    types = np.array([a[0] for a in c.sample])
    if max_replicas == 3000:
        check_sample_is_not_degenerate(c.expected, c.sample)
    else:
        # 6040 replicas on 20 brokers at 302 each: ReplicaCapacityGoal refuses every replica move and nothing else
        assert sorted(np.bincount(c.oc.replica_distribution(), minlength=20)) == [302] * 20
        col = c.expected[:, DEFAULT_GOALS.index("ReplicaCapacityGoal")]
        assert (col[types == MOVE] == REPLICA_REJECT).all() and (col[types != MOVE] == ACCEPT).all()
    c.cm.reset_perf()
    c.cm.set_kernel_timing(True)
    got = c.cm.actions_acceptance(DEFAULT_GOALS, c.sample)
    c.cm.set_kernel_timing(False)
    p = c.cm.perf()
    print(f"accept_launches {p.accept_launches} accept_cells {p.accept_cells} accept_kernel_ms {p.accept_kernel_ms:.3f}; "
          f"oracle counts {np.bincount(c.expected.ravel(), minlength=3).tolist()}")
    assert got.dtype == np.int8 and got.shape == c.expected.shape
    mismatch = np.argwhere(got != c.expected)
    assert mismatch.size == 0, [(c.sample[i], DEFAULT_GOALS[g], int(got[i, g]), int(c.expected[i, g]))
                                for i, g in mismatch[:10]]
    # every one of the 16 default goals is a device goal: each cell was answered by the kernel
    assert p.accept_launches > 0
    assert p.accept_cells == len(c.sample) * len(DEFAULT_GOALS)
    assert p.accept_kernel_ms > 0
    # an [n, 7] int32 array is the same batch
    assert (c.cm.actions_acceptance(DEFAULT_GOALS, np.array(c.sample, dtype=np.int32)) == c.expected).all()


# ------------------------------------------------------------------------------------------------ 2. shape edges
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_gpu_batch_sizes_match_single_calls(cases, n):
    """Prefixes of the interleaved sample: every wavefront boundary of the type segments falls inside mixed types."""
    c = cases(3000)
    acts = c.sample[:n]
    got = c.cm.actions_acceptance(DEFAULT_GOALS, acts)
    assert got.shape == (n, len(DEFAULT_GOALS))
    assert (got == c.expected[:n]).all()
    assert (got == single_calls(c.cm, DEFAULT_GOALS, acts)).all()


@pytest.mark.gpu
def test_gpu_one_goal_and_duplicate_kinds(cases):
    c = cases(3000)
    acts = c.sample[:257]
    for name in ("RackAwareGoal", "LeaderBytesInDistributionGoal"):
        g = DEFAULT_GOALS.index(name)
        got = c.cm.actions_acceptance([name], acts)
        assert got.shape == (257, 1) and (got[:, 0] == c.expected[:257, g]).all()
    seventeen = DEFAULT_GOALS + ["RackAwareGoal"]  # a duplicate kind is a duplicate column
    got = c.cm.actions_acceptance(seventeen, acts)
    assert got.shape == (257, 17)
    assert (got[:, :16] == c.expected[:257]).all() and (got[:, 16] == c.expected[:257, 0]).all()
    assert (got == single_calls(c.cm, seventeen, acts)).all()


@pytest.mark.gpu
def test_gpu_more_goal_columns_than_one_program(cases):
    """More columns than one device program holds (kMaxGoals = 20): the goals are chunked."""
    c = cases(3000)
    acts = c.sample[:130]
    names = DEFAULT_GOALS + DEFAULT_GOALS[::-1] + DEFAULT_GOALS[:9]  # 41 columns: programs of 20, 20 and 1
    cols = [DEFAULT_GOALS.index(g) for g in names]
    got = c.cm.actions_acceptance(names, acts)
    assert (got == c.expected[:130][:, cols]).all()


# ------------------------------------------------------------------------------------------------ 3. chunk boundary
@pytest.mark.gpu
def test_gpu_chunk_boundary_matches_oracle(cases, gpu_lib, tmp_path):
    """CCMI_ACCEPT_CHUNK_ROWS is read at session create: a fresh process with 96 (rounded down to one wavefront, 64
    rows) answers n = 257 in several launches — 172 moves and leadership moves in 192 rows, 85 swaps in 128."""
    c = cases(3000)
    matrix, launches = run_in_fresh_process(gpu_lib, tmp_path, PROPS, dict(CCMI_ACCEPT_CHUNK_ROWS="96"), c.sample[:257],
                                            "cm.actions_acceptance(goals, [tuple(a) for a in sample])")
    assert launches == 5  # 320 rows in chunks of 64
    assert (np.array(matrix, dtype=np.int8) == c.expected[:257]).all()


# ------------------------------------------------------------------------------------------------ 4. capacity goals
@pytest.mark.gpu
def test_gpu_capacity_goals_directed_sample(gpu_lib, oracle_lib):
    bc = constraint(1.05, max_replicas=3000)
    bc.capacity_threshold = CAPACITY_THRESHOLDS
    c = ChainCase.random(gpu_lib, **PROPS)
    c.optimize(CAPACITY_GOALS, bc)
    cm, oc = c.cm, c.oc
    acts = directed_capacity_actions(c.desc, c.placement(), oc)
    expected = oracle_matrix(oc, CAPACITY_GOALS, acts)
    for name in CAPACITY_MIXED:
        col = expected[:, CAPACITY_GOALS.index(name)]
        assert (col == ACCEPT).any() and (col == REPLICA_REJECT).any(), name
    got = cm.actions_acceptance(CAPACITY_GOALS, acts)
    print(f"{len(acts)} directed actions; rejects per goal "
          f"{dict(zip(CAPACITY_GOALS, (expected != ACCEPT).sum(axis=0).tolist()))}")
    assert (got == expected).all()
    assert (got == single_calls(cm, CAPACITY_GOALS, acts)).all()


# ------------------------------------------------------------------------------------------------ 5. errors
@pytest.mark.gpu
def test_gpu_errors_are_the_single_calls(cases):
    c = cases(3000)
    cm, acts = c.cm, c.sample[:9]
    # a kind the session has not optimized
    with pytest.raises(ccmi.IllegalArgumentException):
        cm.action_acceptance_by_goal("RackAwareDistributionGoal", *acts[0])
    assert status_of(lambda: cm.actions_acceptance(["RackAwareGoal", "RackAwareDistributionGoal"], acts)) == \
        (ccmi.IllegalArgumentException, -1)
    # the source broker does not host the partition, at index 5 of 9
    p = acts[5][1]
    stranger = next(b for b in range(20) if b not in c.placement().brokers(p))
    bad = (MOVE, p, stranger, acts[5][2], -1, -1, -1)
    with pytest.raises(ccmi.IllegalArgumentException):
        cm.action_acceptance_by_goal("RackAwareGoal", *bad)
    assert status_of(lambda: cm.actions_acceptance(DEFAULT_GOALS, acts[:5] + [bad] + acts[6:])) == \
        (ccmi.IllegalArgumentException, 5)
    # a swap whose destination broker does not host the destination partition
    swap = next(a for a in c.sample if a[0] == SWAP)
    bad_swap = (SWAP, swap[1], swap[2], swap[3], swap[1], -1, -1)
    with pytest.raises(ccmi.IllegalArgumentException):
        cm.action_acceptance_by_goal("RackAwareGoal", *bad_swap)
    assert status_of(lambda: cm.actions_acceptance(DEFAULT_GOALS, [acts[0], bad_swap])) == \
        (ccmi.IllegalArgumentException, 1)
    # an unknown action type, and an intra-broker type asked of inter-broker goals
    for typ in (7, 3):
        unknown = (typ,) + tuple(acts[2][1:])
        with pytest.raises(ccmi.IllegalArgumentException):
            cm.action_acceptance_by_goal("RackAwareGoal", *unknown)
        assert status_of(lambda: cm.actions_acceptance(DEFAULT_GOALS, acts[:2] + [unknown])) == \
            (ccmi.IllegalArgumentException, 2)
    # indices outside the model are refused before the device sees them
    assert status_of(lambda: cm.actions_acceptance(DEFAULT_GOALS, [(MOVE, 10 ** 6, 0, 1, -1, -1, -1)])) == \
        (ccmi.IllegalArgumentException, 0)
    assert status_of(lambda: cm.actions_acceptance(DEFAULT_GOALS, [(MOVE, acts[0][1], acts[0][2], 20, -1, -1, -1)])) == \
        (ccmi.IllegalArgumentException, 0)
    # the session still answers afterwards
    assert (cm.actions_acceptance(DEFAULT_GOALS, acts) == c.expected[:9]).all()


@pytest.mark.gpu
def test_gpu_terminal_goal_is_a_state_error(gpu_lib):
    """KafkaAssignerDiskUsageDistributionGoal.actionAcceptance throws IllegalStateException (the single call: Engine::
    acceptance's terminal check), whatever else the batch asks."""
    ka = ["KafkaAssignerEvenRackAwareGoal", "KafkaAssignerDiskUsageDistributionGoal"]
    buf = ccmi.RandomCluster.generate(gpu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(ka))
    leaders = cm.leader_distribution()
    pl = Placement(buf.desc, cm.replica_distribution(), leaders)
    follower = next(b for b in pl.brokers(0) if b != leaders[0])
    a = (LEADERSHIP, 0, leaders[0], follower, -1, -1, -1)
    with pytest.raises(ccmi.IllegalStateException):
        cm.action_acceptance_by_goal(ka[1], *a)
    with pytest.raises(ccmi.IllegalStateException):
        cm.actions_acceptance(ka, [a])
    assert cm.actions_acceptance(ka[:1], [a]).tolist() == \
        [[ccmi.ACCEPTANCE.index(cm.action_acceptance_by_goal(ka[0], *a))]]


# ------------------------------------------------------------------------------------------------ 6. state tracking
@pytest.mark.gpu
def test_gpu_batch_after_session_apply_matches_oracle(gpu_lib, oracle_lib):
    """Rows ccmi_session_apply made dirty reach the device before the launch: a batch before and a batch after external
    actions (the accepted moves, leadership moves and swaps of the first batch's sample) both equal the oracle."""
    c = Case(gpu_lib, 3000)
    assert (c.cm.actions_acceptance(DEFAULT_GOALS, c.sample[:300]) == c.expected[:300]).all()
    touched, external = set(), []
    for a, row in zip(c.sample, c.expected):
        parts = {a[1], a[4]} - {-1}
        if (row == ACCEPT).all() and not (parts & touched) and len(external) < 12:
            external.append(a)
            touched |= parts
    assert {a[0] for a in external} == {MOVE, LEADERSHIP, SWAP}
    assert c.cm.apply(external) == len(external)
    c.oc.apply(external)
    pl = c.placement()
    again = random_actions(pl, np.random.RandomState(SEED + 1), 100)
    # actions on the moved partitions and brokers themselves: the reverse of every external action
    again += [(a[0], a[1], a[3], a[2], a[4], -1, -1) for a in external if a[0] != SWAP]
    again += [(SWAP, a[1], a[3], a[2], a[4], -1, -1) for a in external if a[0] == SWAP]
    expected = oracle_matrix(c.oc, DEFAULT_GOALS, again)
    assert (expected != c.expected[0]).any()
    got = c.cm.actions_acceptance(DEFAULT_GOALS, again)
    assert (got == expected).all()


# ------------------------------------------------------------------------------------------------ 7. shared hosts
@pytest.mark.gpu
def test_gpu_shared_hosts_match_oracle(gpu_lib, oracle_lib):
    """Brokers that share a host: the CPU and NW goals test the host's load against the host's capacity (the hostCap
    branch of the predicates). Every legal replica move, leadership move and swap between the 6 brokers."""
    from test_hosts import HOST_GOALS, SHARED, _model

    flat = _model(SHARED)
    c = ChainCase(gpu_lib, flat.desc, flat)
    c.optimize(HOST_GOALS, ccmi.BalancingConstraint())
    cm, oc, pl = c.cm, c.oc, c.placement()
    P = flat.desc.num_partitions
    acts = []
    for p in range(P):
        for src in pl.brokers(p):
            acts += [(MOVE, p, src, dst, -1, -1, -1) for dst in range(6) if dst not in pl.brokers(p)]
        acts += [(LEADERSHIP, p, pl.leaders[p], dst, -1, -1, -1) for dst in pl.brokers(p) if dst != pl.leaders[p]]
    for p in range(P):
        for q in range(p + 1, P, 5):
            acts += [(SWAP, p, sb, db, q, -1, -1) for sb in pl.brokers(p) for db in pl.brokers(q)
                     if sb != db and db not in pl.brokers(p) and sb not in pl.brokers(q)]
    expected = oracle_matrix(oc, HOST_GOALS, acts)
    assert (expected == ACCEPT).any() and (expected == REPLICA_REJECT).any()
    got = cm.actions_acceptance(HOST_GOALS, acts)
    assert (got == expected).all()
