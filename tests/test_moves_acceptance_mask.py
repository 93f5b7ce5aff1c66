"""ccmi_moves_acceptance_mask: for a batch of move / leadership sources, the destination brokers that are legit and that
every optimized goal ACCEPTs, one bit per broker, computed on the device (kernels/accept_mask.hip).

The reference of every bit is the oracle: one OracleCluster.action_acceptance_by_goal per legit cell, on an oracle
cluster that ran the same chain (the action logs are asserted equal first). Legitimacy (GoalUtils.legitMove) is
computed in numpy from the oracle's replica_distribution / leader_distribution and the desc. Every comparison is exact.
"""
import numpy as np
import pytest

import ccmi
from acceptance_support import (CAPACITY_GOALS, CAPACITY_MIXED, CAPACITY_THRESHOLDS, DEFAULT_GOALS, LEADERSHIP, MOVE,
                                SEED, SWAP, ChainCase, directed_capacity_actions, props, run_in_fresh_process, status_of)
from parity import constraint

PER_TYPE = 150
# goals that both set and clear legit bits of the sample at 130 brokers (checked on the oracle's data)
MIXED_FOR_MOVES = ["RackAwareGoal", "ReplicaDistributionGoal", "DiskUsageDistributionGoal",
                   "NetworkInboundUsageDistributionGoal", "NetworkOutboundUsageDistributionGoal",
                   "CpuUsageDistributionGoal", "TopicReplicaDistributionGoal", "LeaderReplicaDistributionGoal",
                   "LeaderBytesInDistributionGoal"]
MIXED_FOR_LEADERSHIP = ["NetworkOutboundUsageDistributionGoal", "CpuUsageDistributionGoal",
                        "LeaderReplicaDistributionGoal", "LeaderBytesInDistributionGoal"]


# ------------------------------------------------------------------------------------------------ the reference
def legit_moves(pl, sources):
    """GoalUtils.legitMove for every (source, broker) cell, the source broker itself excluded."""
    out = np.zeros((len(sources), pl.B), dtype=bool)
    for i, (typ, p, src) in enumerate(sources):
        if typ == MOVE:
            out[i] = ~pl.hosts[p] & ~pl.ineligible[p]
        elif pl.leaders[p] == src:
            out[i] = pl.hosts[p]
        out[i, src] = False
    return out


def sample_sources(pl, rs, per_type):
    """per_type move sources (a random partition, then the broker of a random replica of it) and leadership sources (a
    random partition, then its leader), interleaved."""
    out = []
    for _ in range(per_type):
        p = int(rs.randint(pl.P))
        brokers = pl.brokers(p)
        out.append((MOVE, p, brokers[int(rs.randint(len(brokers)))]))
        p = int(rs.randint(pl.P))
        out.append((LEADERSHIP, p, pl.leaders[p]))
    return out


def oracle_accepts(oc, goals, sources, legit):
    """[n, B, G] bool: the oracle's ACCEPT of every goal for every legit cell (False elsewhere)."""
    out = np.zeros(legit.shape + (len(goals),), dtype=bool)
    for i, b in np.argwhere(legit):
        typ, p, src = sources[i]
        for g, name in enumerate(goals):
            out[i, b, g] = oc.action_acceptance_by_goal(name, typ, p, src, int(b)) == "ACCEPT"
    return out


def expected_mask(legit, accepts, columns):
    return legit & accepts[:, :, list(columns)].all(axis=2)


def assert_same(got, want, sources, what=""):
    assert got.dtype == bool and got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, [(sources[i], int(b), bool(got[i, b]), bool(want[i, b])) for i, b in bad[:10]])


class Case(ChainCase):
    """A product session and an oracle cluster after the same chain, a sample of sources and the oracle's verdicts."""

    def __init__(self, lib, cluster_props, goals=DEFAULT_GOALS, bc=None, sources=None):
        buf = ccmi.RandomCluster.generate(lib, **cluster_props)
        super().__init__(lib, buf.desc, buf)
        self.goals = list(goals)
        self.optimize(self.goals, bc or constraint(1.05, max_replicas=3000))
        self.pl = self.placement()
        self.sources = sources(self) if sources else sample_sources(self.pl, np.random.RandomState(SEED), PER_TYPE)
        self.types = np.array([s[0] for s in self.sources])
        self.legit = legit_moves(self.pl, self.sources)
        self.accepts = oracle_accepts(self.oc, self.goals, self.sources, self.legit)
        self.all_goals = expected_mask(self.legit, self.accepts, range(len(self.goals)))
        for a in (self.legit, self.accepts, self.all_goals):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def cases(gpu_lib, oracle_lib):
    made = {}

    def get(num_brokers):
        if num_brokers not in made:
            made[num_brokers] = Case(gpu_lib, props(num_brokers))
        return made[num_brokers]
    return get


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.gpu
def test_gpu_masks_match_oracle_at_130_brokers(cases):
    c = cases(130)
    n, B, G = len(c.sources), 130, len(DEFAULT_GOALS)
    moves, leads = c.types == MOVE, c.types == LEADERSHIP
    # the sample exercises something, asserted on the oracle's data alone
    for rows, names in ((moves, MIXED_FOR_MOVES), (leads, MIXED_FOR_LEADERSHIP)):
        for name in names:
            col = c.accepts[rows][:, :, DEFAULT_GOALS.index(name)]
            assert col[c.legit[rows]].any() and (~col[c.legit[rows]]).any(), name
    words = [slice(0, 64), slice(64, 128), slice(128, 130)]
    for w in words:
        assert c.all_goals[moves][:, w].any() and (c.legit[moves][:, w] & ~c.all_goals[moves][:, w]).any()
    assert c.all_goals[leads].any(axis=1).sum() >= 1
    print(f"set bits per word of the 16-goal move masks {[int(c.all_goals[moves][:, w].sum()) for w in words]}; "
          f"leadership rows with a set bit {int(c.all_goals[leads].any(axis=1).sum())}")

    c.cm.reset_perf()
    c.cm.set_kernel_timing(True)
    got = c.cm.moves_acceptance_mask(DEFAULT_GOALS, c.sources)
    c.cm.set_kernel_timing(False)
    p = c.cm.perf()
    print(f"accept_launches {p.accept_launches} accept_cells {p.accept_cells} accept_kernel_ms {p.accept_kernel_ms:.3f}")
    assert_same(got, c.all_goals, c.sources, "16 goals")
    assert p.accept_launches > 0
    assert p.accept_cells == n * B * G
    assert p.accept_kernel_ms > 0
    for g, name in enumerate(DEFAULT_GOALS):
        assert_same(c.cm.moves_acceptance_mask([name], c.sources), expected_mask(c.legit, c.accepts, [g]), c.sources, name)
    assert_same(c.cm.moves_acceptance_mask([], c.sources), c.legit, c.sources, "no goals: the legit matrix")


# ------------------------------------------------------------------------------------------------ 2. shape edges
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 5, 65])
@pytest.mark.parametrize("num_brokers", [20, 64, 130])
def test_gpu_shapes_and_tail_bits(cases, num_brokers, n):
    """Prefixes of the interleaved sample at two full words plus a 2-bit tail, exactly one word, and one partial word."""
    c = cases(num_brokers)
    src = c.sources[:n]
    got = c.cm.moves_acceptance_mask(DEFAULT_GOALS, src)
    assert got.dtype == bool and got.shape == (n, num_brokers)
    assert_same(got, c.all_goals[:n], src)
    W = (num_brokers + 63) // 64
    packed = c.cm.moves_acceptance_mask(DEFAULT_GOALS, src, packed=True)
    assert packed.dtype == np.uint64 and packed.shape == (n, W)
    bits = np.array([[(int(packed[i, b >> 6]) >> (b & 63)) & 1 for b in range(W * 64)] for i in range(n)],
                    dtype=bool).reshape(n, W * 64)
    assert not bits[:, num_brokers:].any()
    assert (bits[:, :num_brokers] == got).all()
    as_array = np.array(src, dtype=np.int32).reshape(n, 3)
    assert (c.cm.moves_acceptance_mask(DEFAULT_GOALS, as_array) == got).all()
    assert (c.cm.moves_acceptance_mask(DEFAULT_GOALS, as_array, packed=True) == packed).all()


# ------------------------------------------------------------------------------------------------ 3. many goals
@pytest.mark.gpu
def test_gpu_more_goals_than_one_program(cases):
    """More goals than one device program holds (kMaxGoals = 20): several programs whose masks are ANDed."""
    c = cases(130)
    names = DEFAULT_GOALS + DEFAULT_GOALS[::-1] + DEFAULT_GOALS[:9]  # 41 names: programs of 20, 20 and 1
    cols = [DEFAULT_GOALS.index(g) for g in names]
    c.cm.reset_perf()
    got = c.cm.moves_acceptance_mask(names, c.sources)
    assert_same(got, expected_mask(c.legit, c.accepts, cols), c.sources)
    p = c.cm.perf()
    assert p.accept_launches == 3 and p.accept_cells == len(c.sources) * 130 * 41
    # a subset that spans two programs and leaves goals out: the AND of exactly those columns
    some = (DEFAULT_GOALS[1:12] * 2)[:21]
    assert_same(c.cm.moves_acceptance_mask(some, c.sources),
                expected_mask(c.legit, c.accepts, [DEFAULT_GOALS.index(g) for g in some]), c.sources)


# ------------------------------------------------------------------------------------------------ 4. chunk boundary
@pytest.mark.gpu
def test_gpu_chunk_boundary_matches_oracle(cases, gpu_lib, tmp_path):
    """CCMI_MASK_CHUNK_SOURCES is read at session create: a fresh process with 4 answers n = 10 in 3 launches."""
    c = cases(130)
    mask, launches = run_in_fresh_process(gpu_lib, tmp_path, props(130), dict(CCMI_MASK_CHUNK_SOURCES="4"), c.sources[:10],
                                          "cm.moves_acceptance_mask(goals, [tuple(a) for a in sample])")
    assert launches == 3
    assert_same(np.array(mask, dtype=bool), c.all_goals[:10], c.sources[:10])


# ------------------------------------------------------------------------------------------------ 5. agreement with K9
@pytest.mark.gpu
def test_gpu_mask_agrees_with_actions_acceptance(cases):
    c = cases(130)
    idx = list(np.flatnonzero(c.types == MOVE)[:8]) + list(np.flatnonzero(c.types == LEADERSHIP)[:8])
    src = [c.sources[i] for i in idx]
    got = c.cm.moves_acceptance_mask(DEFAULT_GOALS, src)
    legit = c.legit[idx]
    assert not got[~legit].any()
    assert legit[:8].any() and legit[8:].any()
    for i, b in np.argwhere(legit):
        typ, p, sb = src[i]
        verdicts = c.cm.actions_acceptance(DEFAULT_GOALS, [(typ, p, sb, int(b), -1, -1, -1)])
        assert bool(got[i, b]) == bool((verdicts == 0).all()), (src[i], int(b))


# ------------------------------------------------------------------------------------------------ 6. state tracking
@pytest.mark.gpu
def test_gpu_masks_after_session_apply_match_oracle(gpu_lib, oracle_lib):
    """Rows ccmi_session_apply made dirty reach the device before the launch: after about 20 external actions (accepted
    cells of the first masks, one per partition) the masks of sources on the touched partitions and brokers follow the
    oracle, which applied the same actions."""
    c = Case(gpu_lib, props(130))
    assert_same(c.cm.moves_acceptance_mask(DEFAULT_GOALS, c.sources), c.all_goals, c.sources)
    external, touched = [], set()
    for want_type, limit in ((LEADERSHIP, 3), (MOVE, 20)):
        for i, (typ, p, src) in enumerate(c.sources):
            if typ == want_type and p not in touched and c.all_goals[i].any() and len(external) < limit:
                external.append((typ, p, src, int(np.flatnonzero(c.all_goals[i])[0]), -1, -1, -1))
                touched.add(p)
    assert {a[0] for a in external} == {MOVE, LEADERSHIP} and len(external) == 20
    assert c.cm.apply(external) == len(external)
    c.oc.apply(external)
    pl = c.placement()
    # both ends of every external action, for both source types, then a fresh sample of the new placement
    again = []
    for typ, p, src, dst, *_ in external:
        again += [(MOVE, p, dst), (LEADERSHIP, p, dst), (LEADERSHIP, p, pl.leaders[p])]
        again += [(t, p, src) for t in (MOVE, LEADERSHIP) if src in pl.brokers(p)]
    brokers = {a[2] for a in external} | {a[3] for a in external}
    fresh = sample_sources(pl, np.random.RandomState(SEED + 1), 60)
    again += fresh
    assert any(s[2] in brokers for s in fresh)
    legit = legit_moves(pl, again)
    accepts = oracle_accepts(c.oc, DEFAULT_GOALS, again, legit)
    # the moved replicas' old brokers are legit destinations again: the reference changed with the actions
    for typ, p, src, dst, *_ in external:
        if typ == MOVE:
            assert legit[again.index((MOVE, p, dst)), src] and not c.pl.hosts[p, dst] and pl.hosts[p, dst]
    assert_same(c.cm.moves_acceptance_mask([], again), legit, again, "legit after apply")
    assert_same(c.cm.moves_acceptance_mask(DEFAULT_GOALS, again), expected_mask(legit, accepts, range(16)), again,
                "16 goals after apply")


# ------------------------------------------------------------------------------------------------ 7. ineligible brokers
@pytest.mark.gpu
def test_gpu_ineligible_brokers_are_cleared(gpu_lib, oracle_lib):
    """A BAD_DISKS broker that held an offline replica of a partition stays closed to it (Partition.
    canAssignReplicaToBroker): the bit is clear although the broker no longer hosts the partition."""
    def sources(case):
        pairs = np.argwhere(case.pl.ineligible)
        out = [(MOVE, int(p), b) for p, _ in pairs for b in case.pl.brokers(int(p))]
        return out + sample_sources(case.pl, np.random.RandomState(SEED), 40)

    c = Case(gpu_lib, props(20, num_brokers_with_bad_disk=3), sources=sources)
    pairs = [(int(p), int(b)) for p, b in np.argwhere(c.pl.ineligible)]
    assert pairs
    assert not any(c.pl.hosts[p, b] for p, b in pairs)
    legit = c.cm.moves_acceptance_mask([], c.sources)
    assert_same(legit, c.legit, c.sources, "legit")
    checked = 0
    for i, (typ, p, src) in enumerate(c.sources):
        for q, b in pairs:
            if typ == MOVE and p == q:
                assert not legit[i, b] and not c.pl.hosts[p, b]
                checked += 1
    assert checked >= len(pairs)
    assert_same(c.cm.moves_acceptance_mask(DEFAULT_GOALS, c.sources), c.all_goals, c.sources, "16 goals")


# ------------------------------------------------------------------------------------------------ 8. capacity goals
@pytest.mark.gpu
def test_gpu_capacity_goals_directed_sources(gpu_lib, oracle_lib):
    def sources(case):
        acts = directed_capacity_actions(case.desc, case.pl, case.oc)
        return sorted({(a[0], a[1], a[2]) for a in acts})

    bc = constraint(1.05, max_replicas=3000)
    bc.capacity_threshold = CAPACITY_THRESHOLDS
    c = Case(gpu_lib, props(20), goals=CAPACITY_GOALS, bc=bc, sources=sources)
    assert {s[0] for s in c.sources} == {MOVE, LEADERSHIP}
    for name in CAPACITY_MIXED:
        g = CAPACITY_GOALS.index(name)
        want = expected_mask(c.legit, c.accepts, [g])
        assert want.any() and (c.legit & ~want).any(), name
        assert_same(c.cm.moves_acceptance_mask([name], c.sources), want, c.sources, name)
    assert_same(c.cm.moves_acceptance_mask(CAPACITY_GOALS, c.sources), c.all_goals, c.sources, "all capacity goals")


# ------------------------------------------------------------------------------------------------ 9. errors
@pytest.mark.gpu
def test_gpu_errors_leave_the_session_untouched(cases):
    c = cases(20)
    cm, src = c.cm, c.sources[:9]
    logged = len(cm.actions())
    # a kind the session has not optimized; an intra-broker kind (16) is refused as such, optimized or not
    assert status_of(lambda: cm.moves_acceptance_mask(["RackAwareGoal", "RackAwareDistributionGoal"], src)) == \
        (ccmi.IllegalArgumentException, -1)
    assert ccmi.GOAL_KINDS["IntraBrokerDiskCapacityGoal"] == 16
    assert status_of(lambda: cm.moves_acceptance_mask(["RackAwareGoal", "IntraBrokerDiskCapacityGoal"], src)) == \
        (ccmi.UnsupportedOperationException, -1)
    assert status_of(lambda: cm.moves_acceptance_mask(["IntraBrokerDiskUsageDistributionGoal"], [])) == \
        (ccmi.UnsupportedOperationException, -1)
    # a swap is not a move source, at index 2 of 3
    assert status_of(lambda: cm.moves_acceptance_mask(DEFAULT_GOALS, src[:2] + [(SWAP,) + src[2][1:]])) == \
        (ccmi.IllegalArgumentException, 2)
    # indices outside the model are refused before the device sees them
    assert status_of(lambda: cm.moves_acceptance_mask(DEFAULT_GOALS, [src[0], (MOVE, 10 ** 6, 0)])) == \
        (ccmi.IllegalArgumentException, 1)
    assert status_of(lambda: cm.moves_acceptance_mask(DEFAULT_GOALS, [(MOVE, -1, 0)])) == \
        (ccmi.IllegalArgumentException, 0)
    assert status_of(lambda: cm.moves_acceptance_mask([], [(MOVE, src[0][1], 20)])) == \
        (ccmi.IllegalArgumentException, 0)
    # the source broker does not host the partition, at index 5 of 9
    p = src[5][1]
    stranger = next(b for b in range(20) if not c.pl.hosts[p, b])
    assert status_of(lambda: cm.moves_acceptance_mask(DEFAULT_GOALS, src[:5] + [(MOVE, p, stranger)] + src[6:])) == \
        (ccmi.IllegalArgumentException, 5)
    # a leadership source whose replica is not the leader: no legit destination, no error
    p = next(q for q in range(c.pl.P) if len(c.pl.brokers(q)) > 1)
    follower = next(b for b in c.pl.brokers(p) if b != c.pl.leaders[p])
    for goals in (DEFAULT_GOALS, []):
        rows = cm.moves_acceptance_mask(goals, [(LEADERSHIP, p, follower), (LEADERSHIP, p, c.pl.leaders[p])])
        assert not rows[0].any()
        assert goals or (rows[1] == (c.pl.hosts[p] & (np.arange(20) != c.pl.leaders[p]))).all()
    # the session is as it was and still answers
    assert len(cm.actions()) == logged
    assert_same(cm.moves_acceptance_mask(DEFAULT_GOALS, src), c.all_goals[:9], src)
    acts = [(typ, q, sb, int(np.flatnonzero(c.legit[i])[0]), -1, -1, -1)
            for i, (typ, q, sb) in enumerate(src) if c.legit[i].any()]
    assert acts
    want = np.array([[ccmi.ACCEPTANCE.index(c.oc.action_acceptance_by_goal(g, *a[:4])) for g in DEFAULT_GOALS]
                     for a in acts], dtype=np.int8)
    assert (cm.actions_acceptance(DEFAULT_GOALS, acts) == want).all()
