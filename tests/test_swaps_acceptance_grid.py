"""ccmi_swaps_acceptance_grid: for n source replicas against m candidate replicas, one code per pair — what the loop body
of AbstractGoal.maybeApplySwapAction decides before the goal's own selfSatisfied — computed on the device
(kernels/accept_swap.hip).

The reference of every cell is the oracle, on an oracle cluster that ran the same chain (the action logs are asserted
equal first). The two legitimacy codes (3, 4: GoalUtils.legitMove of the source to the candidate's broker, then of the
candidate to the source's broker) are computed in numpy from the oracle's replica_distribution and the desc. For the
cells legit both ways the full [n, m, G] matrix of OracleCluster.action_acceptance_by_goal is kept, and the expected
code of any goal list is the first non-zero verdict along that list. Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

import ccmi
from acceptance_support import (ACCEPT, CANDIDATE_NOT_LEGIT, DEFAULT_GOALS, REPLICA_REJECT, SEED, SOURCE_NOT_LEGIT, SWAP,
                                ChainCase, Placement, props, run_in_fresh_process, status_of)
from parity import constraint


# ------------------------------------------------------------------------------------------------ the reference
def legit_swaps(pl, sources, candidates):
    """[n, m] int8: 3 where legitMove(source, candidate's broker) fails, else 4 where legitMove(candidate, source's
    broker) fails, else 0."""
    src = np.array(sources, dtype=np.int64).reshape(-1, 2)
    cand = np.array(candidates, dtype=np.int64).reshape(-1, 2)
    closed = pl.hosts | pl.ineligible  # [p, b]: b is no destination of a replica of p
    first = closed[src[:, 0][:, None], cand[:, 1][None, :]]
    second = closed[cand[:, 0][None, :], src[:, 1][:, None]]
    return np.where(first, SOURCE_NOT_LEGIT, np.where(second, CANDIDATE_NOT_LEGIT, ACCEPT)).astype(np.int8)


def oracle_verdicts(oc, goals, sources, candidates, legit):
    """[n, m, G] int8: the oracle's verdict of every goal for the swap of every cell legit both ways (0 elsewhere)."""
    out = np.zeros(legit.shape + (len(goals),), dtype=np.int8)
    kinds = [ccmi.GOAL_KINDS[g] for g in goals]
    call, h = oc.L.oc_action_acceptance_by_kind, oc.h
    for i, j in np.argwhere(legit == ACCEPT):
        (p, sb), (q, db) = sources[i], candidates[j]
        a = C.byref(ccmi.ActionStruct(SWAP, p, sb, db, q, -1, -1))
        for g, kind in enumerate(kinds):
            v = call(h, kind, a)
            assert v >= 0, (goals[g], sources[i], candidates[j])
            out[i, j, g] = v
    return out


def expected_codes(legit, verdicts, columns):
    """The legitimacy code, else the first non-zero verdict along `columns`, else 0."""
    columns = list(columns)
    if not columns:
        return legit.copy()
    v = verdicts[:, :, columns]
    first = (v != 0).argmax(axis=2)  # 0 when every verdict is 0, and then the verdict taken is 0
    code = np.take_along_axis(v, first[:, :, None], axis=2)[:, :, 0]
    return np.where(legit != ACCEPT, legit, code).astype(np.int8)


def assert_same(got, want, sources, candidates, what=""):
    assert got.dtype == np.int8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad),
                           [(sources[i], candidates[j], int(got[i, j]), int(want[i, j])) for i, j in bad[:10]])


def sample_replicas(pl, rs, directed=False):
    """Sources: 8 random replicas of each of 3 random brokers. Candidates: every replica of 3 other random brokers;
    `directed` adds every replica of a broker that hosts the first source's partition (code 3 for that source)."""
    brokers = [int(b) for b in rs.permutation(pl.B)]
    sources = []
    for b in brokers[:3]:
        on = pl.replicas_on(b)
        sources += [on[k] for k in rs.choice(len(on), 8, replace=False)]
    candidates = [r for b in brokers[3:6] for r in pl.replicas_on(b)]
    if directed:
        p, sb = sources[0]
        others = [b for b in pl.brokers(p) if b != sb]
        candidates += pl.replicas_on(others[0] if others else sb)
    return sources, candidates


class Case(ChainCase):
    """A product session and an oracle cluster after the same chain, a grid of replicas and the oracle's verdicts."""

    def __init__(self, lib, cluster_props, goals=DEFAULT_GOALS, bc=None, replicas=None, directed=False):
        buf = ccmi.RandomCluster.generate(lib, **cluster_props)
        super().__init__(lib, buf.desc, buf)
        self.goals = list(goals)
        self.optimize(self.goals, bc or constraint(1.05, max_replicas=3000))
        self.pl = self.placement()
        self.sources, self.candidates = (replicas(self) if replicas else
                                         sample_replicas(self.pl, np.random.RandomState(SEED), directed))
        self.n, self.m = len(self.sources), len(self.candidates)
        self.legit = legit_swaps(self.pl, self.sources, self.candidates)
        self.verdicts = oracle_verdicts(self.oc, self.goals, self.sources, self.candidates, self.legit)
        self.all_goals = self.expected(self.goals)
        for a in (self.legit, self.verdicts, self.all_goals):
            a.setflags(write=False)

    def expected(self, names):
        return expected_codes(self.legit, self.verdicts, [self.goals.index(g) for g in names])


@pytest.fixture(scope="module")
def cases(gpu_lib, oracle_lib):
    made = {}

    def get(num_brokers):
        if num_brokers not in made:
            made[num_brokers] = Case(gpu_lib, props(num_brokers), directed=num_brokers == 130)
        return made[num_brokers]
    return get


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.gpu
def test_gpu_grid_matches_oracle_at_20_brokers(cases):
    c = cases(20)
    n, m, G = c.n, c.m, len(DEFAULT_GOALS)
    assert n == 24 and m > 5 * 64
    # the sample exercises something, asserted on the oracle's data alone
    counts = np.bincount(c.all_goals.ravel(), minlength=5)
    assert (counts > 0).all(), counts
    for block in range(5):  # every one of the first five wavefronts of a row stores a mix
        assert len(np.unique(c.all_goals[:, 64 * block:64 * block + 64])) >= 3
    reverse = c.expected(DEFAULT_GOALS[::-1])
    changed = int((reverse != c.all_goals).sum())
    assert changed > 0
    both = [g for k, g in enumerate(DEFAULT_GOALS)
            if (c.verdicts[:, :, k][c.legit == ACCEPT] == 0).any() and (c.verdicts[:, :, k] != 0).any()]
    print(f"n {n} m {m}: code counts {counts.tolist()}, {changed} cells change under the reversed goal order, "
          f"{len(both)} goals both accept and reject")

    c.cm.reset_perf()
    c.cm.set_kernel_timing(True)
    got = c.cm.swaps_acceptance_grid(DEFAULT_GOALS, c.sources, c.candidates)
    c.cm.set_kernel_timing(False)
    p = c.cm.perf()
    print(f"accept_launches {p.accept_launches} accept_cells {p.accept_cells} accept_kernel_ms {p.accept_kernel_ms:.3f}")
    assert_same(got, c.all_goals, c.sources, c.candidates, "16 goals")
    assert p.accept_launches > 0
    assert p.accept_cells == n * m * G
    assert p.accept_kernel_ms > 0
    for name in DEFAULT_GOALS:
        assert_same(c.cm.swaps_acceptance_grid([name], c.sources, c.candidates), c.expected([name]), c.sources,
                    c.candidates, name)
    assert set(np.unique(c.legit)) == {ACCEPT, SOURCE_NOT_LEGIT, CANDIDATE_NOT_LEGIT}
    assert_same(c.cm.swaps_acceptance_grid([], c.sources, c.candidates), c.legit, c.sources, c.candidates,
                "no goals: the legitimacy grid")
    assert_same(c.cm.swaps_acceptance_grid(DEFAULT_GOALS[::-1], c.sources, c.candidates), reverse, c.sources,
                c.candidates, "reversed goal order")


# ------------------------------------------------------------------------------------------------ 2. shape edges
@pytest.mark.gpu
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_gpu_shapes_and_tail_lanes(cases, n, m):
    """Candidate prefixes of the sample: no block, one lane, one lane short of a block, a block, a block and one lane,
    two blocks and two lanes."""
    c = cases(20)
    src, cand = c.sources[:n], c.candidates[:m]
    got = c.cm.swaps_acceptance_grid(DEFAULT_GOALS, src, cand)
    assert got.dtype == np.int8 and got.shape == (n, m)
    assert_same(got, c.all_goals[:n, :m], src, cand)
    as_arrays = (np.array(src, dtype=np.int32).reshape(n, 2), np.array(cand, dtype=np.int32).reshape(m, 2))
    again = c.cm.swaps_acceptance_grid(DEFAULT_GOALS, *as_arrays)
    assert again.dtype == np.int8 and again.shape == (n, m) and (again == got).all()


@pytest.mark.gpu
def test_gpu_grid_matches_oracle_at_130_brokers(cases):
    """A wider cluster, whose sampled candidate brokers host no source's partition: the candidates end with the
    replicas of a broker that hosts the first source's partition, every one of them code 3 for that source."""
    c = cases(130)
    p, _ = c.sources[0]
    directed = [j for j, (_, db) in enumerate(c.candidates) if c.pl.hosts[p, db]]
    assert directed and (c.all_goals[0, directed] == SOURCE_NOT_LEGIT).all()
    assert c.m >= 142 and c.m % 64 != 0
    assert_same(c.cm.swaps_acceptance_grid(DEFAULT_GOALS, c.sources, c.candidates), c.all_goals, c.sources, c.candidates)
    assert_same(c.cm.swaps_acceptance_grid([], c.sources, c.candidates), c.legit, c.sources, c.candidates, "no goals")


# ------------------------------------------------------------------------------------------------ 3. many goals
@pytest.mark.gpu
def test_gpu_more_goals_than_one_program(cases):
    """More goals than one device program holds (kMaxGoals = 20): several programs; a cell keeps its code unless it is
    still 0, and then takes the next program's."""
    c = cases(20)
    names = DEFAULT_GOALS + DEFAULT_GOALS[::-1] + DEFAULT_GOALS[:9]  # 41 names: programs of 20, 20 and 1
    c.cm.reset_perf()
    got = c.cm.swaps_acceptance_grid(names, c.sources, c.candidates)
    assert_same(got, c.expected(names), c.sources, c.candidates)
    p = c.cm.perf()
    assert p.accept_launches == 3 and p.accept_cells == c.n * c.m * 41
    # 21 names over two programs: the first program's 20 goals accept cells that the 21st, alone in the second, rejects
    k = next(k for k in range(16)
             if ((np.delete(c.verdicts, k, axis=2) == 0).all(axis=2) & (c.verdicts[:, :, k] != 0)).any())
    rest = [g for i, g in enumerate(DEFAULT_GOALS) if i != k]
    some = (rest * 2)[:20] + [DEFAULT_GOALS[k]]
    want = c.expected(some)
    assert ((c.expected(some[:20]) == ACCEPT) & (want != ACCEPT)).any()
    assert_same(c.cm.swaps_acceptance_grid(some, c.sources, c.candidates), want, c.sources, c.candidates, "21 names")


# ------------------------------------------------------------------------------------------------ 4. chunk boundary
@pytest.mark.gpu
def test_gpu_chunk_boundary_matches_oracle(cases, gpu_lib, tmp_path):
    """CCMI_SWAP_CHUNK_CELLS is read at session create: a fresh process with 512 and m = 142 (a row of 192 bytes on the
    device, 2 sources per launch) answers n = 5 in 3 launches."""
    c = cases(130)
    src, cand = c.sources[:5], c.candidates[:142]
    codes, launches = run_in_fresh_process(gpu_lib, tmp_path, props(130), dict(CCMI_SWAP_CHUNK_CELLS="512"),
                                           dict(sources=src, candidates=cand),
                                           'cm.swaps_acceptance_grid(goals, sample["sources"], sample["candidates"])')
    assert launches == 3
    assert_same(np.array(codes, dtype=np.int8).reshape(5, 142), c.all_goals[:5, :142], src, cand)


# ------------------------------------------------------------------------------------------------ 5. agreement with K9
@pytest.mark.gpu
def test_gpu_grid_agrees_with_actions_acceptance(cases):
    c = cases(130)
    src, cand = c.sources[:4], c.candidates[:142]
    got = c.cm.swaps_acceptance_grid(DEFAULT_GOALS, src, cand)
    cells = np.argwhere(c.legit[:4, :142] == ACCEPT)
    assert len(cells) > 100
    assert ((got == SOURCE_NOT_LEGIT) | (got == CANDIDATE_NOT_LEGIT) == (c.legit[:4, :142] != ACCEPT)).all()
    acts = [(SWAP, src[i][0], src[i][1], cand[j][1], cand[j][0], -1, -1) for i, j in cells]
    rows = c.cm.actions_acceptance(DEFAULT_GOALS, acts)
    first = np.take_along_axis(rows, (rows != 0).argmax(axis=1)[:, None], axis=1)[:, 0]
    assert (got[cells[:, 0], cells[:, 1]] == first).all()


# ------------------------------------------------------------------------------------------------ 6. state tracking
@pytest.mark.gpu
def test_gpu_grid_after_session_apply_matches_oracle(gpu_lib, oracle_lib):
    """Rows ccmi_session_apply made dirty reach the device before the launch: after about 10 external swaps (code-0
    cells of the first grid, on distinct partitions) the grid of the swapped replicas, of the replicas of the touched
    brokers and of a fresh sample follows the oracle, which applied the same swaps."""
    c = Case(gpu_lib, props(20))
    assert_same(c.cm.swaps_acceptance_grid(DEFAULT_GOALS, c.sources, c.candidates), c.all_goals, c.sources, c.candidates)
    external, touched = [], set()
    for i, j in np.argwhere(c.all_goals == ACCEPT):
        (p, sb), (q, db) = c.sources[i], c.candidates[j]
        if p not in touched and q not in touched and len(external) < 10:
            external.append((SWAP, p, sb, db, q, -1, -1))
            touched |= {p, q}
    assert len(external) >= 5
    assert c.cm.apply(external) == len(external)
    c.oc.apply(external)
    pl = c.placement()
    fresh_src, fresh_cand = sample_replicas(pl, np.random.RandomState(SEED + 1))
    # both replicas of every swap where they are now, as sources and as candidates, other replicas of the brokers whose
    # loads the swaps changed, then a fresh sample
    moved = [r for _, p, sb, db, q, *_ in external for r in ((p, db), (q, sb))]
    brokers = sorted({a[2] for a in external} | {a[3] for a in external})
    assert len(brokers) >= 2
    sources = moved + [pl.replicas_on(b)[0] for b in brokers] + fresh_src[:8]
    candidates = moved + [r for b in brokers for r in pl.replicas_on(b)[:30]] + fresh_cand[:200]
    legit = legit_swaps(pl, sources, candidates)
    verdicts = oracle_verdicts(c.oc, DEFAULT_GOALS, sources, candidates, legit)
    # a swapped replica's old broker no longer hosts its partition: the replica that took its place there is no code-3
    # candidate for it any more, and the reference changed with the swaps
    for _, p, sb, db, q, *_ in external:
        i, j = sources.index((p, db)), candidates.index((q, sb))
        assert c.pl.hosts[p, sb] and not pl.hosts[p, sb] and legit[i, j] != SOURCE_NOT_LEGIT
    assert_same(c.cm.swaps_acceptance_grid([], sources, candidates), legit, sources, candidates, "legit after apply")
    assert_same(c.cm.swaps_acceptance_grid(DEFAULT_GOALS, sources, candidates),
                expected_codes(legit, verdicts, range(16)), sources, candidates, "16 goals after apply")


# ------------------------------------------------------------------------------------------------ 7. ineligible brokers
@pytest.mark.gpu
def test_gpu_ineligible_brokers_are_not_legit(gpu_lib, oracle_lib):
    """A BAD_DISKS broker that held an offline replica of a partition stays closed to it (Partition.
    canAssignReplicaToBroker) although it no longer hosts the partition: a source of the partition against a candidate on
    that broker is 3, a candidate of the partition against a source on that broker 4 (unless 3 comes first)."""
    def replicas(case):
        pairs = [(int(p), int(b)) for p, b in np.argwhere(case.pl.ineligible)]
        of_partitions = [(p, sb) for p, _ in pairs for sb in case.pl.brokers(p)]
        on_brokers = [r for b in sorted({b for _, b in pairs}) for r in case.pl.replicas_on(b)[:12]]
        more_src, more_cand = sample_replicas(case.pl, np.random.RandomState(SEED))
        return of_partitions + on_brokers + more_src[:4], of_partitions + on_brokers + more_cand[:100]

    c = Case(gpu_lib, props(20, num_brokers_with_bad_disk=3), replicas=replicas)
    pairs = [(int(p), int(b)) for p, b in np.argwhere(c.pl.ineligible)]
    assert pairs
    assert not any(c.pl.hosts[p, b] for p, b in pairs)
    threes = fours = 0
    for p, b in pairs:
        for i, (sp, sb) in enumerate(c.sources):
            for j, (cp, cb) in enumerate(c.candidates):
                if sp == p and cb == b:
                    assert c.legit[i, j] == SOURCE_NOT_LEGIT
                    threes += 1
                elif cp == p and sb == b:
                    assert c.legit[i, j] in (SOURCE_NOT_LEGIT, CANDIDATE_NOT_LEGIT)
                    fours += int(c.legit[i, j] == CANDIDATE_NOT_LEGIT)
    assert threes >= len(pairs) and fours >= 1
    assert_same(c.cm.swaps_acceptance_grid([], c.sources, c.candidates), c.legit, c.sources, c.candidates, "legit")
    assert_same(c.cm.swaps_acceptance_grid(DEFAULT_GOALS, c.sources, c.candidates), c.all_goals, c.sources, c.candidates,
                "16 goals")


# ------------------------------------------------------------------------------------------------ 8. shared hosts
@pytest.mark.gpu
def test_gpu_shared_hosts_match_oracle(gpu_lib, oracle_lib):
    """Brokers that share a host: the CPU and NW goals test the host's load against the host's capacity (the hostCap
    branch of the predicates). Every replica of the 6 brokers as source and as candidate."""
    from test_hosts import HOST_GOALS, SHARED, _model

    flat = _model(SHARED)
    c = ChainCase(gpu_lib, flat.desc, flat)
    c.optimize(HOST_GOALS, ccmi.BalancingConstraint())
    cm, oc, pl = c.cm, c.oc, c.placement()
    every = [r for b in range(pl.B) for r in pl.replicas_on(b)]
    legit = legit_swaps(pl, every, every)
    verdicts = oracle_verdicts(oc, HOST_GOALS, every, every, legit)
    want = expected_codes(legit, verdicts, range(len(HOST_GOALS)))
    assert (want == ACCEPT).any() and (want == REPLICA_REJECT).any()
    assert (np.diag(want) == SOURCE_NOT_LEGIT).all()  # a replica against itself
    assert_same(cm.swaps_acceptance_grid(HOST_GOALS, every, every), want, every, every)
    assert_same(cm.swaps_acceptance_grid([], every, every), legit, every, every, "no goals")


# ------------------------------------------------------------------------------------------------ 9. errors
@pytest.mark.gpu
def test_gpu_errors_leave_the_session_untouched(cases):
    c = cases(20)
    cm, src, cand = c.cm, c.sources[:4], c.candidates[:9]
    n = len(src)
    logged = len(cm.actions())
    # a kind the session has not optimized; an intra-broker kind (16, 17) is refused as such, optimized or not
    assert status_of(lambda: cm.swaps_acceptance_grid(["RackAwareGoal", "RackAwareDistributionGoal"], src, cand)) == \
        (ccmi.IllegalArgumentException, -1)
    assert status_of(lambda: cm.swaps_acceptance_grid(["RackAwareDistributionGoal"], [], [])) == \
        (ccmi.IllegalArgumentException, -1)
    assert ccmi.GOAL_KINDS["IntraBrokerDiskCapacityGoal"] == 16
    assert ccmi.GOAL_KINDS["IntraBrokerDiskUsageDistributionGoal"] == 17
    assert status_of(lambda: cm.swaps_acceptance_grid(["RackAwareGoal", "IntraBrokerDiskCapacityGoal"], src, cand)) == \
        (ccmi.UnsupportedOperationException, -1)
    assert status_of(lambda: cm.swaps_acceptance_grid(["IntraBrokerDiskUsageDistributionGoal"], [], [])) == \
        (ccmi.UnsupportedOperationException, -1)
    assert status_of(lambda: cm.swaps_acceptance_grid(["IntraBrokerDiskUsageDistributionGoal"], src, [])) == \
        (ccmi.UnsupportedOperationException, -1)
    # indices outside the model are refused before the device sees them: i for a source, n + j for a candidate
    assert status_of(lambda: cm.swaps_acceptance_grid(DEFAULT_GOALS, [src[0], (10 ** 6, 0)], cand)) == \
        (ccmi.IllegalArgumentException, 1)
    assert status_of(lambda: cm.swaps_acceptance_grid(DEFAULT_GOALS, [(-1, 0)], cand)) == \
        (ccmi.IllegalArgumentException, 0)
    assert status_of(lambda: cm.swaps_acceptance_grid([], [(src[0][0], 20)], cand)) == \
        (ccmi.IllegalArgumentException, 0)
    assert status_of(lambda: cm.swaps_acceptance_grid([], src, [cand[0], (cand[1][0], -1)])) == \
        (ccmi.IllegalArgumentException, n + 1)
    assert status_of(lambda: cm.swaps_acceptance_grid(DEFAULT_GOALS, src, cand[:3] + [(c.pl.P, 0)])) == \
        (ccmi.IllegalArgumentException, n + 3)
    # a broker that does not hold the partition: the source at index 2, the candidate at j = 5
    p = src[2][0]
    stranger = next(b for b in range(20) if not c.pl.hosts[p, b])
    assert status_of(lambda: cm.swaps_acceptance_grid(DEFAULT_GOALS, src[:2] + [(p, stranger)] + src[3:], cand)) == \
        (ccmi.IllegalArgumentException, 2)
    q = cand[5][0]
    stranger = next(b for b in range(20) if not c.pl.hosts[q, b])
    assert status_of(lambda: cm.swaps_acceptance_grid(DEFAULT_GOALS, src, cand[:5] + [(q, stranger)] + cand[6:])) == \
        (ccmi.IllegalArgumentException, n + 5)
    # both bad: the sources are checked first
    assert status_of(lambda: cm.swaps_acceptance_grid(DEFAULT_GOALS, src[:1] + [(-1, 0)], [(q, stranger)])) == \
        (ccmi.IllegalArgumentException, 1)
    # the session is as it was and still answers
    assert len(cm.actions()) == logged
    assert_same(cm.swaps_acceptance_grid(DEFAULT_GOALS, src, cand), c.all_goals[:4, :9], src, cand)
    assert_same(cm.swaps_acceptance_grid(DEFAULT_GOALS, c.sources, c.candidates), c.all_goals, c.sources, c.candidates)


@pytest.mark.gpu
def test_gpu_terminal_goal_is_a_state_error(gpu_lib):
    """KafkaAssignerDiskUsageDistributionGoal.actionAcceptance throws IllegalStateException: so does a grid that names
    it, except an empty one."""
    ka = ["KafkaAssignerEvenRackAwareGoal", "KafkaAssignerDiskUsageDistributionGoal"]
    buf = ccmi.RandomCluster.generate(gpu_lib, **props(20))
    cm = ccmi.ClusterModel.from_buffers(buf)
    ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(ka))
    pl = Placement(buf.desc, cm.replica_distribution())
    src, cand = pl.replicas_on(0)[:3], pl.replicas_on(1)[:70]
    with pytest.raises(ccmi.IllegalStateException):
        cm.swaps_acceptance_grid(ka, src, cand)
    assert cm.swaps_acceptance_grid(ka, src, []).shape == (3, 0)
    legit = legit_swaps(pl, src, cand)
    assert (legit == ACCEPT).any()
    got = cm.swaps_acceptance_grid(ka[:1], src, cand)
    assert ((got >= SOURCE_NOT_LEGIT) == (legit != ACCEPT)).all() and (got[legit != ACCEPT] == legit[legit != ACCEPT]).all()
    for i, j in np.argwhere(legit == ACCEPT)[:20]:
        a = (SWAP, src[i][0], src[i][1], cand[j][1], cand[j][0], -1, -1)
        assert ccmi.ACCEPTANCE[got[i, j]] == cm.action_acceptance_by_goal(ka[0], *a)
