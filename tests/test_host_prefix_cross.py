"""The host prefix of Engine::crossScan / crossScanSegs: the first CCMI_HOST_PREFIX_CROSS candidates of a
cross scan, in the device's key order (row-major: row k, column j, key k * N + j), are evaluated on the host with the
predicates the device evaluates. A scan they decide posts nothing; a miss posts the whole scan as before. Whatever the
prefix length, a session makes the oracle's decisions with the oracle's reference-equivalent candidate counts; only
where the evaluations run changes (ccmi_host_cross_perf).

The knobs are read when a session is created, so every case sets them before it builds its ClusterModel. The pair
prefix is off (CCMI_HOST_PREFIX=0) throughout, so only the cross prefix varies, and CCMI_HOST_PREFIX_GATE=0 turns the
per-site predictors and their warm-up off: every eligible cross scan tries the prefix.
"""
import threading

import pytest

import ccmi
from parity import check_desc_against_oracle, check_product_against_golden, check_product_against_oracle

DEFAULT_GOALS = list(ccmi.DEFAULT_GOALS)
# Longer than a candidate list of these clusters (N <= 16 brokers), so a prefix runs over whole rows into later ones; it
# still bounds the host's work per scan (move-in batches have thousands of rows).
LONG = "4096"
PREFIXES = ["0", "1", None, LONG]  # None: the built-in default length

SMALL = dict(num_racks=4, num_brokers=16, num_replicas=4800, num_topics=200)
DEAD = dict(num_racks=3, num_brokers=9, num_replicas=2700, num_topics=60, num_dead_brokers=3, rack_aware=1)
GPU_PROPS = dict(num_racks=8, num_brokers=300, num_replicas=30000, num_topics=1000)


def set_knobs(monkeypatch, cross, gate="0", pairs="0"):
    for name, value in (("CCMI_HOST_PREFIX_CROSS", cross), ("CCMI_HOST_PREFIX_GATE", gate), ("CCMI_HOST_PREFIX", pairs)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def outcome(cm, res):
    return dict(actions=cm.actions(), replicas=cm.replica_distribution(), leaders=cm.leader_distribution(),
                goals=[(r.name, r.succeeded, r.candidates, r.actions) for r in res.goal_results])


@pytest.mark.parametrize("props,balance", [(SMALL, None), (DEAD, None)], ids=["small", "dead-brokers"])
def test_emu_oracle_parity_at_every_cross_prefix_length(emu_lib, oracle_lib, monkeypatch, props, balance):
    """SMALL has 16 brokers, so every candidate list is shorter than the default prefix and far shorter than 4096: those
    runs continue a prefix from one row into the next (N <= 16 < H)."""
    assert props["num_brokers"] <= 16
    outs, decided = [], []
    for prefix in PREFIXES:
        set_knobs(monkeypatch, prefix)
        cm, res, _ = check_product_against_oracle(emu_lib, props, DEFAULT_GOALS, balance)
        assert res is not None
        p = cm.perf()
        assert p.host_scans == 0 and p.host_candidates == 0  # the pair counters stay pair-only
        if prefix == "0":
            assert p.host_cross_scans == 0 and p.host_cross_candidates == 0
        else:
            assert p.host_cross_scans > 0 and p.host_cross_candidates >= p.host_cross_scans
        decided.append(p.host_cross_scans)
        outs.append(outcome(cm, res))
    for o in outs[1:]:
        assert o == outs[0]
    assert decided[3] > decided[1]  # a prefix of one row and more decides scans a single candidate does not


def excluded_for_leadership(lib):
    buf = ccmi.RandomCluster.generate(lib, num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)
    bc = ccmi.BalancingConstraint()
    bc.set_resource_balance_percentage(1.05)
    bc.set_capacity_threshold(0.8)
    return buf.desc, buf, bc, ccmi.OptimizationOptions(excluded_brokers_for_leadership=[0, 3, 7, 11])


def with_new_brokers(lib):
    from test_new_brokers import CASES, constraint, new_broker_model
    props, goals, max_replicas = CASES[0]
    bc = constraint(max_replicas)
    m = new_broker_model(props, goals, bc)
    return m.desc, m, bc, None


@pytest.mark.parametrize("make", [excluded_for_leadership, with_new_brokers], ids=["excl-leadership", "new-brokers"])
def test_emu_blocked_candidates_are_counted_alike(emu_lib, oracle_lib, monkeypatch, make):
    """Brokers excluded for leadership and NEW brokers set the replica-dependent candidate filters (exclLeadMove,
    newOnly): the host prefix passes over the candidates Engine::blocked names, as the kernels do, and the goals'
    candidates (Engine::exclLeadCount) must not depend on the side that decided the scan."""
    desc, keep, bc, options = make(emu_lib)
    outs = []
    for prefix in ("0", LONG):
        set_knobs(monkeypatch, prefix)
        cm, res, _ = check_desc_against_oracle(emu_lib, desc, keep, DEFAULT_GOALS, bc, options)
        assert res is not None
        p = cm.perf()
        assert (p.host_cross_scans > 0) == (prefix != "0")
        assert p.host_scans == 0
        outs.append(outcome(cm, res))
    assert outs[0] == outs[1]


def test_emu_default_gate_keeps_the_device_path_on_a_small_golden(emu_lib, monkeypatch):
    """With the predictors on and default knobs, a call site scans on the device until it has warmed up, so every goal
    that scans at all still launches (what tests/test_gpu_parity.py and test_concurrent_sessions.py assert)."""
    set_knobs(monkeypatch, "0", None, "0")
    _, off = check_product_against_golden(emu_lib, "small_20b_default")
    set_knobs(monkeypatch, None, None, None)
    _, on = check_product_against_golden(emu_lib, "small_20b_default")
    scanned = [r.name for r in off.goal_results if r.device_launches > 0]
    assert scanned
    for r in on.goal_results:
        if r.name in scanned:
            assert r.device_launches > 0, r.name


def test_emu_sharded_sessions_never_take_the_cross_prefix(emu_lib, monkeypatch):
    """A world-2 destination-sharded pair (two sessions on two threads, their keys MIN-combined by a callback): the
    prefix is off whatever the knobs say."""
    set_knobs(monkeypatch, LONG)
    props = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)
    bufs = [ccmi.RandomCluster.generate(emu_lib, **props) for _ in range(2)]
    cms = [ccmi.ClusterModel.from_buffers(b, device=0) for b in bufs]
    keys, barrier = [0, 0], threading.Barrier(2)

    def combiner(rank):
        def combine_min(key):
            keys[rank] = key
            barrier.wait(60)
            k = min(keys)
            barrier.wait(60)
            return k
        return combine_min

    bc = ccmi.BalancingConstraint()
    bc.set_resource_balance_percentage(1.05)
    bc.set_capacity_threshold(0.8)
    results, errors = [None, None], []

    def run(rank):
        try:
            cms[rank].set_shard(rank, 2, combiner(rank))
            results[rank] = ccmi.GoalOptimizer(bc).optimizations(cms[rank], ccmi.goals_from_names(DEFAULT_GOALS))
        except BaseException as e:  # noqa: BLE001 - reported below; a broken barrier releases the other rank
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert outcome(cms[0], results[0]) == outcome(cms[1], results[1])
    for cm in cms:
        p = cm.perf()
        assert p.combines > 0
        assert p.host_cross_scans == 0 and p.host_cross_candidates == 0
    # the same cluster unsharded does take it
    single = ccmi.ClusterModel.from_buffers(ccmi.RandomCluster.generate(emu_lib, **props), device=0)
    res = ccmi.GoalOptimizer(bc).optimizations(single, ccmi.goals_from_names(DEFAULT_GOALS))
    assert single.perf().host_cross_scans > 0
    assert outcome(single, res) == outcome(cms[0], results[0])


# DEFAULT_GOALS ends in DiskCapacityGoal's OptimizationFailureException on this cluster (product and oracle alike), so
# the GPU case runs a chain that completes there and whose move-out loops scan through crossScan (chosen on the CPU
# emulation, where the default prefix decides about 200 of its cross scans; the replica-count goals find this cluster
# balanced already and scan nothing).
CROSS_SCAN_GOALS = ["DiskUsageDistributionGoal", "NetworkInboundUsageDistributionGoal",
                    "NetworkOutboundUsageDistributionGoal", "CpuUsageDistributionGoal"]
ROW_BUDGET_SLACK = 16  # tests/test_host_prefix.py: the spread of wall-clock server relaunches between runs, rounded up


def cross_run(lib, prefix):
    mp = pytest.MonkeyPatch()
    try:
        set_knobs(mp, prefix)
        cm, res, _ = check_product_against_oracle(lib, GPU_PROPS, CROSS_SCAN_GOALS, 1.05)
    finally:
        mp.undo()
    assert res is not None
    p = cm.perf()
    print(f"cross prefix {prefix}: host_cross_scans {p.host_cross_scans} host_cross_candidates {p.host_cross_candidates} "
          f"server_scans {p.server_scans} scan_launches {p.scan_launches} server_launches {p.server_launches} "
          f"host_syncs {p.host_syncs}")
    return outcome(cm, res), p


@pytest.mark.gpu
def test_gpu_oracle_parity_and_row_budget_at_the_default_cross_prefix(gpu_lib, oracle_lib):
    """Every eligible cross scan tries the default prefix (gate off). The host-decided scans post nothing, so their
    actions' rows reach the device only with the next posted scan: a row budget that let them pile up past one server
    command would show as extra scan_launches (a prep + scan launch and a server restart each), beyond the spread of
    wall-clock server relaunches ROW_BUDGET_SLACK stands for."""
    off, p_off = cross_run(gpu_lib, "0")
    assert p_off.host_cross_scans == 0 and p_off.host_cross_candidates == 0 and p_off.server_scans > 0
    on, p_on = cross_run(gpu_lib, None)
    assert on == off
    assert p_on.host_cross_scans > 0 and p_on.host_scans == 0
    assert p_on.server_scans < p_off.server_scans  # the host-decided scans were not posted
    assert p_on.scan_launches <= p_off.scan_launches + ROW_BUDGET_SLACK
