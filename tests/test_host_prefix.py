"""The host prefix of Engine::pairScan: the first CCMI_HOST_PREFIX pairs of a pair scan are evaluated on
the host with the predicates the device evaluates, and a scan they decide posts nothing to the device. Whatever the
prefix length, a session makes the oracle's decisions with the oracle's reference-equivalent candidate counts; only
where the evaluations run changes (ccmi_host_prefix_perf).

The knobs are read when a session is created, so every case sets them before it builds its ClusterModel.
CCMI_HOST_PREFIX_GATE=0 turns the per-site predictor and its warm-up off: every eligible pair scan tries the prefix.
"""
import threading

import pytest

import ccmi
from parity import check_desc_against_oracle, check_product_against_golden, check_product_against_oracle

DEFAULT_GOALS = list(ccmi.DEFAULT_GOALS)
ALL_ON_HOST = "100000"  # longer than any pair list of these clusters: every pair scan is decided on the host
PREFIXES = ["0", "1", None, ALL_ON_HOST]  # None: the built-in default length

SMALL = dict(num_racks=4, num_brokers=16, num_replicas=4800, num_topics=200)
DEAD = dict(num_racks=3, num_brokers=9, num_replicas=2700, num_topics=60, num_dead_brokers=3, rack_aware=1)
GPU_PROPS = dict(num_racks=8, num_brokers=300, num_replicas=30000, num_topics=1000)


def set_knobs(monkeypatch, prefix, gate="0"):
    for name, value in (("CCMI_HOST_PREFIX", prefix), ("CCMI_HOST_PREFIX_GATE", gate)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def outcome(cm, res):
    return dict(actions=cm.actions(), replicas=cm.replica_distribution(), leaders=cm.leader_distribution(),
                goals=[(r.name, r.succeeded, r.candidates, r.actions) for r in res.goal_results])


@pytest.mark.parametrize("props,balance", [(SMALL, None), (DEAD, None)], ids=["small", "dead-brokers"])
def test_emu_oracle_parity_at_every_prefix_length(emu_lib, oracle_lib, monkeypatch, props, balance):
    outs = []
    for prefix in PREFIXES:
        set_knobs(monkeypatch, prefix)
        cm, res, _ = check_product_against_oracle(emu_lib, props, DEFAULT_GOALS, balance)
        assert res is not None
        p = cm.perf()
        if prefix == "0":
            assert p.host_scans == 0 and p.host_candidates == 0
        else:
            assert p.host_scans > 0 and p.host_candidates >= p.host_scans
        outs.append(outcome(cm, res))
    for o in outs[1:]:
        assert o == outs[0]


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
    newOnly) the host prefix answers with Engine::blocked: the goals' candidates must not depend on the side."""
    desc, keep, bc, options = make(emu_lib)
    outs = []
    for prefix in ("0", ALL_ON_HOST):
        set_knobs(monkeypatch, prefix)
        cm, res, _ = check_desc_against_oracle(emu_lib, desc, keep, DEFAULT_GOALS, bc, options)
        assert res is not None
        assert (cm.perf().host_scans > 0) == (prefix != "0")
        outs.append(outcome(cm, res))
    assert outs[0] == outs[1]


def test_emu_default_gate_keeps_the_device_path_on_a_small_golden(emu_lib, monkeypatch):
    """With the predictor on, a call site scans on the device until it has warmed up, so every goal that scans at all
    still launches (what tests/test_gpu_parity.py and test_concurrent_sessions.py assert on small goldens)."""
    set_knobs(monkeypatch, "0", None)
    _, off = check_product_against_golden(emu_lib, "small_20b_default")
    set_knobs(monkeypatch, None, None)
    _, on = check_product_against_golden(emu_lib, "small_20b_default")
    scanned = [r.name for r in off.goal_results if r.device_launches > 0]
    assert scanned
    for r in on.goal_results:
        assert (r.device_launches > 0) == (r.name in scanned), r.name


def test_emu_sharded_sessions_never_take_the_host_prefix(emu_lib, monkeypatch):
    """A world-2 destination-sharded pair (two sessions on two threads, their keys MIN-combined by a callback, as
    tests/test_shard.py does across processes): the prefix is off whatever the knobs say."""
    set_knobs(monkeypatch, ALL_ON_HOST)
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
        assert p.host_scans == 0 and p.host_candidates == 0
    # the same cluster unsharded does take it
    single = ccmi.ClusterModel.from_buffers(ccmi.RandomCluster.generate(emu_lib, **props), device=0)
    res = ccmi.GoalOptimizer(bc).optimizations(single, ccmi.goals_from_names(DEFAULT_GOALS))
    assert single.perf().host_scans > 0
    assert outcome(single, res) == outcome(cms[0], results[0])


# The leadership-heavy goal list tests/test_gpu_parity.py runs on the same cluster for its pair-scan cases. With
# DEFAULT_GOALS this cluster ends in DiskCapacityGoal's OptimizationFailureException (product and oracle alike, after
# 23 003 actions and before any pair scan), so that chain pins the parity of the failure and host_scans stays 0 on it
# whatever the prefix; the chain below is the one that reaches the leadership loops.
PAIR_SCAN_GOALS = ["LeaderReplicaDistributionGoal", "CpuUsageDistributionGoal", "NetworkOutboundUsageDistributionGoal",
                   "LeaderBytesInDistributionGoal"]


def gpu_run(gpu_lib, prefix):
    """GPU_PROPS at balance 1.05 with the knobs set: DEFAULT_GOALS (fails in DiskCapacityGoal exactly as the oracle does)
    and PAIR_SCAN_GOALS, both checked against the oracle. Returns PAIR_SCAN_GOALS' (outcome, perf counters)."""
    mp = pytest.MonkeyPatch()
    try:
        set_knobs(mp, prefix)
        cm, res, _ = check_product_against_oracle(gpu_lib, GPU_PROPS, DEFAULT_GOALS, 1.05)
        assert res is None and len(cm.actions()) > 0  # both raised the same exception after the same action log
        assert cm.perf().host_scans == 0
        cm, res, _ = check_product_against_oracle(gpu_lib, GPU_PROPS, PAIR_SCAN_GOALS, 1.05)
    finally:
        mp.undo()
    assert res is not None
    p = cm.perf()
    print(f"prefix {prefix}: host_scans {p.host_scans} host_candidates {p.host_candidates} server_scans {p.server_scans} "
          f"scan_launches {p.scan_launches} server_launches {p.server_launches} host_syncs {p.host_syncs}")
    return outcome(cm, res), p


@pytest.fixture(scope="module")
def gpu_prefix_off(gpu_lib, oracle_lib):
    out, p = gpu_run(gpu_lib, "0")
    assert p.host_scans == 0 and p.host_candidates == 0 and p.server_scans > 0
    return out, p


@pytest.mark.gpu
def test_gpu_oracle_parity_at_the_default_prefix(gpu_lib, oracle_lib, gpu_prefix_off):
    off, p_off = gpu_prefix_off
    on, p_on = gpu_run(gpu_lib, None)
    assert on == off
    assert p_on.host_scans > 0
    assert p_on.server_scans < p_off.server_scans  # the host-decided scans were not posted


ROW_BUDGET_SLACK = 16


@pytest.mark.gpu
def test_gpu_row_budget_keeps_the_scans_on_the_server(gpu_lib, oracle_lib, gpu_prefix_off):
    """Every pair scan decided on the host (2 339 of them on this chain): long runs of accepts whose rows reach the device
    only with the next posted scan. A scan whose rows no longer fit one server command costs a launch of its own and a
    server relaunch, so a budget rule that let rows pile up would show as hundreds of extra scan_launches.

    Measured once on an MI355X (PAIR_SCAN_GOALS): prefix 0 scan_launches 1 058 (127 of them server launches), default
    prefix 1 055 (124), prefix 100000 1 049 (118). The launches that are not server launches were 931 in all three runs:
    the rule declined no scan. The remaining difference is the number of server relaunches, which follows the wall
    clock (a server idle for 0.25 s is restarted): 9 between these runs. The slack is that spread rounded up to 16."""
    off, p_off = gpu_prefix_off
    on, p_on = gpu_run(gpu_lib, ALL_ON_HOST)
    assert on == off
    assert p_on.host_scans > 0
    assert p_on.scan_launches <= p_off.scan_launches + ROW_BUDGET_SLACK
