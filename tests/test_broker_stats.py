"""ccmi_broker_stats: ClusterModel.brokerStats read back from the device tables (kernels/broker_stats.hip).

The reference of every test is the oracle cluster after the same chain (the action logs are asserted equal first):
broker_util for the four utilizations, replica_distribution / leader_distribution for the counts, replica_disks /
disk_utilization for the disks, the desc for capacities, states, racks and hosts, stats() for the potential-NW_OUT
extremes. Everything derived from these is compared exactly: disk_mb, disk_pct, cpu_pct, nw_out_rate, the capacities,
num_core, the counts, and the host rows as ordered double sums (a Python loop in broker order).

The oracle has no per-broker accessor for leadership NW_IN or potential NW_OUT, so leader_nw_in_rate and pnw_out_rate
are checked against a float64 recomputation from the desc: a replica's NW_IN windows never change and a partition's
leader NW_OUT windows travel intact with leadership (loadops.h ldMakeFollower), so
    lbi_b = f32(sum LBI / W) + f32(sum RBI / W) over the leaders on b,
    pot_b = f32(sum LBO / W) + f32(sum RBO / W) over the replicas on b, windows of each partition's original leader.
The tolerance is derived, not measured: |got - want| <= 2^-22 |want| + (2R + 2A) 2^-53 S, A the action count and S the
sum of the absolute window values of the two metrics over all replicas: two float32 roundings on each side, and double
accumulation error of at most R + 2A running-sum updates in the reference plus R additions here. follower_nw_in_rate
gets the same absolute bound; the max and min of pnw_out_rate over alive brokers equal the oracle's exactly.
"""
import random

import numpy as np
import pytest

import ccmi
from acceptance_support import DEFAULT_GOALS, LEADERSHIP, MOVE, SWAP, ChainCase, props
from parity import assign_shared_hosts, constraint
from test_hosts import SHARED, _model as hosts_model
from test_ingest import _random_cluster_via_builder
from test_jbod import INTRA, rebalance_constraint

pytestmark = pytest.mark.gpu

CPU, NW_IN, NW_OUT, DISK = 0, 1, 2, 3
M_LBI, M_LBO, M_RBI, M_RBO = 2, 3, 4, 5
DEAD = ccmi.BROKER_STATES["DEAD"]
EXACT = ("disk_mb", "disk_pct", "cpu_pct", "nw_out_rate", "disk_capacity_mb", "network_in_capacity",
         "network_out_capacity", "num_core", "replicas", "leaders", "broker", "state", "host", "rack")
DOUBLES = ("disk_mb", "cpu_pct", "leader_nw_in_rate", "follower_nw_in_rate", "nw_out_rate", "pnw_out_rate",
           "disk_capacity_mb", "network_in_capacity", "network_out_capacity", "num_core")
JSON_BASIC = {"DiskMB", "DiskPct", "CpuPct", "LeaderNwInRate", "FollowerNwInRate", "NwOutRate", "PnwOutRate", "Replicas",
              "Leaders", "DiskCapacityMB", "NetworkInCapacity", "NetworkOutCapacity", "NumCore"}
JBOD3 = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=200, rack_aware=1, jbod=2, num_logdirs=3,
             logdir_capacity=[75000.0] * 3, num_brokers_with_bad_disk=1)


def jmax0(x):
    """Math.max(x, 0.0)."""
    return x if x != x else (x if x > 0.0 else 0.0)


def disk_pct(disk_mb, cap):
    return 100 * disk_mb / cap if cap > 0 else -1.0


class Expected:
    """The broker, host and disk rows the oracle cluster `oc` stands for, `actions` being its whole action log."""

    def __init__(self, desc, oc, actions):
        B, P, R, W = desc.num_brokers, desc.num_partitions, desc.num_replicas, desc.num_windows
        self.B, self.A = B, len(actions)
        off = list(desc.partition_offset[:P + 1])
        dist, leaders = oc.replica_distribution(), oc.leader_distribution()
        slot_part = np.repeat(np.arange(P), np.diff(off))
        nrep = np.bincount(dist, minlength=B)
        nlead = np.bincount(leaders, minlength=B)
        state = list(desc.broker_state[:B])
        host = [desc.broker_host[b] if desc.broker_host else b for b in range(B)]
        self.alive = [s != DEAD for s in state]
        # ---- the exact columns
        rows = []
        for b in range(B):
            cap = [-1.0 if state[b] == DEAD else desc.broker_capacity[4 * b + k] for k in range(4)]  # Broker.setState
            u = [oc.broker_util(b, k) for k in range(4)]
            r = dict(disk_mb=jmax0(0.0 if nrep[b] == 0 else u[DISK]), cpu_pct=jmax0(100.0 * u[CPU] / cap[CPU]),
                     nw_out_rate=jmax0(u[NW_OUT]), disk_capacity_mb=jmax0(cap[DISK]),
                     network_in_capacity=jmax0(cap[NW_IN]), network_out_capacity=jmax0(cap[NW_OUT]),
                     num_core=jmax0(cap[CPU] / 100), replicas=int(nrep[b]), leaders=int(nlead[b]), broker=b,
                     state=state[b], host=host[b], rack=desc.broker_rack[b], nw_in=u[NW_IN])
            r["disk_pct"] = disk_pct(r["disk_mb"], r["disk_capacity_mb"])
            rows.append(r)
        self.rows = rows
        # ---- leadership NW_IN and potential NW_OUT, recomputed in float64 from the desc
        load = np.array(desc.replica_load[:R * 6 * W], dtype=np.float32).reshape(R, 6, W).astype(np.float64)
        where = {(desc.replica_partition[r], desc.replica_broker[r]): r for r in range(R)}  # (partition, broker) -> replica
        for typ, p, src, dst, dp, _, _ in actions:
            if typ in (MOVE, SWAP):
                where[(p, dst)] = where.pop((p, src))
            if typ == SWAP:
                where[(dp, src)] = where.pop((dp, dst))
        orig_leader = {desc.replica_partition[r]: r for r in range(R) if desc.replica_is_leader[r]}
        lbi = np.zeros((B, 2))
        pot = np.zeros((B, 2))
        for p in range(P):
            r = where[(p, leaders[p])]
            lbi[leaders[p]] += (load[r, M_LBI].sum(), load[r, M_RBI].sum())
        for i, b in enumerate(dist):
            r = orig_leader[int(slot_part[i])]
            pot[b] += (load[r, M_LBO].sum(), load[r, M_RBO].sum())
        f32 = lambda x: float(np.float32(x))  # noqa: E731
        self.lbi = [f32(lbi[b, 0] / W) + f32(lbi[b, 1] / W) for b in range(B)]
        self.pot = [f32(pot[b, 0] / W) + f32(pot[b, 1] / W) for b in range(B)]
        slack = (2 * R + 2 * self.A) * 2.0 ** -53
        self.lbi_slack = slack * float(np.abs(load[:, [M_LBI, M_RBI]]).sum())
        self.pot_slack = slack * float(np.abs(load[:, [M_LBO, M_RBO]]).sum())
        # ---- hosts: brokers of a host in ascending index, hosts in ascending host index
        self.host_brokers = {}
        for b in range(B):
            self.host_brokers.setdefault(host[b], []).append(b)
        # ---- disks
        D = desc.num_disks
        self.disks = []
        if D:
            rd = oc.replica_disks()
            lead_slot = [dist[i] == leaders[slot_part[i]] for i in range(R)]
            for d in range(D):
                cap = -1.0 if desc.disk_capacity[d] < 0 or state[desc.disk_broker[d]] == DEAD else desc.disk_capacity[d]
                util = oc.disk_utilization(d)
                dead = not cap > 0
                self.disks.append(dict(disk_mb=-1.0 if dead else util, disk_pct=-1.0 if dead else util * 100.0 / cap,
                                       capacity=cap, num_replicas=sum(1 for i in range(R) if rd[i] == d),
                                       num_leader_replicas=sum(1 for i in range(R) if rd[i] == d and lead_slot[i]),
                                       disk=d, broker=desc.disk_broker[d]))

    def lbi_bound(self, b):
        return 2.0 ** -22 * abs(self.lbi[b]) + self.lbi_slack

    def pot_bound(self, b):
        return 2.0 ** -22 * abs(self.pot[b]) + self.pot_slack

    def check(self, bs, oc_stats=None):
        got = bs.brokers
        assert len(got) == self.B
        for b, want in enumerate(self.rows):
            for f in EXACT:
                assert got[f][b] == want[f], (b, f, got[f][b], want[f])
            assert list(got["reserved"][b]) == [0, 0, 0, 0]
            l, p = float(got["leader_nw_in_rate"][b]), float(got["pnw_out_rate"][b])
            assert abs(l - jmax0(self.lbi[b])) <= self.lbi_bound(b), (b, l, self.lbi[b], self.lbi_bound(b))
            assert abs(p - jmax0(self.pot[b])) <= self.pot_bound(b), (b, p, self.pot[b], self.pot_bound(b))
            f_want = jmax0(want["nw_in"] - jmax0(self.lbi[b]))
            f_got = float(got["follower_nw_in_rate"][b])
            assert abs(f_got - f_want) <= self.lbi_bound(b), (b, f_got, f_want)
            # and exactly what BasicStats makes of the device's own leader rate
            assert f_got == jmax0(want["nw_in"] - l), (b, f_got, want["nw_in"], l)
        if oc_stats is not None:
            alive = [float(got["pnw_out_rate"][b]) for b in range(self.B) if self.alive[b]]
            assert max(alive) == oc_stats["potential_nw_out_max"]
            assert min(alive) == oc_stats["potential_nw_out_min"]
        self.check_hosts(bs)
        self.check_disks(bs)

    def check_hosts(self, bs):
        got, rows = bs.hosts, bs.brokers
        assert len(got) == len(self.host_brokers)
        for i, h in enumerate(sorted(self.host_brokers)):
            members = self.host_brokers[h]
            assert (got["host"][i], got["broker"][i], got["state"][i]) == (h, -1, -1), i
            assert got["rack"][i] == self.rows[members[0]]["rack"]
            assert list(got["reserved"][i]) == [0, 0, 0, 0]
            for f in DOUBLES:  # SingleHostStats.addBasicStats: 0.0 + row + row ..., ascending broker index
                exact = f in EXACT
                acc = 0.0
                for b in members:
                    acc += self.rows[b][f] if exact else float(rows[f][b])
                assert got[f][i] == acc, (i, f, got[f][i], acc)
            for f in ("replicas", "leaders"):
                assert got[f][i] == sum(self.rows[b][f] for b in members), (i, f)
            assert got["disk_pct"][i] == disk_pct(float(got["disk_mb"][i]), float(got["disk_capacity_mb"][i])), i

    def check_disks(self, bs):
        assert len(bs.disks) == len(self.disks)
        for d, want in enumerate(self.disks):
            for f, v in want.items():
                assert bs.disks[f][d] == v, (d, f, bs.disks[f][d], v)

    def columns_changed_from(self, other):
        """Names of the exact, chain-dependent columns (and the two recomputed ones) that differ on some broker."""
        out = [f for f in ("disk_mb", "disk_pct", "cpu_pct", "nw_out_rate", "replicas", "leaders")
               if any(a[f] != b[f] for a, b in zip(self.rows, other.rows))]
        out += ["leader_nw_in_rate"] if self.lbi != other.lbi else []
        out += ["pnw_out_rate"] if self.pot != other.pot else []
        out += ["follower_nw_in_rate"] if any(a["nw_in"] - x != b["nw_in"] - y for a, b, x, y in
                                              zip(self.rows, other.rows, self.lbi, other.lbi)) else []
        return out


CHAIN_COLUMNS = ["disk_mb", "disk_pct", "cpu_pct", "nw_out_rate", "replicas", "leaders", "leader_nw_in_rate",
                 "pnw_out_rate", "follower_nw_in_rate"]


class Case(ChainCase):
    def expected(self):
        return Expected(self.desc, self.oc, self.oc.actions())


random_case = Case.random


# ------------------------------------------------------------------------------------------------ T1
@pytest.mark.parametrize("num_brokers", [130, 20], ids=["b130", "b20"])
def test_fresh_and_after_the_default_goals(gpu_lib, oracle_lib, num_brokers):
    """130 brokers: three wavefronts, the last one partial; 20: less than one. The stats of the fresh session are the
    reference's brokerStatsBeforeOptimization, those after the chain its brokerStatsAfterOptimization."""
    bc = constraint(1.05, max_replicas=3000)
    c = random_case(gpu_lib, **props(num_brokers))
    before = c.expected()
    fresh = c.cm.broker_stats()
    before.check(fresh, c.oc.stats(bc))
    c.optimize(DEFAULT_GOALS, bc)
    after = c.expected()
    assert after.A > 0 and after.columns_changed_from(before) == CHAIN_COLUMNS  # a stale read would not pass
    after.check(c.cm.broker_stats(), c.oc.stats(bc))
    assert fresh.brokers.tobytes() != c.cm.broker_stats().brokers.tobytes()
    p = c.cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)  # not an acceptance call


# ------------------------------------------------------------------------------------------------ T2
def test_dead_brokers_and_an_empty_broker(gpu_lib, oracle_lib):
    """Two dead brokers (capacity -1: the capacity fields and cpu_pct are 0, disk_pct -1) and one alive broker that
    holds no replica (disk_mb 0), fresh and after the chain has emptied the dead brokers."""
    bc = constraint(1.05, max_replicas=3000)
    base = ccmi.RandomCluster.generate(gpu_lib, num_dead_brokers=2, **props(20))
    from oracle_binding import ArrayDesc, desc_arrays
    a = {k: list(v) if not isinstance(v, int) else v for k, v in desc_arrays(base.desc).items()}
    a["broker_state"] += [0]  # broker 20: alive, no replica
    a["broker_rack"] += [1]
    a["cap"] += [100.0, 300000.0, 200000.0, 300000.0]
    flat = ArrayDesc(a)
    c = Case(gpu_lib, flat.desc, (flat, base))
    dead = [b for b in range(20) if flat.desc.broker_state[b] == DEAD]
    assert len(dead) == 2

    def check_special(bs, empty):
        for b in dead:
            row = bs.brokers[b]
            assert (row["disk_capacity_mb"], row["network_in_capacity"], row["network_out_capacity"],
                    row["num_core"]) == (0.0, 0.0, 0.0, 0.0)
            assert row["cpu_pct"] == 0.0 and row["disk_pct"] == -1.0 and row["state"] == DEAD
        for b in empty:
            assert bs.brokers["replicas"][b] == 0 and bs.brokers["disk_mb"][b] == 0.0

    fresh = c.cm.broker_stats()
    c.expected().check(fresh, c.oc.stats(bc))
    check_special(fresh, [20])
    assert all(fresh.brokers["replicas"][b] > 0 for b in dead)
    c.optimize(DEFAULT_GOALS, bc)
    after = c.cm.broker_stats()
    c.expected().check(after, c.oc.stats(bc))
    check_special(after, dead)  # self-healing moved every replica off the dead brokers
    assert after.brokers["replicas"][20] > 0


# ------------------------------------------------------------------------------------------------ T3
def test_shared_hosts_builder_model(gpu_lib, oracle_lib):
    """test_hosts.SHARED: brokers 0 and 2 share hA, 4 and 5 are named hC in different racks (two hosts), 3 has a host of
    its own. The host rows are ordered sums of the broker rows; the loads stay the broker's own."""
    flat = hosts_model(SHARED)
    c = Case(gpu_lib, flat.desc, flat)
    c.expected().check(c.cm.broker_stats())
    c.optimize(DEFAULT_GOALS, constraint(1.05))
    bs = c.cm.broker_stats()
    c.expected().check(bs)
    assert len(bs.hosts) == 5 and list(bs.hosts["host"]) == sorted(set(bs.brokers["host"]))
    js = bs.get_json_structure()
    # broker 3 was created without a host name: its host (index 2) is written in decimal
    assert [(h["Host"], h["Rack"]) for h in js["hosts"]] == [("2", "r1"), ("hA", "r0"), ("hB", "r1"), ("hC", "r0"),
                                                            ("hC", "r1")]
    assert {(b["Broker"], b["Host"], b["Rack"]) for b in js["brokers"]} == {
        (0, "hA", "r0"), (1, "hB", "r1"), (2, "hA", "r0"), (3, "2", "r1"), (4, "hC", "r0"), (5, "hC", "r1")}


def test_shared_hosts_not_adjacent(gpu_lib, oracle_lib):
    """A RandomCluster whose hosts hold brokers that are not neighbours: within a rack, broker i of the rack goes to the
    rack's host i % H, so a host's brokers are spread over the index range and the host index order is not the order of
    a host's first broker."""
    buf = ccmi.RandomCluster.generate(gpu_lib, **props(22))
    d = buf.desc
    per_rack = {}
    hosts = []
    H = 2
    for b in range(d.num_brokers):
        i = per_rack.setdefault(d.broker_rack[b], 0)
        per_rack[d.broker_rack[b]] = i + 1
        # host indices descend with the rack so the first-appearance order differs from the index order
        hosts.append((d.num_racks - 1 - d.broker_rack[b]) * H + i % H)
    import ctypes as C
    arr = (C.c_int32 * d.num_brokers)(*hosts)
    d.broker_host = C.cast(arr, type(d.broker_host))
    c = Case(gpu_lib, d, (buf, arr))
    c.expected().check(c.cm.broker_stats())
    c.optimize(DEFAULT_GOALS, constraint(1.05, max_replicas=3000))
    bs = c.cm.broker_stats()
    c.expected().check(bs)
    assert len(bs.hosts) == len(set(hosts)) < d.num_brokers
    assert any(len(m) > 1 and m[-1] - m[0] >= len(m) for m in c.expected().host_brokers.values())


# ------------------------------------------------------------------------------------------------ T4
def test_pending_rows_reach_the_device_first(gpu_lib, oracle_lib):
    """ccmi_session_apply leaves dirty rows on the host; broker_stats right after it, with no scan in between, must see
    them (Device::brokerStats packs the pending updates and runs prep before the kernel reads BrokerRec)."""
    bc = constraint(1.05, max_replicas=3000)
    c = random_case(gpu_lib, **props(20))
    c.optimize(DEFAULT_GOALS, bc)
    before = c.cm.broker_stats()
    d = c.desc
    off = list(d.partition_offset[:d.num_partitions + 1])
    dist, leaders = c.oc.replica_distribution(), c.oc.leader_distribution()
    rs = random.Random(7)
    actions, touched = [], set()
    parts = rs.sample(range(d.num_partitions), d.num_partitions)
    for p in parts:  # three moves to brokers that do not host the partition, brokers pairwise distinct
        here = dist[off[p]:off[p + 1]]
        free = [b for b in range(d.num_brokers) if b not in here and b not in touched]
        src = [b for b in here if b not in touched]
        if len(actions) < 3 and free and src:
            actions.append((MOVE, p, src[0], free[0], -1, -1, -1))
            touched |= {src[0], free[0]}
        elif len(actions) == 3 and len(here) > 1:
            followers = [b for b in here if b != leaders[p]]
            actions.append((LEADERSHIP, p, leaders[p], followers[0], -1, -1, -1))
            break
    assert [a[0] for a in actions] == [MOVE, MOVE, MOVE, LEADERSHIP]
    assert c.cm.apply(actions) == 4
    bs = c.cm.broker_stats()  # nothing between apply and the read-back
    c.oc.apply(actions)
    assert c.cm.actions() == c.oc.actions()
    c.expected().check(bs, c.oc.stats(bc))
    changed = [b for b in range(d.num_brokers) if bs.brokers[b].tobytes() != before.brokers[b].tobytes()]
    assert len(changed) >= 4, changed


# ------------------------------------------------------------------------------------------------ T5
def test_jbod_disk_rows(gpu_lib, oracle_lib):
    """jbod=2 with 3 logdirs and one BAD_DISKS broker (a disk with capacity -1: disk_mb = disk_pct = -1, "DEAD" in the
    JSON), fresh and after the two intra-broker goals. Only intra-broker moves run here, so no Disk._replicas keeps a
    replica that left its broker and the oracle's replica_disks() is the membership the reference counts (an
    inter-broker move would leave the replica in its old disk's set as well: Broker.removeReplica does not touch
    disks, and ccmi_broker_stats counts Disk._replicas as the model keeps it)."""
    bc = rebalance_constraint()
    c = random_case(gpu_lib, **JBOD3)
    d = c.desc
    dead = [k for k in range(d.num_disks) if d.disk_capacity[k] < 0]
    assert d.num_disks == 60 and len(dead) == 1
    fresh = c.cm.broker_stats()
    before = c.expected()
    before.check(fresh)
    assert fresh.disks["num_replicas"].sum() == d.num_replicas
    assert fresh.disks["num_leader_replicas"].sum() == d.num_partitions
    assert fresh.disks["num_replicas"][dead[0]] > 0
    c.optimize(INTRA, bc)
    after = c.expected()
    assert after.A > 0 and after.disks != before.disks
    bs = c.cm.broker_stats()
    after.check(bs)
    for k in dead:
        assert (bs.disks["disk_mb"][k], bs.disks["disk_pct"][k], bs.disks["capacity"][k]) == (-1.0, -1.0, -1.0)
    js = bs.get_json_structure()
    for e in js["brokers"]:
        assert set(e) == JSON_BASIC | {"Host", "Broker", "BrokerState", "Rack", "DiskState"}
        mine = sorted(d.disk_logdir[k].decode() for k in range(d.num_disks) if d.disk_broker[k] == e["Broker"])
        assert list(e["DiskState"]) == mine and len(mine) == 3  # logdir order, the broker's TreeMap
        for v in e["DiskState"].values():
            assert set(v) == {"DiskMB", "DiskPct", "NumLeaderReplicas", "NumReplicas"}
    states = js["brokers"][d.disk_broker[dead[0]]]
    assert states["BrokerState"] == "BAD_DISKS"
    assert [v["DiskMB"] for v in states["DiskState"].values()].count("DEAD") == 1
    assert [v["DiskPct"] for v in states["DiskState"].values()].count("DEAD") == 1
    assert c.cm.broker_stats() == bs  # the member list is reused: same answer


# ------------------------------------------------------------------------------------------------ T6
def test_three_windows_through_the_builder(gpu_lib, oracle_lib):
    """num_windows = 3 (test_ingest's builder model with two dead brokers): a W-dependent read would show here. The
    model has replication factor 4 on 3 racks, so the chain is the default goals without RackAwareGoal, which fails
    there before it moves anything."""
    m, _ = _random_cluster_via_builder(gpu_lib, seed=2, dead=(4, 9))
    bc = constraint(1.05, 3000)
    c = Case(gpu_lib, m.desc(), m)
    assert c.desc.num_windows == 3
    before = c.expected()
    before.check(c.cm.broker_stats(), c.oc.stats(bc))
    c.optimize([g for g in DEFAULT_GOALS if g != "RackAwareGoal"], bc)
    assert c.expected().columns_changed_from(before) == CHAIN_COLUMNS
    bs = c.cm.broker_stats()
    c.expected().check(bs, c.oc.stats(bc))
    js = bs.get_json_structure()  # names from the builder; a broker only partitions name has its UNKNOWN host
    ids = m.broker_ids()
    assert [e["Broker"] for e in js["brokers"]] == ids
    for e in js["brokers"]:
        assert e["Rack"] == f"rack{e['Broker'] % 3}"
        assert e["Host"] == (f"UNKNOWN-{e['Broker']}" if e["Broker"] in (4, 9) else f"h{e['Broker']}")
        assert e["BrokerState"] == ("DEAD" if e["Broker"] in (4, 9) else "ALIVE")


# ------------------------------------------------------------------------------------------------ T7
def test_json_and_optimizer_result(gpu_lib, oracle_lib):
    """get_json_structure has exactly the reference's key sets; optimizations(..., broker_stats=True) carries both load
    blocks; a repeated call answers bit for bit the same (the session is not changed)."""
    bc = constraint(1.05, max_replicas=3000)
    c = random_case(gpu_lib, **props(20))
    fresh = c.cm.broker_stats()
    res = c.optimize(DEFAULT_GOALS, bc, broker_stats=True)
    assert res.broker_stats_before_optimization == fresh
    after = res.broker_stats_after_optimization
    assert after is res.broker_stats_after_optimization and after != fresh
    c.expected().check(after, c.oc.stats(bc))
    again = c.cm.broker_stats()
    assert again == after and again.brokers.tobytes() == after.brokers.tobytes()
    assert again.hosts.tobytes() == after.hosts.tobytes() and len(after.disks) == 0
    assert c.cm.actions() == c.oc.actions()  # reading changed nothing
    js = after.get_json_structure()
    assert set(js) == {"hosts", "brokers"} and len(js["brokers"]) == 20 and len(js["hosts"]) == 20
    for e in js["brokers"]:
        assert set(e) == JSON_BASIC | {"Host", "Broker", "BrokerState", "Rack"}  # no DiskState without disks
        assert e["BrokerState"] == "ALIVE" and isinstance(e["Replicas"], int) and isinstance(e["DiskMB"], float)
    for e in js["hosts"]:
        assert set(e) == JSON_BASIC | {"Host", "Rack"}
    assert [e["Host"] for e in js["hosts"]] == sorted(str(b) for b in range(20))  # by name: "10" before "2"
    assert [e["Broker"] for e in js["brokers"]] == list(range(20))
    load = res.load_json(verbose=True)
    assert list(load) == ["loadBeforeOptimization", "loadAfterOptimization"]
    assert load["loadAfterOptimization"] == js and load["loadBeforeOptimization"] == fresh.get_json_structure()
    assert list(res.load_json()) == ["loadAfterOptimization"]
    # without the flag nothing is taken before, and the block is left out even in verbose mode
    c2 = random_case(gpu_lib, **props(20))
    res2 = c2.optimize(DEFAULT_GOALS, bc)
    assert res2.broker_stats_before_optimization is None
    assert list(res2.load_json(verbose=True)) == ["loadAfterOptimization"]
    assert res2.broker_stats_after_optimization == after
