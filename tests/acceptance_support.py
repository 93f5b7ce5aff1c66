"""What the tests of the device-backed session queries share (test_actions_acceptance, test_moves_acceptance_mask,
test_swaps_acceptance_grid, test_broker_stats): constants, the placement of a model, a product session and an oracle
cluster after the same chain, and the fresh-process run of the chunk-boundary tests. Each test file keeps its own
sampling and its own reference."""
import json
import os
import subprocess
import sys

import numpy as np

import ccmi
from oracle_binding import OracleCluster

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_GOALS = list(ccmi.DEFAULT_GOALS)
SEED = 20261019
MOVE, LEADERSHIP, SWAP = 0, 1, 2
# ccmi.ACCEPTANCE indices, then the two legitimacy codes of ccmi.SWAP_CODES
ACCEPT, REPLICA_REJECT, BROKER_REJECT, SOURCE_NOT_LEGIT, CANDIDATE_NOT_LEGIT = range(5)
BAD_DISKS = ccmi.BROKER_STATES["BAD_DISKS"]


def props(num_brokers, **more):
    return dict(num_racks=5, num_brokers=num_brokers, num_replicas=6000, num_topics=300, **more)


class Placement:
    """Partition membership of a model (replica_distribution / leader_distribution order), as lists and as [P, B]
    matrices."""

    def __init__(self, desc, dist, leaders=None):
        self.B, self.P = desc.num_brokers, desc.num_partitions
        self.off = list(desc.partition_offset[:self.P + 1])
        self.dist = list(dist)
        self.leaders = None if leaders is None else list(leaders)
        self.slot_part = np.repeat(np.arange(self.P), np.diff(self.off))
        self.hosts = np.zeros((self.P, self.B), dtype=bool)
        self.hosts[self.slot_part, self.dist] = True
        # Partition._ineligibleBrokers: the BAD_DISKS brokers that held an offline replica of the partition (the desc)
        self.ineligible = np.zeros((self.P, self.B), dtype=bool)
        for r in range(desc.num_replicas):
            if desc.replica_offline[r] and desc.broker_state[desc.replica_broker[r]] == BAD_DISKS:
                self.ineligible[desc.replica_partition[r], desc.replica_broker[r]] = True

    def brokers(self, p):
        return self.dist[self.off[p]:self.off[p + 1]]

    def replicas_on(self, b):
        """Every replica of broker b as (partition, broker)."""
        return [(int(p), int(b)) for p in np.flatnonzero(self.hosts[:, b])]


class ChainCase:
    """A product session and an oracle cluster over one desc; optimize() runs the same chain on both and asserts that
    the action logs are equal."""

    def __init__(self, lib, desc, keepalive):
        self.desc, self.keep = desc, keepalive
        self.cm = ccmi.ClusterModel(desc, lib=lib, keepalive=keepalive)
        self.oc = OracleCluster.from_desc(desc)

    @classmethod
    def random(cls, lib, **cluster_props):
        buf = ccmi.RandomCluster.generate(lib, **cluster_props)
        return cls(lib, buf.desc, buf)

    def optimize(self, goals, bc, **kwargs):
        res = ccmi.GoalOptimizer(bc).optimizations(self.cm, ccmi.goals_from_names(goals), **kwargs)
        self.oc.optimize(goals, bc)
        assert self.cm.actions() == self.oc.actions()
        return res

    def placement(self):
        return Placement(self.desc, self.oc.replica_distribution(), self.oc.leader_distribution())


def status_of(call):
    """(exception type, its first_invalid) of a call that a ccmi error ends, else (None, None)."""
    try:
        call()
    except ccmi.CruiseControlError as e:
        return type(e), getattr(e, "first_invalid", None)
    return None, None


_FRESH_SCRIPT = r"""
import json, sys
import numpy as np
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {tests!r})
import ccmi
from parity import constraint
lib = ccmi.Library.get({lib!r})
buf = ccmi.RandomCluster.generate(lib, **{props!r})
cm = ccmi.ClusterModel.from_buffers(buf)
goals = list(ccmi.DEFAULT_GOALS)
ccmi.GoalOptimizer(constraint(1.05, max_replicas=3000)).optimizations(cm, ccmi.goals_from_names(goals))
sample = json.load(open({sample!r}))
cm.reset_perf()
got = {body}
json.dump(dict(got=got.tolist(), launches=cm.perf().accept_launches), open({out!r}, "w"))
"""


def run_in_fresh_process(gpu_lib, tmp_path, cluster_props, env, sample, body):
    """The chunk sizes are read at session create, so a chunk-boundary test needs a process of its own: a session on
    RandomCluster(cluster_props) after the default goals (max_replicas 3000), under the environment override `env`.
    `body` is an expression over cm, goals and sample (the JSON round trip of `sample`) that gives an array. Returns
    (the array as nested lists, perf().accept_launches of that one call)."""
    sample_file, out = tmp_path / "sample.json", tmp_path / "out.json"
    json.dump(sample, open(sample_file, "w"))
    code = _FRESH_SCRIPT.format(pkg=os.path.join(REPO, "cruise-control_amd"), tests=os.path.join(REPO, "tests"),
                                lib=gpu_lib.path, props=cluster_props, sample=str(sample_file), out=str(out), body=body)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    return res["got"], res["launches"]


# ------------------------------------------------------------------------------------------------ capacity goals
CAPACITY_GOALS = ["ReplicaCapacityGoal", "DiskCapacityGoal", "NetworkInboundCapacityGoal",
                  "NetworkOutboundCapacityGoal", "CpuCapacityGoal", "PotentialNwOutGoal"]
# One threshold for all four resources makes only DiskCapacityGoal reject (the cluster's CPU, NW_IN and NW_OUT sit far
# below any DISK threshold the chain survives), so each resource gets its own: 1.1 x its mean broker utilization
# (CPU 0.0312, NW_IN 0.1142, NW_OUT 0.0515, DISK 0.1100 of capacity). The chain survives them (74 actions) and leaves the
# most utilized brokers within one heavy replica of their limits.
CAPACITY_THRESHOLDS = (0.0343, 0.1256, 0.0566, 0.1210)
# the goals that both accept and reject some action of the directed sample (checked on the oracle): all five.
# ReplicaCapacityGoal's rejects are the max_replicas=302 case of test_actions_acceptance's matrix test.
CAPACITY_MIXED = ["DiskCapacityGoal", "NetworkInboundCapacityGoal", "NetworkOutboundCapacityGoal", "CpuCapacityGoal",
                  "PotentialNwOutGoal"]


def directed_capacity_actions(desc, pl, oc, k=6):
    """For each resource, the replicas of the k partitions that carry most of it x the k most utilized brokers of it
    that do not host the partition (replica moves), and those partitions' leaders to their followers."""
    W, R, P = desc.num_windows, desc.num_replicas, desc.num_partitions
    load = np.array(desc.replica_load[:R * 6 * W], dtype=np.float64).reshape(R, 6, W).mean(axis=2)
    part = np.array(desc.replica_partition[:R])
    acts = []
    # resource -> the ccmi_metric that carries it on a leader: CPU, NW_IN (leader bytes in), NW_OUT, DISK
    for res, metric in ((0, 0), (1, 2), (2, 3), (3, 1)):
        weight = np.zeros(P)
        np.maximum.at(weight, part, load[:, metric])
        util = [oc.broker_util(b, res) for b in range(pl.B)]
        hot = sorted(range(pl.B), key=lambda b: -util[b])[:k]
        for p in (int(x) for x in np.argsort(-weight, kind="stable")[:k]):
            for src in pl.brokers(p):
                acts += [(MOVE, p, src, dst, -1, -1, -1) for dst in hot if dst not in pl.brokers(p)]
            acts += [(LEADERSHIP, p, pl.leaders[p], dst, -1, -1, -1) for dst in pl.brokers(p) if dst != pl.leaders[p]]
    return acts
