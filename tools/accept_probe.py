#!/usr/bin/env python3
"""Times ccmi_actions_acceptance against the per-cell path on one session.

A C1-size session (1000 brokers, 99,999 replicas, 3000 topics) optimizes the 16 default goals; then the same
n x 16 cells (n = 65,536 random replica moves, leadership moves and swaps of the resulting placement) are answered
  * by one ClusterModel.actions_acceptance call (kernels/accept.hip), and
  * by one ClusterModel.action_acceptance_by_goal call per cell (ccmi_action_acceptance_by_kind, the host path).
Prints one JSON line: both wall times, accept_kernel_ms, and the kernel's achieved bytes/s counting 0.45 KB gathered
per action (its replica, partition and two broker records; two of each for a swap) and 1 B stored per cell.

    python tools/accept_probe.py [--actions N] [--loop-actions M]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
import ccmi  # noqa: E402

C1_PROPS = dict(num_racks=20, num_brokers=1000, num_replicas=99999, num_topics=3000)
BYTES_PER_ACTION = 450
BYTES_PER_CELL = 1


def random_actions(cm, desc, n, seed):
    rs = np.random.RandomState(seed)
    B, P = desc.num_brokers, desc.num_partitions
    off = list(desc.partition_offset[:P + 1])
    dist, leaders = cm.replica_distribution(), cm.leader_distribution()
    slot_part = np.repeat(np.arange(P), np.diff(off))
    brokers = lambda p: dist[off[p]:off[p + 1]]  # noqa: E731
    acts = []
    while len(acts) < n:
        kind = len(acts) % 3
        if kind == 0:  # a replica to a broker that does not host its partition
            i, dst = int(rs.randint(len(dist))), int(rs.randint(B))
            p = int(slot_part[i])
            if dst not in brokers(p):
                acts.append((0, p, dist[i], dst, -1, -1, -1))
        elif kind == 1:  # the leader to a follower
            p = int(rs.randint(P))
            followers = [b for b in brokers(p) if b != leaders[p]]
            if followers:
                acts.append((1, p, leaders[p], followers[int(rs.randint(len(followers)))], -1, -1, -1))
        else:  # two replicas of different partitions, neither broker hosting the other's partition
            i, j = int(rs.randint(len(dist))), int(rs.randint(len(dist)))
            p, q = int(slot_part[i]), int(slot_part[j])
            if p != q and dist[i] != dist[j] and dist[j] not in brokers(p) and dist[i] not in brokers(q):
                acts.append((2, p, dist[i], dist[j], q, -1, -1))
    return acts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--actions", type=int, default=65536)
    ap.add_argument("--loop-actions", type=int, default=None,
                    help="actions of the per-cell loop (default: all; its time is reported for that many)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    goals = list(ccmi.DEFAULT_GOALS)
    buf = ccmi.RandomCluster.generate(**C1_PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf, device=args.device)
    bc = ccmi.BalancingConstraint()
    bc.set_resource_balance_percentage(1.05)
    t0 = time.perf_counter()
    ccmi.GoalOptimizer(bc).optimizations(cm, ccmi.goals_from_names(goals))
    chain_s = time.perf_counter() - t0
    acts = np.array(random_actions(cm, buf.desc, args.actions, 20261019), dtype=np.int32)

    cm.actions_acceptance(goals, acts[:64])  # first-launch costs (code object load, buffers) stay out of the timing
    cm.reset_perf()
    cm.set_kernel_timing(True)
    t0 = time.perf_counter()
    batch = cm.actions_acceptance(goals, acts)
    batch_s = time.perf_counter() - t0
    cm.set_kernel_timing(False)
    perf = cm.perf()

    m = args.actions if args.loop_actions is None else min(args.loop_actions, args.actions)
    loop = np.zeros((m, len(goals)), dtype=np.int8)
    rows = [tuple(int(x) for x in a) for a in acts[:m]]
    t0 = time.perf_counter()
    for i, a in enumerate(rows):
        for g, name in enumerate(goals):
            loop[i, g] = ccmi.ACCEPTANCE.index(cm.action_acceptance_by_goal(name, *a))
    loop_s = time.perf_counter() - t0
    same = bool((loop == batch[:m]).all())

    kernel_bytes = args.actions * BYTES_PER_ACTION + perf.accept_cells * BYTES_PER_CELL
    out = dict(brokers=buf.desc.num_brokers, replicas=buf.desc.num_replicas, goals=len(goals), actions=args.actions,
               cells=int(perf.accept_cells), chain_s=round(chain_s, 3), batch_call_ms=round(batch_s * 1e3, 3),
               accept_launches=int(perf.accept_launches), accept_kernel_ms=round(perf.accept_kernel_ms, 4),
               kernel_gbytes_per_s=round(kernel_bytes / (perf.accept_kernel_ms * 1e-3) / 1e9, 1)
               if perf.accept_kernel_ms > 0 else None,
               loop_actions=m, loop_s=round(loop_s, 3), loop_us_per_cell=round(loop_s / (m * len(goals)) * 1e6, 3),
               loop_s_for_all_cells=round(loop_s * args.actions / m, 3),
               speedup=round(loop_s * args.actions / m / batch_s, 1), loop_equals_batch=same,
               verdicts=np.bincount(batch.ravel(), minlength=3).tolist())
    print(json.dumps(out))
    if not same:
        sys.exit("the per-cell loop and the batch disagree")
    if not batch_s < loop_s * args.actions / m:
        sys.exit("the one-call path is not faster than the per-cell loop")


if __name__ == "__main__":
    main()
