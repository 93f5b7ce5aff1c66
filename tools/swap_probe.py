#!/usr/bin/env python3
"""Times ccmi_swaps_acceptance_grid against ccmi_actions_acceptance on one session, for the same question.

A C1-size session (1000 brokers, 99,999 replicas, 3000 topics, as tools/accept_probe.py) optimizes the 16 default goals.
The question is a swap loop's (AbstractGoal.maybeApplySwapAction): for 64 source replicas of one broker against every
replica of 8 other brokers, is the pair legit both ways, and what is the first verdict of the 16 goals that is not
ACCEPT. It is answered, in the same process on the same session,
  * (A) by one ClusterModel.swaps_acceptance_grid call (kernels/accept_swap.hip): 64 + m replicas in, 64 x m codes out,
  * (B) by one ClusterModel.actions_acceptance call (kernels/accept.hip) on the cells that are legit both ways, one swap
    action per cell, whose rows the caller then scans for the first non-zero verdict. Building the action list, and
    the legitimacy checks that select its cells, are not timed: a caller without the grid call pays for them too.
After a warm-up of both, the two calls alternate for --repeats rounds; the medians of the wall times (each call ends in
a stream synchronise) and of the kernels' HIP-event times (accept_kernel_ms) are printed as one JSON line, with both
per-cell figures over the cells each call stands for. The answers are compared before anything is timed.

    python tools/swap_probe.py [--sources N] [--brokers K] [--repeats R]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
import ccmi  # noqa: E402

C1_PROPS = dict(num_racks=20, num_brokers=1000, num_replicas=99999, num_topics=3000)
SWAP = 2


def setup(device):
    """The optimized C1 session: (buffers, model, goal names, seconds of the chain)."""
    goals = list(ccmi.DEFAULT_GOALS)
    buf = ccmi.RandomCluster.generate(**C1_PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf, device=device)
    bc = ccmi.BalancingConstraint()
    bc.set_resource_balance_percentage(1.05)
    t0 = time.perf_counter()
    ccmi.GoalOptimizer(bc).optimizations(cm, ccmi.goals_from_names(goals))
    return buf, cm, goals, time.perf_counter() - t0


def swap_replicas(cm, desc, n, brokers, seed):
    """n replicas of one random broker as sources and every replica of `brokers` other random brokers as candidates,
    both as [k, 2] int32 (partition, broker), and the hosting matrix [P, B]."""
    rs = np.random.RandomState(seed)
    B, P = desc.num_brokers, desc.num_partitions
    off = list(desc.partition_offset[:P + 1])
    dist = np.array(cm.replica_distribution())
    slot_part = np.repeat(np.arange(P), np.diff(off))
    hosts = np.zeros((P, B), dtype=bool)
    hosts[slot_part, dist] = True
    picked = [int(b) for b in rs.permutation(B)[:brokers + 1]]
    on = lambda b: np.stack([np.flatnonzero(hosts[:, b]), np.full(int(hosts[:, b].sum()), b)], axis=1)  # noqa: E731
    src = on(picked[0])
    src = src[np.sort(rs.choice(len(src), min(n, len(src)), replace=False))]
    cand = np.concatenate([on(b) for b in picked[1:]])
    return src.astype(np.int32), cand.astype(np.int32), hosts


def timed(cm, call):
    """(wall ms, kernel ms, launches, result) of one call; the call ends in a stream synchronise."""
    cm.reset_perf()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    p = cm.perf()
    return wall, p.accept_kernel_ms, p.accept_launches, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--brokers", type=int, default=8, help="candidate brokers")
    ap.add_argument("--repeats", type=int, default=101)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    buf, cm, goals, chain_s = setup(args.device)
    G = len(goals)
    src, cand, hosts = swap_replicas(cm, buf.desc, args.sources, args.brokers, 20261019)
    n, m = len(src), len(cand)

    # the cells legit both ways as K9 swap actions: what a caller without the grid call derives from its own model
    legit = cm.swaps_acceptance_grid([], src, cand)
    first = hosts[src[:, 0][:, None], cand[:, 1][None, :]]
    second = hosts[cand[:, 0][None, :], src[:, 1][:, None]]
    if not (legit == np.where(first, 3, np.where(second, 4, 0))).all():  # this cluster has no ineligible brokers
        sys.exit("the legitimacy grid does not follow the hosting matrix")
    rows, cols = np.nonzero(legit == 0)
    acts = np.full((len(rows), 7), -1, dtype=np.int32)
    acts[:, 0], acts[:, 1], acts[:, 2] = SWAP, src[rows, 0], src[rows, 1]
    acts[:, 3], acts[:, 4] = cand[cols, 1], cand[cols, 0]

    grid_call = lambda: cm.swaps_acceptance_grid(goals, src, cand)  # noqa: E731
    k9_call = lambda: cm.actions_acceptance(goals, acts)  # noqa: E731
    # the same answer both ways, which is also the warm-up of both (code object load, buffers)
    cm.set_kernel_timing(True)
    codes = grid_call()
    verdicts = k9_call()
    via_k9 = np.take_along_axis(verdicts, (verdicts != 0).argmax(axis=1)[:, None], axis=1)[:, 0]
    same = bool((codes[rows, cols] == via_k9).all()) and bool(((codes >= 3) == (legit >= 3)).all())
    for _ in range(3):
        grid_call()
        k9_call()

    g_wall, g_kern, k_wall, k_kern = [], [], [], []
    for _ in range(args.repeats):  # alternating, so both see the same machine
        w, k, g_launches, _ = timed(cm, grid_call)
        g_wall.append(w)
        g_kern.append(k)
        w, k, k_launches, _ = timed(cm, k9_call)
        k_wall.append(w)
        k_kern.append(k)
    cm.set_kernel_timing(False)

    med = statistics.median
    grid_cells, k9_cells = n * m * G, len(rows) * G
    out = dict(brokers=buf.desc.num_brokers, replicas=buf.desc.num_replicas, goals=G, sources=n, candidates=m,
               candidate_brokers=args.brokers, repeats=args.repeats, chain_s=round(chain_s, 3), same_answer=same,
               code_counts=np.bincount(codes.ravel(), minlength=5).tolist(),
               grid_pairs=n * m, grid_cells=grid_cells, grid_launches=int(g_launches),
               grid_call_ms=round(med(g_wall), 4), grid_call_ms_min_max=[round(min(g_wall), 4), round(max(g_wall), 4)],
               grid_kernel_ms=round(med(g_kern), 4),
               grid_in_bytes=n * 8 + m * 8, grid_out_bytes=n * m,
               k9_actions=len(rows), k9_cells=k9_cells, k9_launches=int(k_launches),
               k9_call_ms=round(med(k_wall), 4), k9_call_ms_min_max=[round(min(k_wall), 4), round(max(k_wall), 4)],
               k9_kernel_ms=round(med(k_kern), 4),
               k9_in_bytes=len(rows) * 28, k9_out_bytes=k9_cells,
               grid_ns_per_pair=round(med(g_wall) * 1e6 / (n * m), 3),
               k9_ns_per_pair=round(med(k_wall) * 1e6 / max(1, len(rows)), 3),
               call_speedup=round(med(k_wall) / med(g_wall), 2),
               kernel_ratio_grid_over_k9=round(med(g_kern) / med(k_kern), 2) if med(k_kern) > 0 else None)
    print(json.dumps(out))
    if not same:
        sys.exit("the grid and the per-action verdicts disagree")


if __name__ == "__main__":
    main()
