#!/usr/bin/env python3
"""Times ccmi_moves_acceptance_mask against ccmi_actions_acceptance on one session, for the same question.

A C1-size session (1000 brokers, 99,999 replicas, 3000 topics, as tools/accept_probe.py) optimizes the 16 default goals.
The question is a replica-move loop's: for 64 source replicas, which brokers are legit and accepted by all 16 goals —
64 x 1000 x 16 cells. It is answered, in the same process on the same session,
  * by one ClusterModel.moves_acceptance_mask call (kernels/accept_mask.hip): 64 sources in, 64 x 16 words out, and
  * by one ClusterModel.actions_acceptance call (kernels/accept.hip) on the legit cells of those sources, one action per
    (source, legit broker) pair, which the caller then ANDs down per action. Building the action list is not timed.
After a warm-up of both, the two calls alternate for --repeats rounds; the medians of the wall times (each call ends in
a stream synchronise) and of the kernels' HIP-event times (accept_kernel_ms) are printed as one JSON line, with both
per-cell figures over the cells each call stands for. The answers are compared before anything is timed.

    python tools/mask_probe.py [--sources N] [--repeats K]
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
MOVE = 0


def move_sources(cm, desc, n, seed):
    """n random replicas as (MOVE, partition, broker) sources, and the hosting matrix rows of their partitions."""
    rs = np.random.RandomState(seed)
    B, P = desc.num_brokers, desc.num_partitions
    off = list(desc.partition_offset[:P + 1])
    dist = cm.replica_distribution()
    slot_part = np.repeat(np.arange(P), np.diff(off))
    sources, hosted = [], np.zeros((n, B), dtype=bool)
    for i in range(n):
        slot = int(rs.randint(len(dist)))
        p = int(slot_part[slot])
        sources.append((MOVE, p, dist[slot]))
        hosted[i, dist[off[p]:off[p + 1]]] = True
    return sources, hosted


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
    ap.add_argument("--repeats", type=int, default=101)
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
    B, G, n = buf.desc.num_brokers, len(goals), args.sources
    sources, hosted = move_sources(cm, buf.desc, n, 20261019)
    src = np.array(sources, dtype=np.int32)

    # the legit cells as K9 actions: the pure legit mask is what a caller without the mask call derives from its own model
    legit = cm.moves_acceptance_mask([], src)
    if not (legit == ~hosted).all():  # this cluster has no ineligible brokers
        sys.exit("the legit mask is not the complement of the hosting matrix")
    rows, cols = np.nonzero(legit)
    acts = np.full((len(rows), 7), -1, dtype=np.int32)
    acts[:, 0], acts[:, 1], acts[:, 2], acts[:, 3] = MOVE, src[rows, 1], src[rows, 2], cols

    mask_call = lambda: cm.moves_acceptance_mask(goals, src, packed=True)  # noqa: E731
    k9_call = lambda: cm.actions_acceptance(goals, acts)  # noqa: E731
    # the same answer both ways, which is also the warm-up of both (code object load, buffers)
    cm.set_kernel_timing(True)
    mask = cm.moves_acceptance_mask(goals, src)
    via_k9 = np.zeros((n, B), dtype=bool)
    via_k9[rows, cols] = (k9_call() == 0).all(axis=1)
    same = bool((mask == via_k9).all())
    for _ in range(3):
        mask_call()
        k9_call()

    m_wall, m_kern, k_wall, k_kern = [], [], [], []
    for _ in range(args.repeats):  # alternating, so both see the same machine
        w, k, m_launches, _ = timed(cm, mask_call)
        m_wall.append(w)
        m_kern.append(k)
        w, k, k_launches, _ = timed(cm, k9_call)
        k_wall.append(w)
        k_kern.append(k)
    cm.set_kernel_timing(False)

    med = statistics.median
    mask_cells, k9_cells = n * B * G, len(rows) * G
    out = dict(brokers=B, replicas=buf.desc.num_replicas, goals=G, sources=n, repeats=args.repeats,
               chain_s=round(chain_s, 3), same_answer=same, accepted_bits=int(mask.sum()),
               mask_cells=mask_cells, mask_launches=int(m_launches),
               mask_call_ms=round(med(m_wall), 4), mask_call_ms_min_max=[round(min(m_wall), 4), round(max(m_wall), 4)],
               mask_kernel_ms=round(med(m_kern), 4),
               mask_in_bytes=n * 16, mask_out_bytes=n * ((B + 63) // 64) * 8,
               k9_actions=len(rows), k9_cells=k9_cells, k9_launches=int(k_launches),
               k9_call_ms=round(med(k_wall), 4), k9_call_ms_min_max=[round(min(k_wall), 4), round(max(k_wall), 4)],
               k9_kernel_ms=round(med(k_kern), 4),
               k9_in_bytes=len(rows) * 28, k9_out_bytes=k9_cells,
               mask_ns_per_cell=round(med(m_wall) * 1e6 / mask_cells, 3),
               k9_ns_per_cell=round(med(k_wall) * 1e6 / k9_cells, 3),
               call_speedup=round(med(k_wall) / med(m_wall), 2),
               kernel_ratio_mask_over_k9=round(med(m_kern) / med(k_kern), 2) if med(k_kern) > 0 else None)
    print(json.dumps(out))
    if not same:
        sys.exit("the mask and the per-action verdicts disagree")


if __name__ == "__main__":
    main()
