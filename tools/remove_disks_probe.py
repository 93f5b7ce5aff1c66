#!/usr/bin/env python3
"""Times the remove-disks operation at C4 size (10,000 brokers, 999,999 replicas, 4 x 75,000 MB logdirs per broker,
as bench.py --workload c4 generates it, with its BalancingConstraint: capacity threshold 0.8).

Per repeat, on fresh sessions of the same desc:
  * ccmi_session_mark_disks_for_removal of one logdir per broker, each broker's fullest (the C call: the admission
    check of every broker and the re-send of the disk tables with the new capacities);
  * one optimization with goal kind 24, IntraBrokerDiskCapacityGoal(true): the wall time of the call and the K6
    kernel time of intra_brokers from ccmi_perf (HIP events on the session stream), with intra_sort's apart;
  * for scale, a kind-16 optimization (IntraBrokerDiskCapacityGoal) of the unmarked desc on a fresh session.
A broker whose request fails the admission check is left out of the list (counted in `brokers_refused`). The medians
are printed as one JSON line.

    python tools/remove_disks_probe.py [--repeats K] [--device N]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
import ccmi  # noqa: E402

C4_PROPS = dict(num_racks=100, num_brokers=10000, num_replicas=999999, num_topics=10000, rack_aware=1,
                leader_in_first_position=1, jbod=2, num_logdirs=4, logdir_capacity=[75000.0] * 4)
THRESHOLD = 0.8


def constraint():
    bc = ccmi.BalancingConstraint()
    bc.max_replicas_per_broker = 2000
    bc.set_resource_balance_percentage(1.05)
    bc.set_capacity_threshold(THRESHOLD)
    return bc


def fullest_disks(cm):
    """Each broker's fullest logdir (disk_mb of ccmi_broker_stats' disk rows), as desc disk indices."""
    rows = cm.broker_stats().disks
    best = {}
    for d, (b, mb) in enumerate(zip(rows["broker"], rows["disk_mb"])):
        if int(b) not in best or mb > best[int(b)][0]:
            best[int(b)] = (mb, d)
    return [d for _, d in best.values()]


def optimize(cm, goal):
    cm.reset_perf()
    t0 = time.perf_counter()
    try:
        ccmi.GoalOptimizer(constraint()).optimizations(cm, ccmi.goals_from_names([goal]))
        outcome = "ok"
    except ccmi.OptimizationFailureException as e:
        outcome = str(e)[:160]
    wall = (time.perf_counter() - t0) * 1e3
    p = cm.perf()
    return wall, p.intra_kernel_ms, p.intra_sort_ms, len(cm.actions()), outcome


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    buf = ccmi.RandomCluster.generate(**C4_PROPS)
    lib = buf.lib
    if not lib.has_remove_disks:
        sys.exit(f"{lib.path} does not export ccmi_session_mark_disks_for_removal")
    first = ccmi.ClusterModel.from_buffers(buf, device=args.device)
    disks = fullest_disks(first)
    # the call is all or nothing: when the whole list is refused, find the refused brokers with one request each on
    # sessions of their own (each successful mark sends the disk tables again, so this is the slow way)
    whole = (C.c_int32 * max(1, len(disks)))(*disks)
    keep = disks
    if lib.lib.ccmi_session_mark_disks_for_removal(first.handle, whole, len(disks), THRESHOLD, None) != 0:
        one = (C.c_int32 * 1)()
        keep = []
        for d in disks:
            one[0] = d
            if lib.lib.ccmi_session_mark_disks_for_removal(first.handle, one, 1, THRESHOLD, None) == 0:
                keep.append(d)
    first.close()
    arr = (C.c_int32 * max(1, len(keep)))(*keep)
    mark, w24, k24, s24, w16, k16, s16 = [], [], [], [], [], [], []
    for _ in range(1 + args.repeats):  # the first round is the warm-up (code object load, allocations)
        cm = ccmi.ClusterModel.from_buffers(buf, device=args.device)
        cm.set_kernel_timing(True)
        t0 = time.perf_counter()
        lib.check(lib.lib.ccmi_session_mark_disks_for_removal(cm.handle, arr, len(keep), THRESHOLD, None))
        mark.append((time.perf_counter() - t0) * 1e3)
        w, k, s, actions24, outcome24 = optimize(cm, ccmi.REMOVE_DISKS_GOAL)
        w24.append(w), k24.append(k), s24.append(s)
        cm.close()
        cm = ccmi.ClusterModel.from_buffers(buf, device=args.device)
        cm.set_kernel_timing(True)
        w, k, s, actions16, outcome16 = optimize(cm, "IntraBrokerDiskCapacityGoal")
        w16.append(w), k16.append(k), s16.append(s)
        cm.close()
    med = lambda xs: round(statistics.median(xs[1:]), 4)  # noqa: E731
    print(json.dumps(dict(
        config="c4", brokers=C4_PROPS["num_brokers"], replicas=buf.desc.num_replicas, repeats=args.repeats,
        disks_marked=len(keep), brokers_refused=len(disks) - len(keep), mark_ms=med(mark),
        kind24_call_ms=med(w24), kind24_k6_kernel_ms=med(k24), kind24_sort_ms=med(s24), kind24_actions=actions24,
        kind24_outcome=outcome24, kind16_call_ms=med(w16), kind16_k6_kernel_ms=med(k16), kind16_sort_ms=med(s16),
        kind16_actions=actions16, kind16_outcome=outcome16)), flush=True)


if __name__ == "__main__":
    main()
