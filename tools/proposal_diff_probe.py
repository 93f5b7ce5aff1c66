#!/usr/bin/env python3
"""Times ccmi_proposal_diff at C1 and C2 size against the host path of the same session.

Two sessions: C1 (1000 brokers, 99,999 replicas) and C2 (10,000 brokers, 999,999 replicas) as bench.py generates them,
each after the 16 default goals under the default BalancingConstraint, so the diff has the proposals of a real
optimization. After a warm-up (code object load, the initial placement, the buffers) each call is repeated --repeats
times. Printed per size, as one JSON line: the medians of the wall time of the C call with capacity 0 (summary only:
one stream synchronise, 64 bytes back) and with room for every record (two synchronises and the rows back), and of
K14's HIP-event time (the launches of kernels/proposal_diff.hip between two events on the session stream, read from
stats_kernel_ms).

The baseline is the host path on the same session: ccmi_session_apply with zero actions, which is exactly one
buildProposals (the O(P) rebuild every apply, goal and optimization ends with), then ccmi_proposals and
ccmi_proposal_disks into buffers allocated once. Before anything is timed the two answers must be equal, proposal by
proposal, and the summary must equal OptimizerResult.movement_stats over the host's list.

    python tools/proposal_diff_probe.py [--repeats K] [--sizes c1,c2]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
import ccmi  # noqa: E402

SIZES = {"c1": dict(num_racks=20, num_brokers=1000, num_replicas=99999, num_topics=3000),
         "c2": dict(num_racks=100, num_brokers=10000, num_replicas=999999, num_topics=10000)}
MAX_RF = 8


class DeviceCall:
    """The C call itself on a buffer allocated once (ClusterModel.proposal_diff adds the Python conversions)."""

    def __init__(self, cm, capacity):
        self.cm, self.capacity = cm, capacity
        self.records = np.zeros(max(1, capacity), dtype=np.dtype(ccmi.ProposalRecordStruct))
        self.n, self.summary = C.c_int64(0), ccmi.ProposalSummaryStruct()

    def __call__(self):
        cm = self.cm
        cm.lib.check(cm.lib.lib.ccmi_proposal_diff(cm.handle, self.records.ctypes.data if self.capacity else None,
                                                   self.capacity, C.byref(self.n), C.byref(self.summary)))


class HostCall:
    """One buildProposals (ccmi_session_apply of no action), then the two copies out of the host's list."""

    def __init__(self, cm, n):
        self.cm = cm
        self.none = (ccmi.ActionStruct * 1)()
        self.done = C.c_int64(0)
        self.part, self.size, self.old_leader = (np.zeros(max(1, n), dtype=np.int32) for _ in range(3))
        self.old_r, self.new_r, self.old_d, self.new_d = (np.zeros(max(1, n) * MAX_RF, dtype=np.int32) for _ in range(4))

    def __call__(self):
        cm, L, i32 = self.cm, self.cm.lib.lib, C.POINTER(C.c_int32)
        p = lambda a: a.ctypes.data_as(i32)  # noqa: E731
        cm.lib.check(L.ccmi_session_apply(cm.handle, self.none, 0, C.byref(self.done)))
        cm.lib.check(L.ccmi_proposals(cm.handle, MAX_RF, p(self.part), p(self.size), p(self.old_leader), p(self.old_r),
                                      p(self.new_r)))
        cm.lib.check(L.ccmi_proposal_disks(cm.handle, MAX_RF, p(self.old_d), p(self.new_d)))


def same_answer(dev, host, n):
    r = dev.records[:n]
    return bool(dev.n.value == n and np.array_equal(r["partition"], host.part[:n]) and
                np.array_equal(r["size"], host.size[:n]) and np.array_equal(r["old_leader"], host.old_leader[:n]) and
                np.array_equal(r["old_replicas"].ravel(), host.old_r[:n * MAX_RF]) and
                np.array_equal(r["new_replicas"].ravel(), host.new_r[:n * MAX_RF]) and
                np.array_equal(r["old_disks"].ravel(), host.old_d[:n * MAX_RF]) and
                np.array_equal(r["new_disks"].ravel(), host.new_d[:n * MAX_RF]))


def timed(cm, call):
    cm.reset_perf()
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    p = cm.perf()
    return wall, p.stats_kernel_ms, p.stats_launches


def measure(name, props, repeats, device):
    buf = ccmi.RandomCluster.generate(**props)
    cm = ccmi.ClusterModel.from_buffers(buf, device=device)
    t0 = time.perf_counter()
    res = ccmi.GoalOptimizer(ccmi.BalancingConstraint()).optimizations(cm, ccmi.goals_from_names(list(ccmi.DEFAULT_GOALS)))
    chain_s = time.perf_counter() - t0
    cm.set_kernel_timing(True)
    n = cm.lib.lib.ccmi_proposal_count(cm.handle)
    only, full, host = DeviceCall(cm, 0), DeviceCall(cm, n), HostCall(cm, n)
    first_ms, _, _ = timed(cm, full)  # the first call of the session also uploads and allocates
    host()
    only()
    s = full.summary
    stats = [s.num_inter_broker_replica_movements, s.inter_broker_data_to_move_mb, s.num_intra_broker_replica_movements,
             s.intra_broker_data_to_move_mb, s.num_leadership_movements]
    same = (same_answer(full, host, n) and s.num_proposals == n and bytes(only.summary) == bytes(s) and
            stats == res.movement_stats())
    med = statistics.median
    out = dict(config=name, partitions=buf.desc.num_partitions, replicas=buf.desc.num_replicas, proposals=int(n),
               movement_stats=[int(x) for x in stats], chain_s=round(chain_s, 2), repeats=repeats,
               first_call_ms=round(first_ms, 3), out_bytes=160 * int(n), same_answer=bool(same))
    for label, call in (("summary_only", only), ("all_records", full)):
        for _ in range(3):
            timed(cm, call)
        wall, kern = [], []
        for _ in range(repeats):
            w, k, launches = timed(cm, call)
            wall.append(w)
            kern.append(k)
        out[label] = dict(call_ms=round(med(wall), 4), call_ms_min_max=[round(min(wall), 4), round(max(wall), 4)],
                          kernel_ms=round(med(kern), 4), launches=int(launches))
    base = []
    for _ in range(max(5, repeats // 5)):
        t0 = time.perf_counter()
        host()
        base.append((time.perf_counter() - t0) * 1e3)
    out["host_path_ms"] = round(med(base), 4)
    out["host_path_ms_min_max"] = [round(min(base), 4), round(max(base), 4)]
    full()
    out["same_answer"] = bool(same and same_answer(full, host, n))
    print(json.dumps(out), flush=True)
    if not out["same_answer"]:
        sys.exit("the device and the host path gave different proposals or statistics")
    cm.set_kernel_timing(False)
    cm.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=101)
    ap.add_argument("--sizes", default="c1,c2")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    for size in args.sizes.split(","):
        measure(size, SIZES[size], args.repeats, args.device)


if __name__ == "__main__":
    main()
