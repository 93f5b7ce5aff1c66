#!/usr/bin/env python3
"""Times ccmi_execution_plan (ClusterModel.execution_plan) at C1 and C2 size against a host sort of the same keys.

Two sessions: C1 (1000 brokers, 99,999 replicas) and C2 (10,000 brokers, 999,999 replicas) as bench.py generates them,
each after the 16 default goals under the default BalancingConstraint, so the plan is the one of a real proposal set.
The chain is PostponeUrp, then PrioritizeLarge, then Base, with a seeded random partition_state and no proposal_rank.
Two forms of the call: the sizing call (all capacities 0: classify and scan only) and the full call (every list). After
a warm-up (code object load, the initial placement, the scratch buffers) each is repeated --repeats times; the medians
of the wall time of the C call (it ends in one or two stream synchronises and the device-to-host copies) and of K16's
HIP-event time (the launches of kernels/execution_plan.hip between events on the session stream, read from
stats_kernel_ms) are printed as one JSON line per form.

The baseline is a host answer in the same process from the records ccmi_proposal_diff returns (fetched once, outside
the timing): numpy picks the inter-broker tasks, numbers them, builds one (broker, class, size, id) row per list entry
(the old leader and every added broker), np.lexsort orders them, a bincount gives the offsets, and a second lexsort
over (first task's key, -length, broker) the broker order. Its lists, offsets and broker order must equal the product's
before anything is timed. It builds no task table and no leadership list, so it is a lower bound of a host
implementation (the JVM inserts into one TreeSet per broker through a chained comparator).

    python tools/execution_plan_probe.py [--repeats K] [--sizes c1,c2]
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
CHAIN = (ccmi.STRATEGY_POSTPONE_URP, ccmi.STRATEGY_PRIORITIZE_LARGE, ccmi.STRATEGY_BASE)


class Call:
    """The C call itself on buffers allocated once (ClusterModel.execution_plan adds the Python conversions)."""

    def __init__(self, cm, state, sizes):
        self.cm = cm
        B = self.B = cm.desc.num_brokers
        q = self.q = ccmi.ExecutionPlanQueryStruct()
        q.num_strategies = len(CHAIN)
        for i in range(4):
            q.strategies[i] = CHAIN[i] if i < len(CHAIN) else -1
        self.state = state
        q.partition_state = state.ctypes.data_as(C.POINTER(C.c_uint8))
        self.summary = ccmi.PlanSummaryStruct()
        self.inter_off, self.intra_off = np.zeros(B + 1, dtype=np.int64), np.zeros(B + 1, dtype=np.int64)
        self.caps = sizes or (0, 0, 0, 0)
        self.tasks = np.zeros(self.caps[0], dtype=np.dtype(ccmi.PlanTaskStruct))
        self.inter, self.intra = np.zeros(self.caps[1], dtype=np.int32), np.zeros(self.caps[2], dtype=np.int32)
        self.leaders, self.order = np.zeros(self.caps[3], dtype=np.int32), np.zeros(B, dtype=np.int32)

    def __call__(self):
        def ptr(a):
            return a.ctypes.data if len(a) else None

        cm = self.cm
        cm.lib.check(cm.lib.lib.ccmi_execution_plan(
            cm.handle, C.byref(self.q), C.byref(self.summary), ptr(self.tasks), self.caps[0],
            self.inter_off.ctypes.data, ptr(self.inter), self.caps[1], self.order.ctypes.data if self.caps[1] else None,
            self.intra_off.ctypes.data, ptr(self.intra), self.caps[2], ptr(self.leaders), self.caps[3]))


class HostAnswer:
    """The inter-broker lists and the broker order from proposal_diff's records (no disks: a default-goal chain)."""

    def __init__(self, records, state, B):
        self.r, self.state, self.B = records, state, B

    def __call__(self):
        r, B = self.r, self.B
        old, new = r["old_replicas"], r["new_replicas"]
        task = (old != new).any(axis=1)  # the broker sequence changed
        old, new, part = old[task], new[task], r["partition"][task]
        added = (new >= 0) & ~(new[:, :, None] == old[:, None, :]).any(axis=2)
        data = added.sum(axis=1).astype(np.int64) * r["size"][task].astype(np.int64)
        n = len(part)
        ids = np.arange(n, dtype=np.int64)  # records come in partition order: the order of a NULL proposal_rank
        urp = (self.state[part] & ccmi.PSTATE_UNDER_REPLICATED) != 0
        rows, cols = np.nonzero(added)
        broker = np.concatenate((r["old_leader"][task].astype(np.int64), new[rows, cols].astype(np.int64)))
        entry = np.concatenate((ids, rows.astype(np.int64)))
        order = np.lexsort((entry, -data[entry], urp[entry], broker))
        lists = entry[order]
        lens = np.bincount(broker, minlength=B)
        offsets = np.concatenate(([0], np.cumsum(lens)))
        have = np.flatnonzero(lens)
        first = lists[offsets[have]]
        brokers = have[np.lexsort((have, -lens[have], first, -data[first], urp[first]))]
        return lists, offsets, brokers


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
    ccmi.GoalOptimizer(ccmi.BalancingConstraint()).optimizations(cm, ccmi.goals_from_names(list(ccmi.DEFAULT_GOALS)))
    chain_s = time.perf_counter() - t0
    cm.set_kernel_timing(True)
    d = buf.desc
    state = np.random.default_rng(20261020).integers(0, 16, size=d.num_partitions).astype(np.uint8)
    records = cm.proposal_diff().records
    host = HostAnswer(records, state, d.num_brokers)
    med = statistics.median
    sizing = Call(cm, state, None)
    first_ms, _, _ = timed(cm, sizing)  # the first call of the session also uploads and allocates
    s = sizing.summary
    sizes = (int(s.num_inter_tasks), int(s.num_inter_entries), int(s.num_intra_tasks), int(s.num_leader_tasks))
    for label, call in (("sizing", sizing), ("full", Call(cm, state, sizes))):
        timed(cm, call)
        lists, offsets, brokers = host()
        same_order = bool(np.array_equal(call.inter_off, offsets))
        if label == "full":
            first = call.inter.tobytes()
            same_order = same_order and bool(np.array_equal(call.inter, lists)) \
                and bool(np.array_equal(call.order[:len(brokers)], brokers)) and bool((call.order[len(brokers):] == -1).all())
        for _ in range(3):
            timed(cm, call)
        wall, kern, base = [], [], []
        for _ in range(repeats):
            w, k, launches = timed(cm, call)
            wall.append(w)
            kern.append(k)
        for _ in range(max(3, repeats // 10)):
            t0 = time.perf_counter()
            host()
            base.append((time.perf_counter() - t0) * 1e3)
        same = label != "full" or call.inter.tobytes() == first
        lens = np.diff(call.inter_off)
        out = dict(config=name, form=label, brokers=d.num_brokers, partitions=d.num_partitions, repeats=repeats,
                   chain_s=round(chain_s, 2), proposals=len(records), first_call_ms=round(first_ms, 3),
                   call_ms=round(med(wall), 4), call_ms_min_max=[round(min(wall), 4), round(max(wall), 4)],
                   kernel_ms=round(med(kern), 4), launches=int(launches), inter_tasks=sizes[0], inter_entries=sizes[1],
                   leader_tasks=sizes[3], longest_segment=int(lens.max()), brokers_with_tasks=int(s.num_brokers_with_tasks),
                   host_lexsort_ms=round(med(base), 3), same_answer=same, same_order_as_host=same_order)
        print(json.dumps(out), flush=True)
        if not same or not same_order:
            sys.exit("a repeated call gave another answer, or the host answer another order")
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
