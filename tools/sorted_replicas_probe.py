#!/usr/bin/env python3
"""Times ccmi_sorted_replicas (ClusterModel.sorted_replicas) for every broker at C1 and C2 size against a host sort.

Two fresh sessions: C1 (1000 brokers, 99,999 replicas) and C2 (10,000 brokers, 999,999 replicas) as bench.py generates
them. The tables a fresh session holds are the ones a session holds after a chain, so no chain is run. The query is the
capacity goals' Spec: both priority functions (offline, then immigrants), the reversed DISK score, no selection, every
broker. Three forms of the call: the sizing call (capacity 0: keys, counts and offsets only), every record, and every
record with its score. After a warm-up (code object load, the static tail ranks, the scratch buffers) each call is
repeated --repeats times; the medians of the wall time of the C call (it ends in two stream synchronises and the
device-to-host copies of the offsets and the rows) and of K15's HIP-event time (the launches of
kernels/sorted_replicas.hip between events on the session stream, read from stats_kernel_ms) are printed as one JSON
line per form.

The baseline is a host answer in the same process: the same 64-bit keys built with numpy from the desc (the score's
float bits in Double.compare order, the online bit, the rank of Replica.compareTo's tail, which is computed once, as the
session uploads it once), then np.lexsort on (key, broker) and the offsets from a bincount. Its order must equal the
product's before anything is timed. It builds no records, so it is a lower bound of a host implementation.

    python tools/sorted_replicas_probe.py [--repeats K] [--sizes c1,c2]
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
M_DISK = 1


class Call:
    """The C call itself on buffers allocated once (ClusterModel.sorted_replicas adds the Python conversions)."""

    def __init__(self, cm, records, scores):
        self.cm = cm
        B, R = cm.desc.num_brokers, cm.desc.num_replicas
        q = self.q = ccmi.SortedReplicasQueryStruct()
        q.num_priorities = 2
        q.priorities[0], q.priorities[1] = 0, 1
        q.score_resource, q.score_reverse = ccmi.RESOURCES.index("DISK"), 1
        q.above_resource = q.below_resource = -1
        self.B = B
        self.offsets = np.zeros(B + 1, dtype=np.int64)
        self.records = np.zeros((R, 2), dtype=np.int32) if records else None
        self.scores = np.zeros(R, dtype=np.float64) if scores else None
        self.capacity = R if records else 0
        self.total, self.bad = C.c_int64(0), C.c_int64(-1)

    def __call__(self):
        cm = self.cm
        cm.lib.check(cm.lib.lib.ccmi_sorted_replicas(
            cm.handle, C.byref(self.q), None, self.B, self.offsets.ctypes.data,
            None if self.records is None else self.records.ctypes.data,
            None if self.scores is None else self.scores.ctypes.data, self.capacity, C.byref(self.total),
            C.byref(self.bad)))


class HostAnswer:
    """What does not change is gathered once: the tail rank, the DISK score bits, the brokers. Per call the keys, the
    lexsort and the offsets. A fresh random cluster has no offline replica and no immigrant: every priority bit and the
    online bit are set, as the device sets them."""

    def __init__(self, desc, names):
        R, B, W = desc.num_replicas, desc.num_brokers, desc.num_windows
        self.B = B
        load = np.ctypeslib.as_array(desc.replica_load, shape=(R, 6, W))
        self.part = np.ctypeslib.as_array(desc.replica_partition, shape=(R,)).copy()
        self.broker = np.ctypeslib.as_array(desc.replica_broker, shape=(R,)).astype(np.int64)
        P, T = desc.num_partitions, desc.num_topics
        number = np.ctypeslib.as_array(desc.partition_number, shape=(P,))[self.part]
        topic = np.ctypeslib.as_array(desc.partition_topic, shape=(P,))[self.part]
        ids = np.ctypeslib.as_array(desc.broker_id, shape=(B,))[self.broker]
        trank = np.empty(T, dtype=np.int64)
        trank[np.argsort(np.array([n.encode("utf-16-be") for n in names], dtype=object), kind="stable")] = np.arange(T)
        order = np.lexsort((trank[topic], ids, number))
        self.static = np.empty(R, dtype=np.uint64)
        self.static[order] = np.arange(R, dtype=np.uint64)  # no two replicas share the tuple: the rank is dense
        avg = (load[:, M_DISK, :].astype(np.float64).sum(axis=1) / W).astype(np.float32)
        self.bits = avg.view(np.uint32)

    def __call__(self):
        neg = (self.bits & np.uint32(0x80000000)) != 0
        u = np.where(neg, ~self.bits, self.bits | np.uint32(0x80000000))
        u = ~u  # the reversed score
        key = (np.uint64(3) << np.uint64(62)) | (u.astype(np.uint64) << np.uint64(30)) | (np.uint64(1) << np.uint64(29))
        key |= self.static
        order = np.lexsort((key, self.broker))
        offsets = np.concatenate(([0], np.cumsum(np.bincount(self.broker, minlength=self.B))))
        return order, offsets


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
    cm.set_kernel_timing(True)
    d = buf.desc
    host = HostAnswer(d, cm.topic_names())
    med = statistics.median
    for label, records, scores in (("sizing", False, False), ("records", True, False), ("records+scores", True, True)):
        call = Call(cm, records, scores)
        first_ms, _, _ = timed(cm, call)  # the first call of the session also uploads and allocates
        order, offsets = host()
        same_order = bool(np.array_equal(call.offsets, offsets))
        if records:
            first = call.records.tobytes()
            same_order = same_order and bool(np.array_equal(call.records[:, 0], host.part[order])) \
                and bool(np.array_equal(call.records[:, 1], host.broker[order]))
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
        same = not records or call.records.tobytes() == first
        lens = np.diff(call.offsets)
        out = dict(config=name, form=label, brokers=d.num_brokers, replicas=d.num_replicas, repeats=repeats,
                   first_call_ms=round(first_ms, 3), call_ms=round(med(wall), 4),
                   call_ms_min_max=[round(min(wall), 4), round(max(wall), 4)], kernel_ms=round(med(kern), 4),
                   launches=int(launches), records=int(call.total.value), longest_segment=int(lens.max()),
                   out_bytes=(8 * d.num_brokers + 8)
                   + (8 + (8 if scores else 0)) * (int(call.total.value) if records else 0),
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
