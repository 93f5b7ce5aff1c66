#!/usr/bin/env python3
"""Times ccmi_partition_load (ClusterModel.partition_load) at C1 and C2 size against a host answer.

Two fresh sessions: C1 (1000 brokers, 99,999 replicas) and C2 (10,000 brokers, 999,999 replicas) as bench.py generates
them. The tables a fresh session holds are the ones a session holds after a chain, so no chain is run. The query is the
default one (DISK, no max / avg, every topic, partition and broker, no tie ranks), once for every record
(entries = 2^31 - 1) and once for entries = 100. After a warm-up (code object load, the static partition numbers, the
sort buffers) each call is repeated --repeats times; the medians of the wall time of the C call (it ends in two stream
synchronises and one device-to-host copy of the returned rows) and of K13's HIP-event time (the launches of
kernels/partition_load.hip between two events on the session stream, read from stats_kernel_ms) are printed as one JSON
line per configuration.

The baseline is a host answer in the same process: the same keys computed with numpy from the desc (the leader's
latest DISK window as a double, Math.max(x, 0.0)), then np.lexsort on (partition, -key) and the cut; its order must
equal the product's before anything is timed. It builds no records, so it is a lower bound of a host implementation.

    python tools/partition_load_probe.py [--repeats K] [--sizes c1,c2]
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
ALL = 2 ** 31 - 1
M_DISK = 1


class Call:
    """The C call itself on a buffer allocated once (ClusterModel.partition_load adds the Python conversions)."""

    def __init__(self, cm, entries):
        self.cm = cm
        self.q = ccmi.PartitionLoadQueryStruct()
        self.q.resource = ccmi.RESOURCES.index("DISK")
        self.q.entries = entries
        self.q.partition_lower, self.q.partition_upper = -2 ** 31, 2 ** 31 - 1
        self.records = np.zeros(min(entries, cm.desc.num_partitions), dtype=np.dtype(ccmi.PartitionLoadRecordStruct))
        self.nrec, self.nsel = C.c_int64(0), C.c_int64(0)

    def __call__(self):
        cm = self.cm
        cm.lib.check(cm.lib.lib.ccmi_partition_load(cm.handle, C.byref(self.q), self.records.ctypes.data,
                                                    C.byref(self.nrec), C.byref(self.nsel)))

    def order(self):
        return self.records["partition"][:self.nrec.value]


class HostAnswer:
    """The leader's latest DISK window per partition, gathered once (the desc does not change); per call the key
    array, the lexsort and the cut."""

    def __init__(self, desc):
        R, P, W = desc.num_replicas, desc.num_partitions, desc.num_windows
        load = np.ctypeslib.as_array(desc.replica_load, shape=(R, 6, W))
        part = np.ctypeslib.as_array(desc.replica_partition, shape=(R,))
        lead = np.flatnonzero(np.ctypeslib.as_array(desc.replica_is_leader, shape=(R,)))
        self.latest = np.zeros(P, dtype=np.float32)
        self.latest[part[lead]] = load[lead, M_DISK, 0]
        self.index = np.arange(P)

    def __call__(self, entries):
        key = np.maximum(self.latest.astype(np.float64), 0.0)
        return np.lexsort((self.index, -key))[:entries]


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
    host = HostAnswer(buf.desc)
    d = buf.desc
    med = statistics.median
    for label, entries in (("all", ALL), ("100", 100)):
        call = Call(cm, entries)
        first_ms, _, _ = timed(cm, call)  # the first call of the session also uploads and allocates
        first = call.records.tobytes()
        same_order = bool(np.array_equal(call.order(), host(entries)))
        for _ in range(3):
            timed(cm, call)
        wall, kern, base = [], [], []
        for _ in range(repeats):
            w, k, launches = timed(cm, call)
            wall.append(w)
            kern.append(k)
        for _ in range(max(3, repeats // 10)):
            t0 = time.perf_counter()
            host(entries)
            base.append((time.perf_counter() - t0) * 1e3)
        same = call.records.tobytes() == first
        out = dict(config=name, entries=label, partitions=d.num_partitions, replicas=d.num_replicas, repeats=repeats,
                   first_call_ms=round(first_ms, 3), call_ms=round(med(wall), 4),
                   call_ms_min_max=[round(min(wall), 4), round(max(wall), 4)], kernel_ms=round(med(kern), 4),
                   launches=int(launches), records=int(call.nrec.value), selected=int(call.nsel.value),
                   out_bytes=80 * int(call.nrec.value), host_lexsort_ms=round(med(base), 3),
                   same_answer=same, same_order_as_host=same_order)
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
