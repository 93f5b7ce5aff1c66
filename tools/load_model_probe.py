#!/usr/bin/env python3
"""Times ccmi_builder_populate_from_aggregator (K18) against the parent path at C2's shape: about 340,000 partitions at
RF 3 on 10,000 brokers, W = 5 windows, M = 9 (KafkaMetricDef's common metrics).

Six windows are fed (five stable ones and the current one), one sample of every partition each, so every partition is a
row of the aggregate. The parent path is MetricSampleAggregator.aggregate() followed by the
AggregationResult.populate_partition loop, one interpreter round trip per partition; next to it the same loop as bare
ccmi_builder_populate_partition calls on prepared buffers, which is what a shim's per-partition downcall costs at best.
The bulk call runs --repeats times, each on a fresh builder; the split of the median call is the library's own
(HIP events on the aggregator's stream for the kernels and copies, the host clock for the rest). Before a number is
reported the builders of the three paths must hold identical descs, replica loads compared as bit patterns.

    python tools/load_model_probe.py [--partitions P] [--brokers B] [--repeats K] [--skip-python-loop]
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

W, WINDOW_MS, RF = 5, 300_000, 3
LONG_MAX = (1 << 63) - 1
HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X
CAP = {"CPU": 100.0, "NW_IN": 1e7, "NW_OUT": 1e7, "DISK": 1e9}
FNS = [f for _, f in ccmi.KAFKA_COMMON_METRICS]
PICK = [[n for n, _ in ccmi.KAFKA_COMMON_METRICS].index(m) for m in ccmi.LoadMonitorModel.METRICS]


def new_model(lib, brokers):
    m = ccmi.LoadMonitorModel(num_windows=W, lib=lib)
    for b in range(brokers):
        m.create_broker("rack%d" % (b % 50), "h%d" % b, b, CAP)
    return m


def desc_arrays(m):
    d = m.desc()
    P, R = d.num_partitions, d.num_replicas

    def arr(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy()

    out = dict(partition_topic=arr(d.partition_topic, P), partition_number=arr(d.partition_number, P),
               partition_offset=arr(d.partition_offset, P + 1), replica_partition=arr(d.replica_partition, R),
               replica_broker=arr(d.replica_broker, R), replica_is_leader=arr(d.replica_is_leader, R),
               replica_offline=arr(d.replica_offline, R),
               replica_load=arr(d.replica_load, R * 6 * d.num_windows).view(np.uint32))
    out["topic_names"] = np.array([d.topic_names[t] for t in range(d.num_topics)])
    out["shape"] = np.array([d.num_windows, d.num_brokers, d.num_topics, P, R, d.num_disks])
    return out


def same(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partitions", type=int, default=340_000)
    ap.add_argument("--brokers", type=int, default=10_000)
    ap.add_argument("--topics", type=int, default=30_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-python-loop", action="store_true", help="leave out the populate_partition loop (slow)")
    args = ap.parse_args()
    P, B, T = args.partitions, args.brokers, args.topics
    lib = ccmi.Library.get()
    rng = np.random.default_rng(18)

    # the topology: RF 3 on distinct brokers, the leader anywhere among them, 2 % offline replicas
    topic = rng.integers(0, T, P).astype(np.int32)
    number = np.zeros(P, dtype=np.int32)
    order = np.argsort(topic, kind="stable")
    starts = np.r_[0, np.flatnonzero(np.diff(topic[order])) + 1]
    number[order] = np.arange(P) - np.repeat(starts, np.diff(np.r_[starts, P]))
    first = rng.integers(0, B, P)
    step = rng.integers(1, B // 3, (P, RF - 1)).cumsum(axis=1)
    brokers = np.c_[first, (first[:, None] + step) % B].astype(np.int32)  # distinct: the steps sum to less than B
    leader = brokers[np.arange(P), rng.integers(0, RF, P)].astype(np.int32)
    topo = ccmi.PartitionTopology(["topic%d" % t for t in range(T)], topic, number, np.arange(P + 1) * RF,
                                  brokers.reshape(-1), leader, replica_offline=rng.random(P * RF) < 0.02)

    agg = ccmi.MetricSampleAggregator(W, WINDOW_MS, 1, FNS, topic, T, lib=lib)
    ents = np.arange(P, dtype=np.int32)
    for w in range(W + 1):
        vals = rng.uniform(0.0, 5e4, (P, len(FNS)))
        vals[:, 0] = rng.uniform(0.0, 0.01, P)
        vals[rng.random(P) < 0.2, 8] = 0.0  # replication bytes out not reported
        agg.add_samples(ents, w * WINDOW_MS + rng.integers(0, WINDOW_MS, P), vals)
    o = ccmi.AggregationOptions(0.0, 0.0, 1, 0, ccmi.GRANULARITY_ENTITY, False)

    # ---- the parent path
    agg.aggregate(-1, LONG_MAX, o)  # warm-up: buffers
    agg_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = agg.aggregate(-1, LONG_MAX, o)
        agg_ms.append((time.perf_counter() - t0) * 1e3)
    assert res.num_entities == P and res.values.shape == (P, len(FNS), W)
    names = topo.topic_names
    python_loop_s = None
    if not args.skip_python_loop:
        per_row = new_model(lib, B)
        reps, leaders = brokers.tolist(), leader.tolist()
        off = topo.replica_offline.reshape(P, RF)
        t0 = time.perf_counter()
        for row, e in enumerate(res.entities.tolist()):
            res.populate_partition(per_row, row, names[topic[e]], int(number[e]), reps[e], leaders[e],
                                   offline=[b for b, f in zip(reps[e], off[e]) if f])
        python_loop_s = time.perf_counter() - t0
    bare = new_model(lib, B)
    lead = np.ascontiguousarray(res.values[:, PICK, :], dtype=np.float32)
    enc = [n.encode() for n in names]
    fn, handle = lib.lib.ccmi_builder_populate_partition, bare.handle
    i32p, u8p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    flat, offl = topo.replica_broker_id, topo.replica_offline
    t0 = time.perf_counter()
    for row, e in enumerate(res.entities.tolist()):
        lib.check(fn(handle, enc[topic[e]], int(number[e]), flat[e * RF:].ctypes.data_as(i32p), RF, int(leader[e]),
                     offl[e * RF:].ctypes.data_as(u8p), None, lead[row].ctypes.data_as(f32p)))
    bare_loop_s = time.perf_counter() - t0
    want = desc_arrays(bare)
    if python_loop_s is not None:
        assert same(desc_arrays(per_row), want), "the two per-row loops disagree"
        del per_row

    # ---- the bulk call
    split = (C.c_double * 8)()
    calls = []
    for i in range(args.repeats + 1):  # the first call sizes the buffers
        m = new_model(lib, B)
        t0 = time.perf_counter()
        c = m.populate_from_aggregator(agg, -1, LONG_MAX, o, topo)
        ms = (time.perf_counter() - t0) * 1e3
        lib.check(lib.lib.ccmi_load_model_timing(agg.handle, split))
        if i:
            calls.append((ms, list(split)))
        if i == args.repeats:
            assert (c.num_rows, c.num_populated) == (P, P)
            assert same(desc_arrays(m), want), "the bulk call's desc differs from the per-row loop's"
    calls.sort(key=lambda x: x[0])
    ms, s = calls[len(calls) // 2]
    R = P * RF
    out_bytes = R * 6 * W * 4
    algo_bytes = out_bytes + R * 8 + P * 6 * W * 4  # the loads, a descriptor per replica, the six picked rows
    result = {
        "partitions": P, "replicas": R, "brokers": B, "topics": T, "windows": W, "metrics": len(FNS),
        "aggregate_ms": round(statistics.median(agg_ms), 3),
        "per_row_python_loop_s": None if python_loop_s is None else round(python_loop_s, 3),
        "per_row_bare_calls_s": round(bare_loop_s, 3),
        "bulk_call_ms": round(ms, 3),
        "bulk_split_ms": {"aggregate_host_clock": round(s[0], 3), "rows_kernel_tail_and_topology_upload": round(s[1], 3),
                          "classify_and_offsets": round(s[2], 3), "columns": round(s[3], 3),
                          "load_values": round(s[4], 3), "copies_back": round(s[5], 3),
                          "host_checks_and_append": round(s[6], 3), "c_call": round(s[7], 3)},
        "load_values_output_bytes": out_bytes,
        "load_values_output_fraction_of_hbm_peak": round(out_bytes / (s[4] * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
        "load_values_algorithmic_fraction_of_hbm_peak": round(algo_bytes / (s[4] * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
        "speedup_over_python_loop": None if python_loop_s is None
        else round((statistics.median(agg_ms) * 1e-3 + python_loop_s) / (ms * 1e-3), 1),
        "speedup_over_bare_calls": round((statistics.median(agg_ms) * 1e-3 + bare_loop_s) / (ms * 1e-3), 1),
        "descs_identical": True,
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
