#!/usr/bin/env python3
"""Times one sampling round of ccmi.MetricsProcessor (K20) at C2's shape, generated on the host.

Shape: 10,000 brokers, 340,000 partitions at RF 3 over 30,000 topics. Every broker reports its 55 broker-scope types
once, the seven topic-scope types once per topic it hosts a replica of, and one PARTITION_SIZE per replica it hosts:
about 1.0 M partition records, 7 M topic records and 550,000 broker records, shuffled into one arrival order.

Measured, as medians over --repeats rounds after a warm-up (each round: clear, add_metrics, process):
  device add_metrics            : the upload of the columns (the topic names are interned on the host)
  device process                : the samples come back as rows
  device process_into           : the rows go to a partition and a broker aggregator on the device
  host numpy grouping           : the holder reduction alone, vectorised: a stable argsort of the same 64-bit keys and a
                                  segmented sum (np.add.reduceat); it does not build the samples
Before anything is timed the round must give 340,000 partition samples and 10,000 broker samples, the brokers' CPU
values must come back unchanged, and diskUsage must equal the numpy per-broker sum to 1e-9 relative (the device adds in
the HashMap's order, numpy in key order). The sort's traffic is priced as passes x 2 x 16 B x records against the
process time, as bytes per second.

    python tools/metrics_processor_probe.py [--repeats K] [--brokers B] [--partitions P] [--topics T]
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

TOPIC_TYPES = np.array([2, 3, 11, 12, 13, 14, 15], dtype=np.uint8)
BROKER_TYPES = np.array([t for t in range(63) if t != 4 and t not in TOPIC_TYPES.tolist()], dtype=np.uint8)


def generate(rng, B, P, T, rf=3):
    topic_of = rng.integers(0, T, P).astype(np.int32)
    order = np.argsort(topic_of, kind="stable")
    number = np.empty(P, dtype=np.int32)
    starts = np.searchsorted(topic_of[order], np.arange(T))
    number[order] = (np.arange(P) - starts[topic_of[order]]).astype(np.int32)
    first = rng.integers(0, B, P)
    replicas = (first[:, None] + np.arange(rf)[None, :] * (B // rf + 1)) % B  # rf distinct brokers
    leader = replicas[:, 0].astype(np.int32)
    # PARTITION_SIZE per replica
    rb = replicas.reshape(-1).astype(np.int32)
    rt = np.repeat(topic_of, rf)
    rp = np.repeat(number, rf)
    cols = [(np.full(rb.size, 4, np.uint8), rb, rng.uniform(1e6, 1e10, rb.size), rt, rp)]
    # topic types per distinct (broker, topic)
    pairs = np.unique(rb.astype(np.int64) * T + rt)
    pb, pt = (pairs // T).astype(np.int32), (pairs % T).astype(np.int32)
    for t in TOPIC_TYPES:
        cols.append((np.full(pb.size, t, np.uint8), pb, rng.uniform(1e3, 1e7, pb.size), pt, np.full(pb.size, -1, np.int32)))
    for t in BROKER_TYPES:
        v = rng.uniform(1.0, 90.0, B) if t == 5 else rng.uniform(1e3, 1e8, B)
        cols.append((np.full(B, t, np.uint8), np.arange(B, dtype=np.int32), v, np.full(B, -1, np.int32),
                     np.full(B, -1, np.int32)))
    ty, br, va, to, pa = (np.concatenate([c[i] for c in cols]) for i in range(5))
    perm = rng.permutation(ty.size)
    ty, br, va, to, pa = ty[perm], br[perm], va[perm], to[perm], pa[perm]
    tm = rng.integers(1_000_000, 1_060_000, ty.size).astype(np.int64)
    names = ["topic-%05d" % i for i in range(T)]
    cluster = (names, topic_of, number, np.arange(P + 1, dtype=np.int32) * rf, leader)
    return (ty, br, tm, va, to, pa, names), cluster


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brokers", type=int, default=10_000)
    ap.add_argument("--partitions", type=int, default=340_000)
    ap.add_argument("--topics", type=int, default=30_000)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    records, cluster = generate(rng, a.brokers, a.partitions, a.topics)
    ty, br, tm, va, to, pa, names = records
    n, B, P = int(ty.size), a.brokers, a.partitions
    node_ids, cores = np.arange(B, dtype=np.int32), np.full(B, 16.0)
    mp = ccmi.MetricsProcessor()

    mp.add_metrics(*records)
    s = mp.process(*cluster, node_ids, cores)
    assert (s.num_partition_samples, s.num_broker_samples) == (P, B), (s.num_partition_samples, s.num_broker_samples)
    cpu = np.zeros(B)
    cpu[br[ty == 5]] = va[ty == 5]
    assert np.array_equal(s.broker_values[:, 0], cpu)
    disk = np.bincount(br[ty == 4], weights=va[ty == 4], minlength=B) / (1024 * 1024)
    assert np.allclose(s.broker_values[:, 1], disk, rtol=1e-9, atol=0.0)
    fallback = s.num_hash_fallback_brokers

    def add():
        mp.clear()
        mp.add_metrics(*records)

    def round_process():
        add()
        mp.process(*cluster, node_ids, cores)

    fns9 = [f for _, f in ccmi.KAFKA_COMMON_METRICS]
    part = ccmi.MetricSampleAggregator(5, 300_000, 1, fns9, cluster[1], num_groups=a.topics)
    brok = ccmi.MetricSampleAggregator(5, 300_000, 1, fns9 + [ccmi.AGG_AVG] * 47, np.arange(B, dtype=np.int32))

    def round_into():
        add()
        mp.process_into(*cluster, node_ids, cores, part, brok)

    def numpy_grouping():
        key = (br.astype(np.uint64) << np.uint64(46)) | ((to + 1).astype(np.uint64) << np.uint64(24)) | \
              ((pa + 1).astype(np.uint64) << np.uint64(6)) | ty.astype(np.uint64)
        order = np.argsort(key, kind="stable")
        k = key[order]
        heads = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
        sums = np.add.reduceat(va[order], heads)
        return sums / np.diff(np.concatenate((heads, [n])))

    out = {"brokers": B, "partitions": P, "topics": a.topics, "records": n, "repeats": a.repeats,
           "partition_samples": s.num_partition_samples, "broker_samples": s.num_broker_samples,
           "hash_fallback_brokers": fallback,
           "device_add_metrics": timed(add, a.repeats),
           "device_add_metrics_process": timed(round_process, a.repeats),
           "device_add_metrics_process_into": timed(round_into, a.repeats),
           "host_numpy_grouping": timed(numpy_grouping, max(1, a.repeats // 2))}
    passes = (46 + int(B).bit_length() + 7) // 8
    process_ms = out["device_add_metrics_process"]["ms"] - out["device_add_metrics"]["ms"]
    out["sort_passes"] = passes
    out["process_only_ms"] = round(process_ms, 3)
    out["sort_traffic_gb"] = round(passes * 2 * 16 * n / 1e9, 3)
    out["sort_traffic_over_process_gb_per_s"] = round(passes * 2 * 16 * n / 1e9 / (process_ms / 1e3), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
