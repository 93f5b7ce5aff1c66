"""What the tests and the probe of ccmi_builder_populate_from_aggregator share: seeded partition topologies with the
sample batches that make a chosen number of entities rows of the aggregate, the features of such a case found on the CPU
(with the restatement of the aggregator, metric_aggregator_support), the parent path (aggregate() and one
ccmi_builder_populate_partition per row) and an exact snapshot of a builder's desc."""
import ctypes as C
import random

import numpy as np

import ccmi
import metric_aggregator_support as S

CAP = {"CPU": 100.0, "NW_IN": 1e6, "NW_OUT": 1e6, "DISK": 1e7}
NUM_BROKERS = 12
DEAD = (4, 9)             # created alive=False (handleDeadBroker) and marked DEAD afterwards
JBOD = (2, 5)             # brokers with logdirs
LOGDIRS = ("/d0", "/d1")
FNS = [f for _, f in ccmi.KAFKA_COMMON_METRICS]
PICK = [[n for n, _ in ccmi.KAFKA_COMMON_METRICS].index(m) for m in ccmi.LoadMonitorModel.METRICS]
BYTE_RATES = (2, 3, 7, 8)  # the aggregator metrics behind the four byte rates of the builder
ALL_TIME = (-1, S.LONG_MAX)
# no extrapolation allowed: an entity is a row iff it has a sample in every window of the range
OPTIONS = dict(min_valid_entity_ratio=0.0, min_valid_entity_group_ratio=0.0, min_valid_windows=1,
               max_allowed_extrapolations_per_entity=0, granularity=ccmi.GRANULARITY_ENTITY)


class Case:
    """A topology of E partitions, `rows` of which are sampled in every one of the W windows, a few only in the
    current window (present, never valid) and a few never (absent). A partition has an empty replica range with
    probability p_skip, and is offline with the same."""

    def __init__(self, seed, rows, W, max_rf=8, extra=5, topics=None, p_skip=0.06):
        rng = random.Random(seed)
        self.W, self.rows = W, rows
        E = self.E = rows + extra
        others = set(rng.sample(range(E), extra))
        self.row_entities = [e for e in range(E) if e not in others]
        others = sorted(others)
        self.late, self.absent = others[:extra - extra // 2], others[extra - extra // 2:]
        T = topics or max(2, min(40, E // 6))
        self.topic_names = ["topic%d" % t for t in range(T)]
        self.partition_topic = [rng.randrange(T) for _ in range(E)]
        seen = [0] * T
        self.partition_number = []
        for t in self.partition_topic:
            self.partition_number.append(seen[t])
            seen[t] += 1
        self.replica_offset, self.replica_broker_id, self.leader_broker_id = [0], [], []
        self.replica_offline, self.replica_logdir = [], []
        for e in range(E):
            n = 0 if rng.random() < p_skip else rng.randint(1, max_rf)
            reps = rng.sample(range(NUM_BROKERS), n)
            self.replica_broker_id += reps
            self.replica_offset.append(len(self.replica_broker_id))
            self.leader_broker_id.append(-1 if n == 0 or rng.random() < p_skip else reps[rng.randrange(n)])
            self.replica_offline += [1 if rng.random() < 0.1 else 0 for _ in reps]
            self.replica_logdir += [rng.randrange(len(LOGDIRS)) if b in JBOD else -1 for b in reps]
        # the samples: one batch per window 1..W, then the current window W + 1
        self.batches = []
        zero = set(e for e in self.row_entities if rng.random() < 0.08)
        unreported = set(e for e in self.row_entities if rng.random() < 0.2)
        nrng = np.random.default_rng(seed)
        for w in range(1, W + 2):
            ents = np.array(self.row_entities if w <= W else self.late + self.row_entities[:3], dtype=np.int32)
            vals = nrng.uniform(0.0, 50.0, (len(ents), len(FNS)))
            vals[:, 0] = nrng.uniform(0.0, 0.02, len(ents))  # CPU_USAGE is a unit interval
            for i, e in enumerate(ents.tolist()):
                if e in zero:
                    vals[i, list(BYTE_RATES)] = 0.0
                elif e in unreported:
                    vals[i, 8] = 0.0
            times = (w - 1) * S.WINDOW_MS + nrng.integers(0, S.WINDOW_MS, len(ents))
            order = nrng.permutation(len(ents))
            self.batches.append((ents[order], times[order], vals[order]))

    def topology(self, **override):
        kw = dict(topic_names=self.topic_names, partition_topic=self.partition_topic,
                  partition_number=self.partition_number, replica_offset=self.replica_offset,
                  replica_broker_id=self.replica_broker_id, leader_broker_id=self.leader_broker_id,
                  replica_offline=self.replica_offline, replica_logdir=self.replica_logdir, logdir_names=LOGDIRS)
        kw.update(override)
        return ccmi.PartitionTopology(**kw)

    def replicas(self, e):
        return self.replica_broker_id[self.replica_offset[e]:self.replica_offset[e + 1]]

    def kept(self, e):
        """populatePartitionLoad creates replicas for partition e (given that e is a row)."""
        return len(self.replicas(e)) > 0 and self.leader_broker_id[e] >= 0

    def aggregator(self, lib):
        agg = ccmi.MetricSampleAggregator(self.W, S.WINDOW_MS, 1, FNS, self.partition_topic, len(self.topic_names),
                                          lib=lib)
        for ents, times, vals in self.batches:
            agg.add_samples(ents, times, vals)
        return agg

    def restatement(self):
        ref = S.MetricSampleAggregator(self.W, S.WINDOW_MS, 1, FNS, self.partition_topic)
        for ents, times, vals in self.batches:
            ref.add_samples(ents.tolist(), times.tolist(), vals.tolist())
        return ref

    def features(self):
        """Found on the CPU alone: the rows by the restatement, the rest from the topology."""
        ref = self.restatement()
        comp = ref.completeness(*ALL_TIME, S.AggregationOptions(0.0, 0.0, 1, 0, S.ENTITY, False))
        rows = sorted(int(e) for e in comp.valid_entities)
        busy = set()  # entities with a nonzero byte rate in some sample of the aggregated windows
        for ents, _, vals in self.batches[:self.W]:
            busy |= set(ents[vals[:, list(BYTE_RATES)].any(axis=1)].tolist())
        f = dict(rows=len(rows), windows=len(comp.valid_window_indices))
        f["rows_are_the_sampled"] = rows == self.row_entities
        row_set = set(rows)
        f["not_a_row"] = any(e not in row_set for e in ref.raw) and len(self.absent) > 0
        f["empty_range"] = any(not self.replicas(e) for e in rows)
        f["offline"] = any(self.replicas(e) and self.leader_broker_id[e] < 0 for e in rows)
        before = after = zero_bytes = False
        for e in rows:
            if not self.kept(e):
                continue
            reps = self.replicas(e)
            at = reps.index(self.leader_broker_id[e])
            before |= at > 0
            after |= at < len(reps) - 1
            zero_bytes |= e not in busy
        f["follower_before_leader"], f["follower_after_leader"], f["zero_bytes"] = before, after, zero_bytes
        first_of_topic, kept_seen, late_first = {}, set(), False
        for e in range(self.E):
            t = self.partition_topic[e]
            first_of_topic.setdefault(t, e)
            if e in row_set and self.kept(e) and t not in kept_seen:
                kept_seen.add(t)
                late_first |= first_of_topic[t] != e
        f["topic_first_kept_is_not_its_first"] = late_first
        return f


def new_model(lib, W):
    """The brokers of every case: 12 in 3 racks, two created dead, two with logdirs."""
    m = ccmi.LoadMonitorModel(num_windows=W, lib=lib)
    order = list(range(NUM_BROKERS))
    random.Random(W).shuffle(order)
    for b in order:
        m.create_broker("rack%d" % (b % 3), "h%d" % b, b, CAP, alive=b not in DEAD,
                        disk_capacity_by_logdir={d: 5e6 for d in LOGDIRS} if b in JBOD else None)
    return m


def finish_model(m):
    for b in DEAD:
        m.set_broker_state(b, "DEAD")
    return m


def options(include_invalid=False, **kw):
    o = dict(OPTIONS)
    o.update(kw)
    return ccmi.AggregationOptions(include_invalid_entities=include_invalid, **o)


def populate_per_row(model, res, topo):
    """The parent path's second half: one ccmi_builder_populate_partition per row of `res`, ascending entities, with
    the row's six leader metrics. The same call LoadMonitorModel.populate_partition makes, without its list handling.
    Stops at the first error, as a loop over populate_partition does."""
    lib = model.lib
    wv = res.values.shape[2] if len(res.entities) else 0
    lead = np.ascontiguousarray(res.values[:, PICK, :], dtype=np.float32) if len(res.entities) else None
    names = [n.encode() for n in topo.topic_names]
    logdirs = [n.encode() for n in topo.logdir_names]
    off = topo.replica_offset
    fn = lib.lib.ccmi_builder_populate_partition
    model._desc = None
    for row, e in enumerate(res.entities.tolist()):
        o0, n = int(off[e]), int(off[e + 1] - off[e])
        if n == 0:
            continue  # partitionInfo == null: LoadMonitor skips the partition
        ld = None
        if topo.replica_logdir is not None:
            ld = (C.c_char_p * n)(*[logdirs[i] if i >= 0 else None for i in topo.replica_logdir[o0:o0 + n].tolist()])
        lib.check(fn(model.handle, names[topo.partition_topic[e]], int(topo.partition_number[e]),
                     topo.replica_broker_id[o0:].ctypes.data_as(C.POINTER(C.c_int32)), n, int(topo.leader_broker_id[e]),
                     None if topo.replica_offline is None
                     else topo.replica_offline[o0:].ctypes.data_as(C.POINTER(C.c_uint8)),
                     ld, lead[row].ctypes.data_as(C.POINTER(C.c_float))))
    assert wv in (0, model.W)


def snapshot(model):
    """Every field of the builder's desc, the broker ids and the topic names, as comparable values; floats as bits."""
    d = model.desc()

    def arr(p, n, dtype):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype).copy() if n and p else np.zeros(0, dtype=dtype)

    B, P, R, D, W = d.num_brokers, d.num_partitions, d.num_replicas, d.num_disks, d.num_windows
    s = dict(num_windows=W, num_racks=d.num_racks, num_brokers=B, num_topics=d.num_topics, num_partitions=P,
             num_replicas=R, num_disks=D, num_disk_assignments=d.num_disk_assignments,
             num_replica_loads=d.num_replica_loads, replica_load_order=bool(d.replica_load_order),
             broker_ids=model.broker_ids(),
             topic_names=[d.topic_names[t].decode() for t in range(d.num_topics)],
             disk_logdir=[d.disk_logdir[i].decode() for i in range(D)])
    for name, n, dtype in (("broker_id", B, np.int32), ("broker_rack", B, np.int32), ("broker_state", B, np.int32),
                           ("broker_host", B, np.int32), ("partition_topic", P, np.int32),
                           ("partition_number", P, np.int32), ("partition_offset", P + 1, np.int32),
                           ("partition_replicas", R, np.int32), ("replica_partition", R, np.int32),
                           ("replica_broker", R, np.int32), ("replica_is_leader", R, np.uint8),
                           ("replica_offline", R, np.uint8), ("disk_broker", D, np.int32),
                           ("replica_disk", R if D else 0, np.int32), ("disk_demoted", D, np.uint8)):
        s[name] = arr(getattr(d, name), n, dtype).tolist()
    s["broker_capacity"] = arr(d.broker_capacity, B * 4, np.float64).view(np.uint64).tolist()
    s["disk_capacity"] = arr(d.disk_capacity, D, np.float64).view(np.uint64).tolist()
    s["replica_load"] = arr(d.replica_load, R * 6 * W, np.float32).view(np.uint32)
    return s


def assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        if k == "replica_load":
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
        else:
            assert got[k] == want[k], k


def loads_of(model):
    d = model.desc()
    n = d.num_replicas * 6 * d.num_windows
    return np.ctypeslib.as_array(d.replica_load, shape=(n,)).copy() if n else np.zeros(0, dtype=np.float32)
