"""The reference of the partition load tests: a restatement of PartitionLoadRunnable.getResult on per-replica loads.

The oracle has no per-replica load accessor, so the expected records are computed here: per-replica float32 windows and
double running sums taken from desc.replica_load, the oracle's action log replayed on them, the value rules of
Load.expectedUtilizationFor(resource, wantMaxLoad, wantAvgLoad), and Python's sorted on (-key, rank, partition).

Replay: a move or a swap only relabels replicas. A LEADERSHIP action applies Replica.makeFollower to the source replica
(loadops.h ldMakeFollower) and adds the delta (CPU, LEADER_BYTES_OUT, REPLICATION_BYTES_OUT) to the destination replica
unless that replica's load is empty (Load.addLoad), every step in the float / double operations of loadops.h: a window
value is a float32, `a.v[i] = (float)((double)a.v[i] + d)`, a running sum a double. test_partition_load_reference.py
pins this restatement to the oracle's broker utilization.
"""
import re

import numpy as np

import ccmi

CPU, NW_IN, NW_OUT, DISK = 0, 1, 2, 3
M_CPU, M_DISK, M_LBI, M_LBO, M_RBI, M_RBO = range(6)
MOVE, LEADERSHIP, SWAP = 0, 1, 2
DEFAULT, MAX, AVG = 0, 1, 2
MODES = {DEFAULT: {}, MAX: dict(max_load=True), AVG: dict(avg_load=True)}
METRICS = {CPU: (M_CPU,), DISK: (M_DISK,), NW_IN: (M_LBI, M_RBI), NW_OUT: (M_LBO, M_RBO)}
FLOAT_MIN = 2.0 ** -149  # Float.MIN_VALUE
RECORD = np.dtype(ccmi.PartitionLoadRecordStruct)
f32 = np.float32


def jmax0(x):
    """Math.max(x, 0.0)."""
    return x if x != x else (x if x > 0.0 else 0.0)


class Window:
    """loadops.h Window: float32 values (newest first) and the double running sum."""

    def __init__(self, values):
        self.v = [f32(x) for x in values]
        self.sum = 0.0
        for x in self.v:
            self.sum += float(x)

    @staticmethod
    def zero(W):
        return Window([0.0] * W)

    def add(self, other):  # ldAdd
        for i, x in enumerate(other.v):
            d = float(x)
            self.v[i] = f32(float(self.v[i]) + d)
            self.sum += d

    def set(self, i, x):  # ldSet
        self.sum += x - float(self.v[i])
        self.v[i] = f32(x)

    def avg(self):  # ldAvg
        return f32(self.sum / len(self.v))


class _Loads:
    """Replica id -> its six Windows."""

    def __init__(self, raw, loaded, W):
        self.raw, self.loaded, self.W, self.made = raw, loaded, W, {}

    def __getitem__(self, r):
        if r not in self.made:
            self.made[r] = [Window(self.raw[r, k]) if r in self.loaded else Window.zero(self.W) for k in range(6)]
        return self.made[r]


class Restatement:
    def __init__(self, desc):
        B, P, R, W = desc.num_brokers, desc.num_partitions, desc.num_replicas, desc.num_windows
        self.B, self.P, self.R, self.W = B, P, R, W
        self.topics = [desc.topic_names[t].decode() for t in range(desc.num_topics)]
        self.topic = list(desc.partition_topic[:P])
        self.number = list(desc.partition_number[:P])
        raw = np.array(desc.replica_load[:R * 6 * W], dtype=np.float32).reshape(R, 6, W)
        loaded = set(range(R))
        if desc.replica_load_order and desc.num_replica_loads > 0:
            loaded = set(desc.replica_load_order[:desc.num_replica_loads])
        # an empty load keeps zeroed windows (LoadVec's) and is told apart by `has`; a replica's windows are built when
        # first read (most followers never are)
        self.load = _Loads(raw, loaded, W)
        self.has = [r in loaded for r in range(R)]
        self.abs_nw_out = float(np.abs(raw[sorted(loaded)][:, [M_LBO, M_RBO]].astype(np.float64)).sum())
        self.broker = list(desc.replica_broker[:R])
        off = list(desc.partition_offset[:P + 1])
        self.slots = [list(desc.partition_replicas[off[p]:off[p + 1]]) for p in range(P)]
        self.leader = [-1] * P
        for r in range(R):
            if desc.replica_is_leader[r]:
                self.leader[desc.replica_partition[r]] = r
        self.where = {(desc.replica_partition[r], self.broker[r]): r for r in range(R)}
        self.leaderships = 0

    # ------------------------------------------------------------------------------------------- replay
    def _relabel(self, r, p, src, dst):
        assert self.where.pop((p, src)) == r
        self.where[(p, dst)] = r
        self.broker[r] = dst

    def _make_follower(self, L):  # ldMakeFollower
        W = self.W
        tot_out, tot_in, chg = Window.zero(W), Window.zero(W), Window.zero(W)
        tot_out.add(L[M_LBO])
        tot_out.add(L[M_RBO])
        tot_in.add(L[M_LBI])
        tot_in.add(L[M_RBI])
        for i in range(W):
            n, out, c = float(tot_in.v[i]), float(tot_out.v[i]), float(L[M_CPU].v[i])
            follower = 0.0 if n == 0.0 and out == 0.0 else c * (0.15 * n) / (0.7 * n + 0.15 * out)
            chg.set(i, float(L[M_CPU].v[i]) - follower)
            L[M_CPU].set(i, follower)
        delta = {M_CPU: Window.zero(W), M_LBO: Window.zero(W), M_RBO: Window.zero(W)}
        delta[M_CPU].add(chg)
        delta[M_LBO].add(L[M_LBO])
        delta[M_RBO].add(L[M_RBO])
        L[M_LBO], L[M_RBO] = Window.zero(W), Window.zero(W)
        return delta

    def apply(self, actions):
        for typ, p, src, dst, dp, _, _ in actions:
            if typ == MOVE:
                self._relabel(self.where[(p, src)], p, src, dst)
            elif typ == SWAP:
                a, b = self.where[(p, src)], self.where[(dp, dst)]
                self._relabel(a, p, src, dst)
                self._relabel(b, dp, dst, src)
            elif typ == LEADERSHIP:
                sr, dr = self.where[(p, src)], self.where[(p, dst)]
                assert self.leader[p] == sr
                delta = self._make_follower(self.load[sr])
                if self.has[dr]:
                    for k, w in delta.items():
                        self.load[dr][k].add(w)
                # Partition.relocateLeadership: positions 0 and indexOf(dr) swap, wherever the old leader sits (a
                # model whose leader is not its partition's first replica keeps it elsewhere)
                s = self.slots[p]
                j = s.index(dr)
                s[0], s[j] = s[j], s[0]
                self.leader[p] = dr
                self.leaderships += 1
        return self

    # ------------------------------------------------------------------------------------------- values
    def term(self, w, mode, latest):
        if mode == MAX:
            mx = w.v[0]
            for x in w.v[1:]:
                mx = x if x > mx else mx
            return float(mx) if mx > 0 else FLOAT_MIN  # Math.max(Float.MIN_VALUE, max_i v[i])
        if latest and mode == DEFAULT:
            return float(w.v[0])
        return float(w.avg())

    def util(self, p, res, mode):
        r = self.leader[p]
        if not self.has[r]:
            return 0.0
        acc = 0.0
        for k in METRICS[res]:
            acc += self.term(self.load[r][k], mode, res == DISK)
        return jmax0(acc)

    def keys(self, res, mode):
        return [self.util(p, res, mode) for p in range(self.P)]

    def brokers(self, p):
        """The leader's broker, then Partition.followers(): _replicas order without the leader."""
        lead = self.leader[p]
        return [self.broker[lead]] + [self.broker[r] for r in self.slots[p] if r != lead]

    # ------------------------------------------------------------------------------------------- the response
    def selected(self, topic=None, partition_range=None, broker_index=None):
        pat = re.compile(topic) if topic is not None else None
        lo, hi = partition_range if partition_range is not None else (-2 ** 31, 2 ** 31 - 1)
        keep = []
        for p in range(self.P):
            if pat is not None and not pat.fullmatch(self.topics[self.topic[p]]):
                continue
            if not lo <= self.number[p] <= hi:
                continue
            if broker_index and not any(self.broker[r] in broker_index for r in self.slots[p]):
                continue
            keep.append(p)
        return keep

    def order(self, res, mode, tie_rank=None, keep=None):
        key = self.keys(res, mode)
        rank = list(range(self.P)) if tie_rank is None else [int(x) for x in tie_rank]
        return sorted(range(self.P) if keep is None else keep, key=lambda p: (-key[p], rank[p], p))

    def records(self, order, mode):
        out = np.zeros(len(order), dtype=RECORD)
        for i, p in enumerate(order):
            out["util"][i] = [self.util(p, res, mode) for res in range(4)]
            out["partition"][i] = p
            b = self.brokers(p)
            out["num_replicas"][i] = len(b)
            out["brokers"][i] = b + [-1] * (8 - len(b))
        return out

    def expected(self, res, mode, tie_rank=None, entries=2 ** 31 - 1, **selection):
        """(records, num_selected) of the response."""
        keep = self.selected(**selection) if selection else None
        order = self.order(res, mode, tie_rank, keep)
        return self.records(order[:entries], mode), len(order)


def assert_same(state, want, num_selected):
    """The product's PartitionLoadState against (records, num_selected) of the restatement, byte for byte."""
    assert state.num_selected == num_selected
    got = state.records
    assert len(got) == len(want)
    if got.tobytes() != want.tobytes():
        for i in range(len(want)):
            assert got[i].tobytes() == want[i].tobytes(), (i, got[i], want[i])
