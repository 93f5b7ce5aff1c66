"""The reference of the sorted replicas tests: an independent restatement of SortedReplicas on per-replica state.

Model state: partition_load_support.Restatement (per-replica float32 windows and double running sums from the desc, the
oracle's action log replayed on them with the makeFollower / makeLeader load rules) gives every replica's current
broker, load and leadership; this module adds the original broker (the desc's), original-offline (the desc's flag, or a
dead original broker: Replica.isOriginalOffline) and current-offline (Replica.isCurrentOffline: original-offline while
still on the original broker, or on a dead broker).

The comparator is written from SortedReplicas.java:75-90 and Replica.compareTo (Replica.java:350-377) as a
functools.cmp_to_key over tuples (priorities..., score, offline, partition number, original broker id, topic name): the
priority functions by Integer.compare in list order, the score by Double.compare (written out below: -0.0 < 0.0), then
compareTo. The selections are ReplicaSortFunctionFactory's lambdas. Nothing here packs a key.
"""
import functools
import struct

import numpy as np

from partition_load_support import (CPU, DISK, M_CPU, M_DISK, M_LBI, M_LBO, M_RBI, M_RBO, NW_IN, NW_OUT, Restatement,
                                    Window, jmax0)

DEAD = 1  # ccmi_broker_state
PRIO = {"offline": 0, "immigrants": 1, 0: 0, 1: 1}
RES = {"CPU": CPU, "NW_IN": NW_IN, "NW_OUT": NW_OUT, "DISK": DISK, 0: 0, 1: 1, 2: 2, 3: 3}


def double_bits(x):
    """Double.doubleToLongBits as a signed long."""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def double_compare(a, b):
    """Double.compare (Double.java): <, >, then the long bits, so -0.0 < 0.0. NaN is outside the contract."""
    if a < b:
        return -1
    if a > b:
        return 1
    x, y = double_bits(a), double_bits(b)
    return 0 if x == y else (-1 if x < y else 1)


def integer_compare(a, b):
    return -1 if a < b else (1 if a > b else 0)


def string_compare(a, b):
    """String.compareTo: by UTF-16 code unit, then by length."""
    x, y = a.encode("utf-16-be"), b.encode("utf-16-be")
    return -1 if x < y else (1 if x > y else 0)


def replica_compare_to(a, b):
    """Replica.compareTo on the tail (offline, partition number, original broker id, topic name)."""
    (off1, part1, orig1, topic1), (off2, part2, orig2, topic2) = a, b
    if off1 and not off2:
        return -1
    if not off1 and off2:
        return 1
    if part1 != part2:
        return 1 if part1 > part2 else -1
    if orig1 != orig2:
        return 1 if orig1 > orig2 else -1
    return string_compare(topic1, topic2)


def comparator(num_priorities, has_score):
    """SortedReplicas._replicaComparator over tuples (priorities..., score, offline, number, original id, topic)."""
    def compare(t1, t2):
        for i in range(num_priorities):  # comparePriority
            c = integer_compare(t1[i], t2[i])
            if c:
                return c
        if has_score:
            c = double_compare(t1[num_priorities], t2[num_priorities])
            if c:
                return c
        return replica_compare_to(t1[num_priorities + 1:num_priorities + 5], t2[num_priorities + 1:num_priorities + 5])
    return compare


def sort_tuples(tuples, num_priorities, has_score):
    return sorted(tuples, key=functools.cmp_to_key(comparator(num_priorities, has_score)))


class SortedModel:
    """Per-replica state of a model and the lists SortedReplicas would hold."""

    def __init__(self, desc):
        self.rs = Restatement(desc)
        rs = self.rs
        self.B, self.R = rs.B, rs.R
        self.part = list(desc.replica_partition[:rs.R])
        self.orig = list(desc.replica_broker[:rs.R])
        self.ids = list(desc.broker_id[:rs.B])
        self.dead = [desc.broker_state[b] == DEAD for b in range(rs.B)]
        self.orig_offline = [bool(desc.replica_offline[r]) or self.dead[self.orig[r]] for r in range(rs.R)]
        self._scores = {}

    def apply(self, actions):
        self.rs.apply(actions)
        self._scores = {}
        return self

    # ------------------------------------------------------------------------------------------- replica state
    def broker(self, r):
        return self.rs.broker[r]

    def is_leader(self, r):
        return self.rs.leader[self.part[r]] == r

    def immigrant(self, r):
        return self.orig[r] != self.rs.broker[r]

    def current_offline(self, r):
        b = self.rs.broker[r]
        return (self.orig_offline[r] and b == self.orig[r]) or self.dead[b]

    def topic(self, r):
        return self.rs.topics[self.rs.topic[self.part[r]]]

    def group_avg(self, r, res):
        """(double) valuesForGroup(resource group).avg(): a float32 widened; an empty load scores 0."""
        key = (r, res)
        if key not in self._scores:
            if not self.rs.has[r]:
                v = 0.0
            else:
                L = self.rs.load[r]
                if res == CPU:
                    v = float(L[M_CPU].avg())
                elif res == DISK:
                    v = float(L[M_DISK].avg())
                else:
                    acc = Window.zero(self.rs.W)
                    acc.add(L[M_LBI if res == NW_IN else M_LBO])
                    acc.add(L[M_RBI if res == NW_IN else M_RBO])
                    v = float(acc.avg())
            self._scores[key] = v
        return self._scores[key]

    def util(self, r, res):
        """Replica.load().expectedUtilizationFor(res)."""
        if not self.rs.has[r]:
            return 0.0
        L = self.rs.load[r]
        acc = 0.0
        if res == CPU:
            acc += float(L[M_CPU].avg())
        elif res == DISK:
            acc += float(L[M_DISK].v[0])
        else:
            acc += float(L[M_LBI if res == NW_IN else M_LBO].avg())
            acc += float(L[M_RBI if res == NW_IN else M_RBO].avg())
        return jmax0(acc)

    def replicas_of(self, b):
        return [r for r in range(self.R) if self.rs.broker[r] == b]

    # ------------------------------------------------------------------------------------------- the lists
    def selected(self, r, leaders=False, followers=False, online=False, offline=False, immigrants=False,
                 immigrant_or_offline=False, above=None, below=None, excluded_topics=None, included_topics=None, **_):
        """ReplicaSortFunctionFactory's selection functions, all of them."""
        if leaders and not self.is_leader(r):
            return False
        if followers and self.is_leader(r):
            return False
        if online and self.current_offline(r):
            return False
        if offline and not self.current_offline(r):
            return False
        if immigrants and not self.immigrant(r):
            return False
        if immigrant_or_offline and not (self.immigrant(r) or self.current_offline(r)):
            return False
        if excluded_topics is not None and not (self.orig_offline[r] or self.topic(r) not in excluded_topics):
            return False
        if included_topics is not None and self.topic(r) not in included_topics:
            return False
        if above is not None and not self.util(r, RES[above[0]]) > above[1]:
            return False
        if below is not None and not self.util(r, RES[below[0]]) < below[1]:
            return False
        return True

    def tuple_of(self, r, priorities=(), score=None, reverse=False, **_):
        t = []
        for p in priorities:
            if PRIO[p] == 0:
                t.append(0 if self.current_offline(r) else 1)  # PRIORITIZE_OFFLINE_REPLICAS
            else:
                t.append(0 if self.immigrant(r) else 1)        # PRIORITIZE_IMMIGRANTS
        if score is None:
            t.append(0.0)
        else:
            v = self.group_avg(r, RES[score])
            t.append(-v if reverse else v)
        p = self.part[r]
        t += [self.current_offline(r), self.rs.number[p], self.ids[self.orig[r]], self.topic(r)]
        return tuple(t)

    def expected(self, brokers=None, **spec):
        """Per asked broker ([(partition, broker), ...], [score, ...]) in SortedReplicas' order."""
        ask = list(range(self.B)) if brokers is None else list(brokers)
        by_broker = {b: [] for b in ask}
        for r in range(self.R):
            b = self.rs.broker[r]
            if b in by_broker and self.selected(r, **spec):
                by_broker[b].append(r)
        nprio, has_score = len(spec.get("priorities", ())), spec.get("score") is not None
        out = []
        for b in ask:
            rows = sort_tuples([self.tuple_of(r, **spec) + (r,) for r in by_broker[b]], nprio, has_score)
            out.append(([(self.part[t[-1]], b) for t in rows], [t[nprio] for t in rows]))
        return out


def assert_same(lists, scores, want):
    """The product's lists and scores against SortedModel.expected: list for list, score bits for score bits."""
    assert len(lists) == len(want) and len(scores) == len(want)
    for i, (rows, sc) in enumerate(want):
        got = [tuple(int(x) for x in row) for row in lists[i]]
        differ = [k for k in range(min(len(got), len(rows))) if got[k] != rows[k]][:3]
        assert got == rows, (i, len(got), len(rows), differ)
        assert [double_bits(float(x)) for x in scores[i]] == [double_bits(x) for x in sc], i


def check(cm, model, brokers=None, **spec):
    """One query on the product and on the restatement; returns the product's lists."""
    lists, scores = cm.sorted_replicas(brokers, with_scores=True, **spec)
    assert_same(lists, scores, model.expected(brokers, **spec))
    return lists


def as_bytes(lists):
    return [np.ascontiguousarray(x).tobytes() for x in lists]
