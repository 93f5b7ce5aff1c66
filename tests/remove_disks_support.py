"""The yardstick of the remove-disks tests: a literal restatement of RemoveDisksRunnable.checkCanRemoveDisks
(servlet/handler/async/runnable/RemoveDisksRunnable.java:131-161), Disk.markDiskForRemoval (model/Disk.java:113-118)
and IntraBrokerDiskCapacityGoal(shouldEmptyZeroCapacityDisks).optimize with no optimized goals
(analyzer/goals/IntraBrokerDiskCapacityGoal.java, AbstractGoal.optimize :85-131, maybeMoveReplicaBetweenDisks :351-378)
on a flat desc.

Nothing here depends on a hash order: brokersToBalance is a TreeSet of the alive brokers, a broker's disks iterate in
logdir order (TreeMap), candidateDisks.sort is TimSort's binary insertion sort (fewer than 32 disks) with the goal's
truncating comparator, and a disk's tracked replicas are ordered by prioritizeDiskImmigrants (original disk is not this
disk first), then the reversed DISK score in Double.compare order, then Replica.compareTo. Per-replica loads, scores
and offline state come from sorted_replicas_support.SortedModel (float32 windows widened as the reference does).

initGoalState's broker-level check sums a broker's load, which this module does not restate: Yardstick.optimize
refuses a model that is within 1e-6 relative of that limit instead of deciding it.
"""
import ctypes as C
import functools

import ccmi
from sorted_replicas_support import DISK, SortedModel, double_compare, replica_compare_to

INTRA_MOVE = 3  # ccmi action type INTRA_BROKER_REPLICA_MOVEMENT
GOAL = "IntraBrokerDiskCapacityGoal"
DEAD = 1        # ccmi_broker_state


class IllegalArgument(Exception):
    pass


class OptimizationFailure(Exception):
    def __init__(self, message, num_disks=None, total_capacity=None):
        super().__init__(message)
        self.num_disks, self.total_capacity = num_disks, total_capacity


def double_int_value(x):
    """((Double) x).intValue(): NaN is 0, out of range saturates, else truncation toward zero."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def tim_sort_small(a, compare):
    """java.util.TimSort.sort for fewer than MIN_MERGE (32) elements: countRunAndMakeAscending, then binarySort."""
    n = len(a)
    assert n < 32
    if n < 2:
        return
    run_hi = 1
    if compare(a[run_hi], a[0]) < 0:
        run_hi += 1
        while run_hi < n and compare(a[run_hi], a[run_hi - 1]) < 0:
            run_hi += 1
        a[0:run_hi] = a[0:run_hi][::-1]
    else:
        run_hi += 1
        while run_hi < n and compare(a[run_hi], a[run_hi - 1]) >= 0:
            run_hi += 1
    for start in range(run_hi, n):
        pivot = a[start]
        left, right = 0, start
        while left < right:
            mid = (left + right) >> 1
            if compare(pivot, a[mid]) < 0:
                right = mid
            else:
                left = mid + 1
        a[left + 1:start + 1] = a[left:start]
        a[left] = pivot


def java_fixed(x, digits):
    """String.format("%.<digits>f") of a finite double (HALF_UP on the shortest repr, as java.util.Formatter)."""
    from decimal import ROUND_HALF_UP, Decimal
    return str(Decimal(repr(float(x))).quantize(Decimal(1).scaleb(-digits), rounding=ROUND_HALF_UP))


class Yardstick:
    """The model state the goal reads: disks (capacity, state, utilization, replica set) and replicas."""

    def __init__(self, desc, excluded_topics=()):
        self.desc = desc
        self.sm = SortedModel(desc)
        B, R, D = desc.num_brokers, desc.num_replicas, desc.num_disks
        self.B, self.R, self.D = B, R, D
        self.ids = list(desc.broker_id[:B])
        self.broker_alive = [desc.broker_state[b] != DEAD for b in range(B)]
        self.broker_disk_cap = [desc.broker_capacity[4 * b + ccmi.DISK] for b in range(B)]
        self.disk_broker = list(desc.disk_broker[:D])
        self.logdir = [desc.disk_logdir[d].decode() for d in range(D)]
        # Disk(logDir, broker, capacity): negative = dead (capacity -1); Broker.setState(DEAD) kills its disks
        self.alive = [desc.disk_capacity[d] >= 0 and self.broker_alive[self.disk_broker[d]] for d in range(D)]
        self.cap = [desc.disk_capacity[d] if self.alive[d] else -1.0 for d in range(D)]
        self.disks_of = [sorted((d for d in range(D) if self.disk_broker[d] == b), key=lambda d: self.logdir[d])
                         for b in range(B)]
        self.part = list(desc.replica_partition[:R])
        self.du = [self.sm.util(r, DISK) for r in range(R)]
        self.score = [self.sm.group_avg(r, DISK) for r in range(R)]
        self.tail = [(self.sm.current_offline(r), self.sm.rs.number[self.part[r]], self.ids[self.sm.orig[r]],
                      self.sm.topic(r)) for r in range(R)]
        excluded = set(excluded_topics)
        topic_index = self.sm.rs.topic
        # selectOnlineReplicas && selectReplicasBasedOnExcludedTopics (ReplicaSortFunctionFactory.java:135-146)
        self.selected = [not self.sm.current_offline(r) and
                         (not excluded or self.sm.orig_offline[r] or topic_index[self.part[r]] not in excluded)
                         for r in range(R)]
        self.orig_disk = [desc.replica_disk[r] if desc.replica_disk else -1 for r in range(R)]
        self.disk = list(self.orig_disk)
        self.util = [0.0] * D
        self.members = [set() for _ in range(D)]
        for r in range(R):  # createReplica + setReplicaLoad: Disk.addReplicaLoad in replica order
            if self.disk[r] >= 0:
                self._add(self.disk[r], r)
        for i in range(desc.num_disk_assignments):  # the fixture's placement step: Disk.addReplica in order
            self._add(desc.disk_assign_disk[i], desc.disk_assign_replica[i])
        self.initial_disk = list(self.disk)
        self.actions = []
        self.candidates = 0

    def _add(self, d, r):  # Disk.addReplica
        self.util[d] += self.du[r]
        self.members[d].add(r)
        self.disk[r] = d

    def _remove(self, d, r):  # Disk.removeReplica
        self.util[d] -= self.du[r]
        self.members[d].remove(r)

    # ------------------------------------------------------------------------------- RemoveDisksRunnable
    def disks_named(self, broker_logdirs):
        """{broker id: logdirs} as desc disk indices; "Invalid log dirs provided" for an unknown one."""
        out = []
        for broker_id, logdirs in broker_logdirs.items():
            for logdir in logdirs:
                found = [d for d in range(self.D)
                         if self.ids[self.disk_broker[d]] == broker_id and self.logdir[d] == logdir]
                if not found:
                    raise IllegalArgument(f"Invalid log dirs provided for broker {broker_id}.")
                out.append(found[0])
        return out

    def check_can_remove(self, disks, capacity_threshold):
        """checkCanRemoveDisks, the brokers named in ascending order."""
        listed = set(disks)
        for b in sorted({self.disk_broker[d] for d in listed}, key=lambda b: self.ids[b]):
            mine = self.disks_of[b]
            if len(mine) == len([d for d in mine if d in listed]):
                raise IllegalArgument(f"No log dir remaining to move replicas to for broker {self.ids[b]}.")
            future_usage, remaining = 0.0, 0.0
            for d in mine:
                future_usage += self.util[d]
                if d not in listed:
                    remaining += self.cap[d]
            # Java double division: x / 0.0 is an infinity, 0.0 / 0.0 is NaN (every comparison false)
            if remaining == 0.0:
                ratio = float("nan") if future_usage == 0.0 or future_usage != future_usage else \
                    (float("inf") if future_usage > 0 else float("-inf"))
            else:
                ratio = future_usage / remaining
            if ratio > capacity_threshold:
                raise IllegalArgument(f"Not enough remaining capacity to move replicas to for broker {self.ids[b]}.")

    def mark(self, disks):
        for d in disks:  # Disk.markDiskForRemoval
            self.cap[d] = 0.0

    def can_remove(self, disks, capacity_threshold):
        try:
            self.check_can_remove(disks, capacity_threshold)
            return True
        except IllegalArgument:
            return False

    # ------------------------------------------------------------------------------- the goal
    def over_limit(self, d, thr, empty_zero):
        """isUtilizationOverLimit (:270-275)."""
        if empty_zero and self.cap[d] == 0:
            return self.util[d] > 0 or len(self.members[d]) > 0
        return self.util[d] > self.cap[d] * thr

    def tracked(self, d):
        """disk.trackedSortedReplicas(...).sortedReplicas(true): a clone, in the comparator's order."""
        def compare(r1, r2):
            p1, p2 = (0 if self.orig_disk[r1] != d else 1), (0 if self.orig_disk[r2] != d else 1)
            if p1 != p2:
                return -1 if p1 < p2 else 1
            c = double_compare(-self.score[r1], -self.score[r2])
            return c if c else replica_compare_to(self.tail[r1], self.tail[r2])
        return sorted((r for r in self.members[d] if self.selected[r]), key=functools.cmp_to_key(compare))

    def _init_goal_state(self, thr):
        for b in range(self.B):
            if not self.broker_alive[b]:
                continue
            existing = sum(self.du[r] for r in range(self.R) if self.sm.broker(r) == b)
            allowed = self.broker_disk_cap[b] * thr
            if not existing < allowed * (1 - 1e-6) and not (existing == 0 and allowed >= 0):
                raise NotImplementedError("the broker-level check of initGoalState is not restated this close to it")

    def optimize(self, thr, empty_zero=True, brokers=None):
        """AbstractGoal.optimize: initGoalState, rebalanceForBroker over the alive brokers, updateGoalState.
        `brokers` restricts the broker loop (test use: one broker's records)."""
        self._init_goal_state(thr)
        for b in sorted((b for b in range(self.B) if self.broker_alive[b]), key=lambda b: self.ids[b]):
            if brokers is None or b in brokers:
                self._rebalance(b, thr, empty_zero)
        self._update_goal_state(thr, empty_zero)

    def _rebalance(self, b, thr, empty_zero):
        disks = self.disks_of[b]
        over = [d for d in disks if self.alive[d] and self.over_limit(d, thr, empty_zero)]
        if not over:
            return
        cands = [d for d in disks if d not in over]

        def compare(d1, d2):
            a1 = self.cap[d1] * thr - self.util[d1]
            a2 = self.cap[d2] * thr - self.util[d2]
            return double_int_value(a2 - a1)
        tim_sort_small(cands, compare)
        for d in over:
            for r in self.tracked(d):
                self._maybe_move(r, cands, thr, empty_zero)
                if not self.over_limit(d, thr, empty_zero):
                    break

    def _maybe_move(self, r, cands, thr, empty_zero):
        for t in cands:
            self.candidates += 1
            if not self.alive[t]:  # legitMoveBetweenDisks (the candidates are the broker's own disks)
                continue
            u = self.du[r]
            should_move = u >= 0 if empty_zero else u > 0  # selfSatisfied
            if not (should_move and self.util[t] + u < self.cap[t] * thr):
                continue
            src = self.disk[r]  # relocateReplica(tp, broker, logdir): removeReplica, then addReplica
            self._remove(src, r)
            self._add(t, r)
            b = self.disk_broker[src]
            self.actions.append((INTRA_MOVE, self.part[r], b, b, -1, src, t))
            return t
        return None

    def disk_string(self, d):
        """Disk.toString (Disk.java:241-245)."""
        return "Disk[logdir=%s,state=%s,capacity=%s,replicaCount=%d]" % (
            self.logdir[d], "ALIVE" if self.alive[d] else "DEAD", java_fixed(self.cap[d], 6), len(self.members[d]))

    def _update_goal_state(self, thr, empty_zero):
        for b in sorted((b for b in range(self.B) if self.broker_alive[b]), key=lambda b: self.ids[b]):
            for d in self.disks_of[b]:
                if self.alive[d] and self.over_limit(d, thr, empty_zero):
                    raise OptimizationFailure(
                        "[%s] Utilization (%s) for disk %s on broker %d is above capacity limit."
                        % (GOAL, java_fixed(self.util[d], 2), self.disk_string(d), self.ids[b]),
                        num_disks=1, total_capacity=self.util[d] / thr)
                if empty_zero and self.cap[d] == 0 and self.members[d]:
                    raise OptimizationFailure("[%s] Could not move all replicas from disk %s on broker %d"
                                              % (GOAL, self.logdir[d], self.ids[b]))

    def outcome(self, thr, empty_zero=True):
        """("ok",) or ("fail", message, num_disks, total_capacity) of one optimize()."""
        try:
            self.optimize(thr, empty_zero)
            return ("ok",)
        except OptimizationFailure as e:
            return ("fail", str(e), e.num_disks, e.total_capacity)

    def replica_disks(self):
        """ClusterModel.replica_disks(): the disk of every replica slot in partition order."""
        return [self.disk[r] for r in self.desc.partition_replicas[:self.R]]

    def proposals(self):
        """(partition, old (broker, disk) pairs, new pairs) of every partition whose placement changed, as sets."""
        out = {}
        for r in range(self.R):
            if self.disk[r] != self.initial_disk[r]:
                out.setdefault(self.part[r], None)
        for p in out:
            rs = [r for r in range(self.R) if self.part[r] == p]
            out[p] = (frozenset((self.sm.broker(r), self.initial_disk[r]) for r in rs),
                      frozenset((self.sm.broker(r), self.disk[r]) for r in rs))
        return out


# ----------------------------------------------------------------------------------- product side helpers
class ZeroedDesc:
    """A copy of a desc whose listed disks have capacity 0.0 (what markDiskForRemoval leaves); keeps its array."""

    def __init__(self, desc, disks):
        D = desc.num_disks
        caps = list(desc.disk_capacity[:D])
        for d in disks:
            if caps[d] >= 0:  # a dead disk stays dead
                caps[d] = 0.0
        self.keep = (C.c_double * max(1, D))(*caps)
        self.desc = ccmi.ClusterDesc.from_buffer_copy(desc)
        self.desc.disk_capacity = C.cast(self.keep, C.POINTER(C.c_double))


def product_proposals(cm):
    return {p.partition: (frozenset(zip(p.old_replicas, p.old_disks)), frozenset(zip(p.new_replicas, p.new_disks)))
            for p in cm.proposals()}


def product_outcome(cm, run):
    """run() -> ("ok",) or ("fail", message, num_disks, total_capacity) with the failure's recommendation."""
    try:
        run()
        return ("ok",)
    except ccmi.OptimizationFailureException as e:
        recs = list(e.provision.recommendation_by_recommender.values())
        if not recs:
            return ("fail", str(e), None, None)
        return ("fail", str(e), recs[0].num_disks, recs[0].total_capacity)


def assert_matches(cm, y, got, want):
    """The product's action log, final disks, proposals with logdirs and outcome against the yardstick's."""
    assert got[:2] == want[:2], (got, want)
    if want[0] == "fail":
        assert got[2] == want[2], (got, want)
        if want[3] is not None:
            assert got[3] == want[3], (got, want)
    acts = cm.actions()
    differ = [k for k in range(min(len(acts), len(y.actions))) if acts[k] != y.actions[k]][:3]
    assert acts == y.actions, (len(acts), len(y.actions), differ)
    assert cm.replica_disks() == y.replica_disks()
    if want[0] == "ok":  # a failed optimization returns no proposals (the exception leaves GoalOptimizer)
        assert product_proposals(cm) == y.proposals()


# ----------------------------------------------------------------------------------- RemoveDisksTest
# RemoveDisksTest.java:62-133 with TestConstants (LARGE_BROKER_CAPACITY 300000.0, TYPICAL_CPU_CAPACITY 100.0,
# MEDIUM_BROKER_CAPACITY 200000.0, LOGDIR0 /mnt/i00, LOGDIR1 /mnt/i01, DISK_CAPACITY 150000.0 each), the default
# disk capacity threshold 0.8, and getAggregatedMetricValues(40.0, 100.0, 130.0, replicaLoad)
LOGDIR0, LOGDIR1 = "/mnt/i00", "/mnt/i01"
REMOVE_DISKS_TEST_ROWS = (("medium", 300000.0 / 4, True), ("zero", 0.0, True), ("max", 300000.0 / 2 * 0.8, False))


def remove_disks_test_model(disk_load):
    bld = ccmi.ClusterModelBuilder()
    capacity = {"CPU": 100.0, "DISK": 300000.0, "NW_IN": 300000.0, "NW_OUT": 200000.0}
    for broker, rack in ((0, "A::0"), (1, "B::0"), (2, "C::1")):
        bld.create_broker(rack, broker, capacity, {LOGDIR0: 150000.0, LOGDIR1: 150000.0})
    bld.create_replica("A::0", 0, "topic", 0, 0, True, False, LOGDIR0)
    bld.set_replica_load("A::0", 0, "topic", 0, 40.0, 100.0, 130.0, disk_load)
    return bld.build()
