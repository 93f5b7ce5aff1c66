"""The reference of the execution plan tests: ExecutionTaskPlanner.addExecutionProposals restated literally.

`build_plan` works from plain proposal tuples in the order of the caller's collection and never touches the device
output. It restates ExecutionTaskPlanner.java:137-273 (the three maybeAdd* methods, sanityCheckExecutionTasks,
maybeDropReplicaSwapTasks), AbstractReplicaMovementStrategy.java:28-85 (chain, chainBaseReplicaMovementStrategyIfAbsent,
applyStrategy), the six strategy comparators as they are written, including the (int) narrowing of the size and id
differences, brokerComparator (:518-539) and getInterBrokerReplicaMovementTasks (:348-439).

The cluster the planner reads is the one the entry point assumes: every partition still has its old replicas, all in
sync, its old leader and its old logdirs. What the strategies read from the live ISR state comes in as one byte of
ccmi.PSTATE_* bits per partition (MISSING: the partition is not in the cluster metadata, which only
PostponeUrpReplicaMovementStrategy distinguishes).

tests/test_execution_plan_reference.py pins this file to the expectations of the reference's own unit tests.
"""
import ctypes as C
from collections import namedtuple
from functools import cmp_to_key

import numpy as np

import ccmi

Proposal = namedtuple("Proposal", "partition size old_leader old_replicas new_replicas old_disks new_disks")
Task = namedtuple("Task", "id proposal to_add data")
MISSING = None
INT32_MAX = 2 ** 31 - 1
SUMMARY_FIELDS = [f for f, _ in ccmi.PlanSummaryStruct._fields_ if f != "reserved"]
SENTINEL = 0xA5

BASE, LARGE, SMALL, URP, MIN_ISR, ONE_ABOVE = range(6)
assert ccmi.MOVEMENT_STRATEGIES[BASE].startswith("Base") and ccmi.MOVEMENT_STRATEGIES[URP].startswith("PostponeUrp")


def proposal(partition, size, old_leader, old_replicas, new_replicas, old_disks=None, new_disks=None):
    n = len(old_replicas)
    return Proposal(partition, size, old_leader, tuple(old_replicas), tuple(new_replicas),
                    tuple(old_disks) if old_disks is not None else (-1,) * n,
                    tuple(new_disks) if new_disks is not None else (-1,) * len(new_replicas))


def from_ccmi(p):
    """A ccmi.ExecutionProposal of the host path as a plain tuple."""
    return proposal(p.partition, p.partition_size, p.old_leader, p.old_replicas, p.new_replicas, p.old_disks,
                    p.new_disks)


def in_collection_order(proposals, rank=None):
    """The proposals in ascending (rank[partition], partition): the order the entry point numbers them in."""
    return sorted(proposals, key=lambda p: ((int(rank[p.partition]) if rank is not None else 0), p.partition))


# ---- ExecutionProposal.java
def replicas_to_add(p):  # :74
    return [b for b in p.new_replicas if b not in p.old_replicas]


def between_disks(p):  # :76-78: brokers of new placements that are not added and not old placements
    old = list(zip(p.old_replicas, p.old_disks))
    return [b for b, d in zip(p.new_replicas, p.new_disks) if b in p.old_replicas and (b, d) not in old]


def data_to_move(p):  # :242-244
    return (len(replicas_to_add(p)) + len(between_disks(p))) * p.size


def has_leader_action(p):  # :219-221
    old_leader_disk = p.old_disks[p.old_replicas.index(p.old_leader)]
    return (p.old_leader, old_leader_disk) != (p.new_replicas[0], p.new_disks[0])


# ---- the comparators, as written
def java_int(x):
    """(int) of a long."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


class Chain:
    """A ReplicaMovementStrategy chain over `state` (partition -> PSTATE_* bits, MISSING, or absent = 0).
    narrow=False compares the sizes as int64 values: the device's order when the summary reports size_overflow."""

    def __init__(self, strategies, state=None, narrow=True):
        self.strategies = list(strategies)
        if BASE not in self.strategies:  # chainBaseReplicaMovementStrategyIfAbsent
            self.strategies.append(BASE)
        self.state = state
        self.narrow = narrow

    def bits(self, task):
        if self.state is None:
            return 0
        if isinstance(self.state, dict):
            return self.state.get(task.proposal.partition, 0)
        return int(self.state[task.proposal.partition])

    def _int(self, x):
        return java_int(x) if self.narrow else (x > 0) - (x < 0)

    def compare_one(self, s, t1, t2):
        if s == BASE:  # BaseReplicaMovementStrategy.java:19
            return java_int(t1.id - t2.id)
        if s == LARGE:  # PrioritizeLargeReplicaMovementStrategy.java:18
            return self._int(t2.data - t1.data)
        if s == SMALL:  # PrioritizeSmallReplicaMovementStrategy.java:18
            return self._int(t1.data - t2.data)
        b1, b2 = self.bits(t1), self.bits(t2)
        if s == URP:  # PostponeUrpReplicaMovementStrategy.java:25-58
            e1, e2 = b1 is not MISSING, b2 is not MISSING
            u1 = e1 and bool(b1 & ccmi.PSTATE_UNDER_REPLICATED)
            u2 = e2 and bool(b2 & ccmi.PSTATE_UNDER_REPLICATED)
            if e1 and e2:
                return (0 if u2 else 1) if u1 else (-1 if u2 else 0)
            if e1:
                return 0 if u1 else -1
            if e2:
                return 0 if u2 else 1
            return 0
        b1, b2 = b1 or 0, b2 or 0
        if s == MIN_ISR:  # PrioritizeMinIsrWithOfflineReplicasStrategy.java:40-54
            under1, under2 = bool(b1 & ccmi.PSTATE_UNDER_MIN_ISR), bool(b2 & ccmi.PSTATE_UNDER_MIN_ISR)
            at1, at2 = bool(b1 & ccmi.PSTATE_AT_MIN_ISR), bool(b2 & ccmi.PSTATE_AT_MIN_ISR)
            if under1:
                return 0 if under2 else -1
            return 1 if under2 else ((0 if at2 else -1) if at1 else (1 if at2 else 0))
        if s == ONE_ABOVE:  # PrioritizeOneAboveMinIsrWithOfflineReplicasStrategy.java:40-50
            a1, a2 = bool(b1 & ccmi.PSTATE_ONE_ABOVE_MIN_ISR), bool(b2 & ccmi.PSTATE_ONE_ABOVE_MIN_ISR)
            if a1:
                return 0 if a2 else -1
            return 1 if a2 else 0
        raise ValueError(s)

    def compare(self, t1, t2):  # AbstractReplicaMovementStrategy.chain, :37-40, left to right
        for s in self.strategies:
            c = self.compare_one(s, t1, t2)
            if c != 0:
                return c
        return 0


class Plan:
    def __init__(self, num_brokers, chain):
        self.num_brokers = num_brokers
        self.chain = chain
        self.tasks = []          # the inter-broker tasks by execution id (empty after the drop)
        self.inter = {}          # broker -> its tasks in TreeSet order
        self.intra = {}          # broker -> partitions
        self.leader_tasks = []   # partitions
        self.summary = dict.fromkeys(SUMMARY_FIELDS, 0)

    # ---- what the entry point returns
    def inter_ids(self):
        return [[t.id for t in self.inter.get(b, [])] for b in range(self.num_brokers)]

    def intra_lists(self):
        return [list(self.intra.get(b, [])) for b in range(self.num_brokers)]

    def task_rows(self):
        return [(t.proposal.partition, len(t.to_add), t.data) for t in self.tasks]

    def broker_compare(self, b1, b2):  # brokerComparator, :521-538
        s1, s2 = self.inter.get(b1, []), self.inter.get(b2, [])
        if not s1:
            return 0 if not s2 else 1
        if not s2:
            return -1
        c = self.chain.compare(s1[0], s2[0])
        return c if c != 0 else (len(s2) - len(s1) if len(s1) != len(s2) else b1 - b2)

    def broker_order(self):
        return sorted((b for b in self.inter if self.inter[b]), key=cmp_to_key(self.broker_compare))

    def remaining(self):
        return len({t.id for s in self.inter.values() for t in s})

    def next_round(self, ready_brokers, in_progress=(), max_moves=1 << 30):
        """getInterBrokerReplicaMovementTasks, :348-439. Returns execution ids; the tasks leave the plan."""
        out = []

        def tree_add(ids, b):  # TreeSet.add under the comparator as it is now
            for i, x in enumerate(ids):
                c = self.broker_compare(b, x)
                if c == 0:
                    return
                if c < 0:
                    ids.insert(i, b)
                    return
            ids.append(b)

        ids = []
        for b in self.inter:
            tree_add(ids, b)
        new_task_added, capped = True, False
        in_progress = set(in_progress)
        num_in_progress, partitions_involved = len(in_progress), set()
        while new_task_added and not capped:
            new_task_added = False
            involved = set()
            for b in list(ids):
                if capped:
                    break
                if b in involved:
                    continue
                for task in list(self.inter[b]):
                    if num_in_progress >= max_moves:
                        capped = True
                        break
                    src, dests = task.proposal.old_leader, set(task.to_add)
                    if src in involved or involved & dests:
                        continue
                    tp = task.proposal.partition
                    executable = ready_brokers[src] > 0 and all(ready_brokers[d] > 0 for d in task.to_add)
                    if executable and tp not in in_progress and tp not in partitions_involved:
                        partitions_involved.add(tp)
                        out.append(task.id)
                        involved.add(src)
                        involved |= dests
                        for x in [src] + sorted(dests):
                            if x in ids:
                                ids.remove(x)
                        self.inter[src].remove(task)
                        for d in dests:
                            self.inter[d].remove(task)
                        for x in [src] + sorted(dests):
                            tree_add(ids, x)
                        ready_brokers[src] -= 1
                        for d in dests:
                            ready_brokers[d] -= 1
                        new_task_added = True
                        num_in_progress += 1
                        break
        return out


def build_plan(proposals, num_brokers, strategies=(), state=None, narrow=True):
    """addExecutionProposals over `proposals` (Proposal tuples in the collection's iteration order)."""
    chain = Chain(strategies, state, narrow)
    plan = Plan(num_brokers, chain)
    # maybeAddInterBrokerReplicaMovementTasks, :186-207: the cluster has old_replicas in order, all in sync
    for p in proposals:
        if tuple(p.new_replicas) != tuple(p.old_replicas):
            plan.tasks.append(Task(len(plan.tasks), p, tuple(replicas_to_add(p)), data_to_move(p)))
    key = cmp_to_key(chain.compare)
    for t in plan.tasks:  # applyStrategy, AbstractReplicaMovementStrategy.java:65-83
        for b in (t.proposal.old_leader,) + t.to_add:
            plan.inter.setdefault(b, []).append(t)
    for b in plan.inter:
        plan.inter[b].sort(key=key)
    # maybeAddIntraBrokerReplicaMovementTasks, :237-250: the current logdir of a replica is its old disk
    for p in proposals:
        for b in between_disks(p):
            plan.intra.setdefault(b, []).append(p.partition)
    # maybeAddLeaderChangeTasks, :261-271: the current leader is the old leader
    for p in proposals:
        if has_leader_action(p) and p.old_leader != p.new_replicas[0]:
            plan.leader_tasks.append(p.partition)
    s = plan.summary
    s["num_inter_tasks"] = len(plan.tasks)
    s["num_intra_tasks"] = sum(len(v) for v in plan.intra.values())
    s["num_leader_tasks"] = len(plan.leader_tasks)
    s["size_overflow"] = int(any(t.data > INT32_MAX for t in plan.tasks))
    if s["num_intra_tasks"] > 0:
        if any(t.to_add for t in plan.tasks):  # sanityCheckExecutionTasks throws, :152-160
            s["mingled"] = 1
            plan.intra, plan.leader_tasks = {}, []
        plan.tasks, plan.inter = [], {}  # maybeDropReplicaSwapTasks, :168-173
    s["num_inter_entries"] = sum(len(v) for v in plan.inter.values())
    s["num_brokers_with_tasks"] = sum(1 for v in plan.inter.values() if v)
    return plan


# ---- comparing a device plan with the restatement
def summary_dict(s):
    assert int(s.reserved) == 0
    return {f: int(getattr(s, f)) for f in SUMMARY_FIELDS}


def check(cm, want_proposals, strategies=(), rank=None, state=None, narrow=True):
    """The whole plan of ClusterModel.execution_plan against the restatement fed with `want_proposals` (Proposal tuples
    in any order): the task table, every inter and intra list, the broker order, the leadership tasks, the summary.
    Returns (the device plan, the restated plan)."""
    B = cm.desc.num_brokers
    want = build_plan(in_collection_order(want_proposals, rank), B, strategies, state, narrow)
    got = cm.execution_plan(strategies, proposal_rank=rank, partition_state=state)
    assert summary_dict(got.summary) == want.summary
    assert [(int(r["partition"]), int(r["num_to_add"]), int(r["data_to_move_mb"])) for r in got.tasks] == \
        want.task_rows()
    assert [[int(x) for x in seg] for seg in got.inter] == want.inter_ids()
    assert [int(b) for b in got.broker_order] == want.broker_order()
    assert [[int(x) for x in seg] for seg in got.intra] == want.intra_lists()
    assert [int(x) for x in got.leader_tasks] == want.leader_tasks
    return got, want


def raw_call(cm, strategies=(), caps=(0, 0, 0, 0), rooms=None, rank=None, state=None):
    """ccmi_execution_plan through ctypes into sentinel-filled buffers with room for `rooms` entries each (default: the
    capacities) plus 8 guard entries. Returns (status, summary, dict of the buffers as numpy arrays)."""
    B = cm.desc.num_brokers
    rooms = caps if rooms is None else rooms
    q = ccmi.ExecutionPlanQueryStruct()
    q.num_strategies = len(strategies)
    for i in range(4):
        q.strategies[i] = strategies[i] if i < len(strategies) else -1
    keep = []
    if rank is not None:
        keep.append(np.ascontiguousarray(rank, dtype=np.int32))
        q.proposal_rank = keep[-1].ctypes.data_as(C.POINTER(C.c_int32))
    if state is not None:
        keep.append(np.ascontiguousarray(state, dtype=np.uint8))
        q.partition_state = keep[-1].ctypes.data_as(C.POINTER(C.c_uint8))
    guard = 8
    bufs = {
        "tasks": np.full((rooms[0] + guard) * 16, SENTINEL, dtype=np.uint8),
        "inter_offsets": np.full(B + 1 + guard, -7, dtype=np.int64),
        "inter": np.full(rooms[1] + guard, -7, dtype=np.int32),
        "order": np.full(B + guard, -7, dtype=np.int32),
        "intra_offsets": np.full(B + 1 + guard, -7, dtype=np.int64),
        "intra": np.full(rooms[2] + guard, -7, dtype=np.int32),
        "leaders": np.full(rooms[3] + guard, -7, dtype=np.int32),
    }
    summary = ccmi.PlanSummaryStruct()
    st = cm.lib.lib.ccmi_execution_plan(cm.handle, C.byref(q), C.byref(summary), bufs["tasks"].ctypes.data, caps[0],
                                        bufs["inter_offsets"].ctypes.data, bufs["inter"].ctypes.data, caps[1],
                                        bufs["order"].ctypes.data, bufs["intra_offsets"].ctypes.data,
                                        bufs["intra"].ctypes.data, caps[2], bufs["leaders"].ctypes.data, caps[3])
    return st, summary, bufs
