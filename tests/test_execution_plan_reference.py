"""The restatement of ExecutionTaskPlanner the GPU tests compare with (execution_plan_support.py), pinned to the
expectations of the reference's own ExecutionTaskPlannerTest and PostponeUrpReplicaMovementStrategyTest. The
expectations are data read off the Java tests (tests/golden/execution_plan_kat.json); nothing here runs on a device.
"""
import json
import os

import pytest

import ccmi
from execution_plan_support import (BASE, LARGE, MISSING, SMALL, URP, Chain, Task, build_plan, java_int, proposal)

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "execution_plan_kat.json")))
BITS = {"UNDER_REPLICATED": ccmi.PSTATE_UNDER_REPLICATED, "UNDER_MIN_ISR": ccmi.PSTATE_UNDER_MIN_ISR,
        "AT_MIN_ISR": ccmi.PSTATE_AT_MIN_ISR, "ONE_ABOVE_MIN_ISR": ccmi.PSTATE_ONE_ABOVE_MIN_ISR}


def _state(names):
    return {int(p): sum(BITS[n] for n in flags) for p, flags in names.items()}


def _proposals(rows):
    return [proposal(*r) for r in rows]


@pytest.mark.parametrize("case", KAT["rounds"], ids=lambda c: c["name"])
def test_first_round_of_the_planner_tests(case):
    ready = {int(b): n for b, n in case["ready_brokers"].items()}  # shared by the runs, as in the Java test
    for run in case["runs"]:
        chain = [ccmi.MOVEMENT_STRATEGIES.index(s) for s in run["strategies"]]
        plan = build_plan(_proposals(case["proposals"]), case["num_brokers"], chain, _state(case["partition_state"]))
        assert plan.summary["num_inter_tasks"] == len(case["proposals"]) and plan.summary["mingled"] == 0
        got = [plan.tasks[t].proposal.partition for t in plan.next_round(ready, (), KAT["max_moves"])]
        want = run["expected_first_tasks"]
        assert got[:len(want)] == want, run["strategies"]
        assert sorted(got) == [r[0] for r in case["proposals"]] and plan.remaining() == 0
    assert all(n >= 0 for n in ready.values())


@pytest.mark.parametrize("case", KAT["counts"], ids=lambda c: c["name"])
def test_task_counts_of_the_planner_tests(case):
    plan = build_plan(_proposals(case["proposals"]), case["num_brokers"])
    if "expected_leader_tasks" in case:
        assert plan.leader_tasks == case["expected_leader_tasks"]
    if "expected_num_leader_tasks" in case:
        assert plan.summary["num_leader_tasks"] == case["expected_num_leader_tasks"]
    if "expected_num_inter_tasks" in case:
        assert plan.summary["num_inter_tasks"] == case["expected_num_inter_tasks"] == len(plan.tasks)
    if "expected_num_intra_tasks" in case:  # with intra-broker tasks the swap tasks are dropped, nothing is thrown
        assert plan.summary["num_intra_tasks"] == case["expected_num_intra_tasks"]
        assert sorted(b for b, v in plan.intra.items() if v) == [0, 1]
        assert plan.tasks == [] and plan.inter == {} and plan.summary["mingled"] == 0
        assert plan.summary["num_inter_tasks"] == 1  # counted before the drop


def test_postpone_urp_comparator_cases():
    kat = KAT["postpone_urp_comparator"]
    names = list(kat["partitions"])
    state = {i: (MISSING if kat["partitions"][n] is None else sum(BITS[f] for f in kat["partitions"][n]))
             for i, n in enumerate(names)}
    chain = Chain([URP], state)
    tasks = {n: Task(0, proposal(i, 10000, 0, [0], [0]), (), 0) for i, n in enumerate(names)}
    for a, b, want in kat["cases"]:
        assert chain.compare_one(URP, tasks[a], tasks[b]) == want, (a, b)


def test_narrowing_and_the_appended_base():
    assert java_int(2 ** 31) == -2 ** 31 and java_int(2 ** 32 + 5) == 5 and java_int(-1) == -1
    big = Task(0, proposal(0, 2 ** 31 + 1, 0, [0], [1]), (1,), 2 ** 31 + 1)
    zero = Task(1, proposal(1, 0, 0, [0], [1]), (1,), 0)
    # (int)(2^31 + 1) is negative and (int)-(2^31 + 1) positive: the narrowed comparators order the two the wrong way
    assert Chain([SMALL]).compare(big, zero) < 0 and Chain([SMALL], narrow=False).compare(big, zero) > 0
    assert Chain([LARGE]).compare(big, zero) > 0 and Chain([LARGE], narrow=False).compare(big, zero) < 0
    assert Chain([LARGE]).strategies == [LARGE, BASE] and Chain([BASE, LARGE]).strategies == [BASE, LARGE]
    same = Task(2, proposal(2, 0, 0, [0], [1]), (1,), 0)
    assert Chain([SMALL]).compare(zero, same) < 0  # equal sizes: the execution id decides


def test_mingled_and_drop():
    # a disk move on broker 0 and an inter-broker move with a destination: the reference throws
    disk = proposal(0, 5, 0, [0, 1], [0, 1], [0, 2], [1, 2])
    move = proposal(1, 7, 2, [2, 3], [2, 4], [4, 6], [4, 8])
    plan = build_plan([disk, move], 5)
    assert plan.summary["mingled"] == 1 and plan.summary["num_inter_tasks"] == 1
    assert plan.summary["num_intra_tasks"] == 1 and plan.summary["num_inter_entries"] == 0
    assert (plan.tasks, plan.inter, plan.intra, plan.leader_tasks) == ([], {}, {}, [])
    # a disk move and a pure reorder: dropped, not thrown; the leadership task stays
    swap = proposal(1, 7, 2, [2, 3], [3, 2], [4, 6], [6, 4])
    plan = build_plan([disk, swap], 5)
    assert plan.summary["mingled"] == 0 and plan.summary["num_inter_tasks"] == 1 and plan.tasks == []
    assert plan.intra == {0: [0]} and plan.leader_tasks == [1]
    # a leader whose disk alone changed: hasLeaderAction, but no leadership task
    plan = build_plan([disk], 5)
    assert plan.leader_tasks == [] and plan.summary["num_leader_tasks"] == 0 and plan.summary["num_intra_tasks"] == 1
