"""ccmi_execution_plan on a library without it, and what the binding promises on the CPU.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The plan is built on the
device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the same and
ClusterModel.execution_plan refuses with UnsupportedOperationException instead of answering on the host.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ccmi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)
STRUCTS = (("ccmi_execution_plan_query", ccmi.ExecutionPlanQueryStruct, 64), ("ccmi_plan_task", ccmi.PlanTaskStruct, 16),
           ("ccmi_plan_summary", ccmi.PlanSummaryStruct, 64))


def _read(*path):
    return open(os.path.join(REPO, *path)).read()


def test_symbol_is_additive_at_abi_13():
    header = _read("include", "ccmi.h")
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_execution_plan" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_execution_plan\(ccmi_session\* s, const ccmi_execution_plan_query\* q, "
                     r"ccmi_plan_summary\* summary,\s*ccmi_plan_task\* tasks[^;]*int64_t task_capacity,\s*"
                     r"int64_t\* inter_offsets[^;]*int32_t\* inter_entries[^;]*int64_t inter_capacity, "
                     r"int32_t\* broker_order[^;]*int64_t\* intra_offsets[^;]*int32_t\* intra_entries[^;]*"
                     r"int64_t intra_capacity, int32_t\* leader_tasks[^;]*int64_t leader_capacity\);", header)
    assert re.search(r"ccmi_execution_plan\s+<- ExecutionTaskPlanner\.addExecutionProposals", header)  # the list at the top
    for value, name in enumerate(("BASE", "PRIORITIZE_LARGE", "PRIORITIZE_SMALL", "POSTPONE_URP",
                                  "PRIORITIZE_MIN_ISR_WITH_OFFLINE", "PRIORITIZE_ONE_ABOVE_MIN_ISR_WITH_OFFLINE")):
        assert re.search(r"\bCCMI_STRATEGY_%s = %d\b" % (name, value), header), name
        assert getattr(ccmi, "STRATEGY_" + name) == value
    assert len(ccmi.MOVEMENT_STRATEGIES) == 6 and ccmi.MOVEMENT_STRATEGIES[0] == "BaseReplicaMovementStrategy"
    for name, value in (("UNDER_REPLICATED", 1), ("UNDER_MIN_ISR", 2), ("AT_MIN_ISR", 4), ("ONE_ABOVE_MIN_ISR", 8)):
        assert re.search(r"\bCCMI_PSTATE_%s = %d\b" % (name, value), header), name
        assert getattr(ccmi, "PSTATE_" + name) == value
    # the assumption the plan is computed under is stated in the header
    assert "still has the session's initial placement" in header and "size_overflow" in header
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "plan" in f]


def test_documents_name_the_entry_point_the_kernels_and_the_probe():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):  # with the header: the four documents
        assert "ccmi_execution_plan" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "K16 measured" in design and "csrc/kernels/execution_plan.hip" in design
    assert "tools/execution_plan_probe.py" in design and os.path.exists(os.path.join(REPO, "tools", "execution_plan_probe.py"))
    assert "Execution plan: what the executor does first with the proposals" in _read("INTEGRATION.md")
    makefile = _read("cruise-control_amd", "Makefile")
    assert "csrc/ccmi_execution_plan.cpp" in makefile and "csrc/kernels/execution_plan.hip" in makefile


@pytest.mark.parametrize("name,mirror,size", STRUCTS, ids=[s[0] for s in STRUCTS])
def test_struct_mirrors_match_the_header(name, mirror, size):
    assert C.sizeof(mirror) == size and size & (size - 1) == 0
    header = _read("include", "ccmi.h")
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            declared.append(re.sub(r"\[\d+\]", "", decl.split()[-1]).lstrip("*"))
    assert declared == [f for f, _ in mirror._fields_]
    assert ccmi.ExecutionPlanQueryStruct.strategies.offset == 4
    assert ccmi.ExecutionPlanQueryStruct.proposal_rank.offset == 48
    assert ccmi.ExecutionPlanQueryStruct.partition_state.offset == 56
    assert ccmi.PlanTaskStruct.data_to_move_mb.offset == 8
    assert ccmi.PlanSummaryStruct.mingled.offset == 48


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_execution_plan is False
    assert not hasattr(emu_lib.lib, "ccmi_execution_plan")


def test_emu_execution_plan_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.execution_plan()  # a fresh session
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.execution_plan(["PostponeUrpReplicaMovementStrategy", ccmi.STRATEGY_PRIORITIZE_LARGE],
                          proposal_rank=np.arange(cm.desc.num_partitions),
                          partition_state=np.zeros(cm.desc.num_partitions, dtype=np.uint8))
    assert cm.actions() == []
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)


def test_next_round_is_a_host_walk_over_the_lists():
    """ExecutionPlan.next_round needs no library: the four partition movements of the reference's planner test, filed
    by hand the way the entry point returns them, give the reference's first round under the base strategy."""
    tasks = np.zeros(4, dtype=np.dtype(ccmi.PlanTaskStruct))
    tasks["partition"], tasks["num_to_add"], tasks["data_to_move_mb"] = [0, 1, 2, 3], 1, [10, 30, 20, 10]
    inter = [np.array(x, dtype=np.int32) for x in ([0, 3], [0, 1], [1, 2], [2, 3])]  # old leader and destination
    plan = ccmi.ExecutionPlan(ccmi.PlanSummaryStruct(), tasks, inter, np.array([0, 1, 2, 3], dtype=np.int32),
                              [[]] * 4, [], [ccmi.STRATEGY_BASE], None)
    ready = {b: 14 for b in range(4)}
    assert plan.next_round(ready, (), 1250) == [0, 2, 1, 3] and plan.remaining() == 0
    assert ready == {b: 12 for b in range(4)}
    assert plan.task_key(2) == (2,)
