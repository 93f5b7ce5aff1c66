"""ccmi_actions_acceptance (ABI v13) on a library without it.

The batched acceptance call runs on the device only, so the CPU tests' emulation build (tests/emu) reports ABI 13 but
does not export the symbol: the binding loads it all the same, and ClusterModel.actions_acceptance refuses with
UnsupportedOperationException instead of answering on the host.
"""
import re
import os

import numpy as np
import pytest

import ccmi
from parity import constraint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)


def test_binding_and_header_are_abi_13():
    header = open(os.path.join(REPO, "include", "ccmi.h")).read()
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_actions_acceptance" in ccmi.EXPORTED_SYMBOLS
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]


def test_emu_loads_at_abi_13_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert not emu_lib.has_actions_acceptance
    assert not hasattr(emu_lib.lib, "ccmi_actions_acceptance")


def test_emu_actions_acceptance_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    goals = ["RackAwareGoal", "ReplicaCapacityGoal"]
    ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(goals))
    a = cm.actions()[-1]
    reverse = (a[0], a[1], a[3], a[2], -1, -1, -1)
    # the single call works on the emulation; the batch does not fall back to it
    assert cm.action_acceptance_by_goal(goals[0], *reverse[:4]) in ccmi.ACCEPTANCE
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.actions_acceptance(goals, [reverse])
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.actions_acceptance(goals, np.zeros((0, 7), dtype=np.int32))
    # the perf counters of the batch exist and stay at zero
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)
