"""ccmi_moves_acceptance_mask on a library without it.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The masks are computed on
the device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the same, and
ClusterModel.moves_acceptance_mask refuses with UnsupportedOperationException instead of answering on the host.
"""
import os
import re

import numpy as np
import pytest

import ccmi
from parity import constraint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)


def test_symbol_is_additive_at_abi_13():
    header = open(os.path.join(REPO, "include", "ccmi.h")).read()
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_moves_acceptance_mask" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_moves_acceptance_mask\(", header)
    assert "typedef struct ccmi_move_source {" in header
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "mask" in f]


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_moves_acceptance_mask is False
    assert not hasattr(emu_lib.lib, "ccmi_moves_acceptance_mask")


def test_emu_moves_acceptance_mask_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    goals = ["RackAwareGoal", "ReplicaCapacityGoal"]
    ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(goals))
    a = cm.actions()[-1]
    source = (a[0], a[1], a[3])  # the replica the last action moved, where it is now
    for packed in (False, True):
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.moves_acceptance_mask(goals, [source], packed=packed)
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.moves_acceptance_mask(goals, [], packed=packed)
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.moves_acceptance_mask([], np.zeros((0, 3), dtype=np.int32), packed=packed)
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)
