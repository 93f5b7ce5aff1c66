"""ccmi_swaps_acceptance_grid on a library without it.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The grid is computed on
the device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the same, and
ClusterModel.swaps_acceptance_grid refuses with UnsupportedOperationException instead of answering on the host.
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
    assert "ccmi_swaps_acceptance_grid" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_swaps_acceptance_grid\(", header)
    assert "typedef struct ccmi_swap_replica {" in header
    assert "typedef enum ccmi_swap_code {" in header
    # the enum's values are the indices of SWAP_CODES
    assert ccmi.SWAP_CODES == ["ACCEPT", "REPLICA_REJECT", "BROKER_REJECT", "SOURCE_NOT_LEGIT", "CANDIDATE_NOT_LEGIT"]
    for value, name in enumerate(ccmi.SWAP_CODES):
        assert re.search(rf"CCMI_SWAP_{name} = {value}\b", header), name
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "swap" in f and "accept" in f]


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_swaps_acceptance_grid is False
    assert not hasattr(emu_lib.lib, "ccmi_swaps_acceptance_grid")


def test_emu_swaps_acceptance_grid_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    goals = ["RackAwareGoal", "ReplicaCapacityGoal"]
    ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(goals))
    a, b = cm.actions()[-1], cm.actions()[0]
    source, candidate = (a[1], a[3]), (b[1], b[3])  # replicas the chain moved, where they are now
    for src, cand in (([source], [candidate]), ([source], []), ([], [candidate]), ([], []),
                      (np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.int32))):
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.swaps_acceptance_grid(goals, src, cand)
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.swaps_acceptance_grid([], src, cand)
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)
