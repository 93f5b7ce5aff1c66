"""ccmi_broker_stats on a library without it.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The stats are computed on
the device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the same,
ClusterModel.broker_stats and GoalOptimizer.optimizations(..., broker_stats=True) refuse with
UnsupportedOperationException instead of answering on the host, and optimizations without the flag is what it was.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ccmi
from parity import constraint

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)
GOALS = ["RackAwareGoal", "ReplicaCapacityGoal"]


def test_symbol_is_additive_at_abi_13():
    header = open(os.path.join(REPO, "include", "ccmi.h")).read()
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_broker_stats" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_broker_stats\(", header)
    assert "typedef struct ccmi_basic_stats {" in header
    assert "typedef struct ccmi_disk_stats {" in header
    assert re.search(r"ccmi_broker_stats\s+<- ClusterModel\.brokerStats", header)  # the list at the top
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "broker_stats" in f]
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "ccmi_broker_stats" in integration


def test_struct_mirrors_match_the_header():
    assert C.sizeof(ccmi.BasicStatsStruct) == 128
    assert C.sizeof(ccmi.DiskStatsStruct) == 40
    assert np.dtype(ccmi.BasicStatsStruct).itemsize == 128 and np.dtype(ccmi.DiskStatsStruct).itemsize == 40
    header = open(os.path.join(REPO, "include", "ccmi.h")).read()
    for name, struct in (("ccmi_basic_stats", ccmi.BasicStatsStruct), ("ccmi_disk_stats", ccmi.DiskStatsStruct)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                declared += [re.sub(r"\[\d+\]", "", x).strip() for x in decl.split(None, 1)[1].split(",")]
        assert declared == [f for f, _ in struct._fields_], name
    # the fields a shim reads at fixed offsets
    assert ccmi.BasicStatsStruct.replicas.offset == 88 and ccmi.BasicStatsStruct.reserved.offset == 112
    assert ccmi.DiskStatsStruct.num_replicas.offset == 24


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_broker_stats is False
    assert not hasattr(emu_lib.lib, "ccmi_broker_stats")


def test_emu_broker_stats_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.broker_stats()  # a fresh session
    with pytest.raises(ccmi.UnsupportedOperationException):
        ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(GOALS), broker_stats=True)
    assert cm.actions() == []  # refused before any goal ran
    res = ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(GOALS))
    assert res.broker_stats_before_optimization is None
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.broker_stats()
    with pytest.raises(ccmi.UnsupportedOperationException):
        res.broker_stats_after_optimization
    with pytest.raises(ccmi.UnsupportedOperationException):
        res.load_json()
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)


def test_emu_optimizations_without_the_flag_is_unchanged(emu_lib):
    """The default path of optimizations() issues no new call: the same actions, proposals and device launches as a
    session that never heard of the flag, and no stats-launch beyond the goals' own."""
    runs = []
    for kwargs in ({}, dict(broker_stats=False)):
        buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
        cm = ccmi.ClusterModel.from_buffers(buf)
        res = ccmi.GoalOptimizer(constraint(1.05)).optimizations(cm, ccmi.goals_from_names(GOALS), **kwargs)
        p = cm.perf()
        runs.append((res.actions, [(g.name, g.succeeded, g.candidates, g.actions) for g in res.goal_results],
                     p.stats_launches, p.scan_launches + p.server_scans, p.accept_launches))
        assert res.broker_stats_before_optimization is None and res._stats_after is None
    assert runs[0] == runs[1] and runs[0][0]
