"""ccmi_partition_load on a library without it.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The response is keyed and
sorted on the device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the
same and ClusterModel.partition_load refuses with UnsupportedOperationException instead of answering on the host.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ccmi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)


def _read(*path):
    return open(os.path.join(REPO, *path)).read()


def test_symbol_is_additive_at_abi_13():
    header = _read("include", "ccmi.h")
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_partition_load" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_partition_load\(ccmi_session\* s, const ccmi_partition_load_query\* q,\s*"
                     r"ccmi_partition_load_record\* records[^;]*int64_t\* num_records, int64_t\* num_selected", header)
    assert "typedef struct ccmi_partition_load_query {" in header
    assert "typedef struct ccmi_partition_load_record {" in header
    assert re.search(r"ccmi_partition_load\s+<- PartitionLoadRunnable\.getResult", header)  # the list at the top
    # the contract's argument for max mode and the left-out metric are in the header
    assert "Float.MIN_VALUE" in header and "MESSAGE_IN_RATE" in header
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "partition_load" in f]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ccmi_partition_load" in _read(doc), doc
    assert "tie_rank" in _read("INTEGRATION.md") and "msg_in" in _read("INTEGRATION.md")


def test_struct_mirrors_match_the_header():
    assert C.sizeof(ccmi.PartitionLoadQueryStruct) == 64
    assert C.sizeof(ccmi.PartitionLoadRecordStruct) == 80
    assert np.dtype(ccmi.PartitionLoadRecordStruct).itemsize == 80
    header = _read("include", "ccmi.h")
    for name, struct in (("ccmi_partition_load_query", ccmi.PartitionLoadQueryStruct),
                         ("ccmi_partition_load_record", ccmi.PartitionLoadRecordStruct)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                declared.append(re.sub(r"\[\d+\]", "", decl.split()[-1]).lstrip("*"))
        assert declared == [f for f, _ in struct._fields_], name
    # the fields a shim reads at fixed offsets
    assert ccmi.PartitionLoadQueryStruct.topic_selected.offset == 40
    assert ccmi.PartitionLoadQueryStruct.tie_rank.offset == 56
    assert ccmi.PartitionLoadRecordStruct.partition.offset == 32
    assert ccmi.PartitionLoadRecordStruct.brokers.offset == 40
    assert ccmi.PartitionLoadRecordStruct.reserved.offset == 72


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_partition_load is False
    assert not hasattr(emu_lib.lib, "ccmi_partition_load")


def test_emu_partition_load_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.partition_load()  # a fresh session
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.partition_load("CPU", max_load=True, entries=10, topic="T.*", partition_range=(0, 3), broker_ids=[1])
    assert cm.actions() == []
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)
