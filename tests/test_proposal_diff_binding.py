"""ccmi_proposal_diff on a library without it.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The diff is computed on
the device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the same and
ClusterModel.proposal_diff refuses with UnsupportedOperationException instead of answering on the host.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ccmi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)
STRUCTS = (("ccmi_proposal_record", "ProposalRecordStruct", 160), ("ccmi_proposal_summary", "ProposalSummaryStruct", 64))


def _read(*path):
    return open(os.path.join(REPO, *path)).read()


def test_symbol_is_additive_at_abi_13():
    header = _read("include", "ccmi.h")
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_proposal_diff" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_proposal_diff\(ccmi_session\* s, ccmi_proposal_record\* records[^;]*"
                     r"int64_t capacity,\s*int64_t\* num_records, ccmi_proposal_summary\* summary", header)
    for name, _, _ in STRUCTS:
        assert "typedef struct %s {" % name in header
    # the list at the top
    assert re.search(r"ccmi_proposal_diff\s+<- AnalyzerUtils\.getDiff / OptimizerResult\.getMovementStats", header)
    # the both-kinds case is in the contract
    assert "ExecutionProposal.java:81-84" in header and "counts as inter-broker" in header
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "proposal" in f]


def test_documents_name_the_entry_point():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ccmi_proposal_diff" in _read(doc), doc
    integration = _read("INTEGRATION.md")
    assert "ccmi_proposal_record" in integration and "ccmi_proposal_summary" in integration
    assert "proposal_diff.hip" in _read("DESIGN.md") and "proposal_diff_probe.py" in _read("README.md")


def test_struct_mirrors_match_the_header():
    header = _read("include", "ccmi.h")
    for name, mirror, size in STRUCTS:
        struct = getattr(ccmi, mirror)
        assert C.sizeof(struct) == size and np.dtype(struct).itemsize == size
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = []
        for decl in body.split(";"):
            words = decl.split()
            if words:
                ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}[words[0]]
                for field in "".join(words[1:]).split(","):
                    m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", field)
                    declared.append((m.group(1), ctype * int(m.group(2)) if m.group(2) else ctype))
        assert declared == list(struct._fields_), name
    rec = ccmi.ProposalRecordStruct
    assert (rec.partition.offset, rec.flags.offset, rec.old_replicas.offset, rec.new_replicas.offset,
            rec.old_disks.offset, rec.new_disks.offset) == (0, 20, 32, 64, 96, 128)
    assert ccmi.ProposalSummaryStruct.num_leadership_movements.offset == 40
    assert ccmi.ProposalSummaryStruct.reserved.offset == 48


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_proposal_diff is False
    assert not hasattr(emu_lib.lib, "ccmi_proposal_diff")


def test_emu_proposal_diff_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    for kwargs in ({}, dict(capacity=10), dict(summary_only=True)):
        with pytest.raises(ccmi.UnsupportedOperationException):
            cm.proposal_diff(**kwargs)
    assert cm.actions() == [] and cm.proposals() == []
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)
