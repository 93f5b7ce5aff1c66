"""ccmi_sorted_replicas on a library without it, and the restatement the GPU tests compare with.

The entry point is additive at ABI v13 and its capability flag is the presence of the symbol. The lists are selected and
sorted on the device only, so the CPU tests' emulation build (tests/emu) does not export it: the binding loads all the
same and ClusterModel.sorted_replicas refuses with UnsupportedOperationException instead of answering on the host.
"""
import ctypes as C
import os
import re

import pytest

import ccmi
from sorted_replicas_support import double_bits, double_compare, sort_tuples, string_compare

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = dict(num_racks=5, num_brokers=20, num_replicas=6000, num_topics=300)


def _read(*path):
    return open(os.path.join(REPO, *path)).read()


def test_symbol_is_additive_at_abi_13():
    header = _read("include", "ccmi.h")
    assert int(re.search(r"#define CCMI_ABI_VERSION (\d+)", header).group(1)) == 13 == ccmi.ABI_VERSION
    assert "ccmi_sorted_replicas" in ccmi.EXPORTED_SYMBOLS
    assert re.search(r"ccmi_status ccmi_sorted_replicas\(ccmi_session\* s, const ccmi_sorted_replicas_query\* q,\s*"
                     r"const int32_t\* brokers[^;]*int64_t n, int64_t\* offsets[^;]*ccmi_swap_replica\* records[^;]*"
                     r"double\* scores[^;]*int64_t capacity, int64_t\* num_records, int64_t\* first_invalid", header)
    assert "typedef struct ccmi_sorted_replicas_query {" in header
    assert re.search(r"ccmi_sorted_replicas\s+<- SortedReplicas\.sortedReplicas", header)  # the list at the top
    for name, value in (("CCMI_SEL_LEADERS", 1), ("CCMI_SEL_FOLLOWERS", 2), ("CCMI_SEL_ONLINE", 4),
                        ("CCMI_SEL_OFFLINE", 8), ("CCMI_SEL_IMMIGRANTS", 16), ("CCMI_SEL_IMMIGRANT_OR_OFFLINE", 32),
                        ("CCMI_PRIO_OFFLINE", 0), ("CCMI_PRIO_IMMIGRANTS", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    assert (ccmi.SEL_LEADERS, ccmi.SEL_FOLLOWERS, ccmi.SEL_ONLINE, ccmi.SEL_OFFLINE, ccmi.SEL_IMMIGRANTS,
            ccmi.SEL_IMMIGRANT_OR_OFFLINE) == (1, 2, 4, 8, 16, 32)
    assert ccmi.SORT_PRIORITIES == ("offline", "immigrants")
    # the perf counters are the ones ccmi_actions_acceptance added: no new fields
    fields = [f for f, _ in ccmi.PerfStruct._fields_]
    assert fields[-3:] == ["accept_launches", "accept_cells", "accept_kernel_ms"]
    assert len(fields) == len(set(fields)) and not [f for f in fields if "sorted" in f]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):  # with the header: the four documents
        assert "ccmi_sorted_replicas" in _read(doc), doc
    assert "K15 measured" in _read("DESIGN.md")
    integration = _read("INTEGRATION.md")
    assert "eligibleBrokers" in integration and "eligibleReplicasForSwap" in integration


def test_struct_mirror_matches_the_header():
    assert C.sizeof(ccmi.SortedReplicasQueryStruct) == 64
    header = _read("include", "ccmi.h")
    name = "ccmi_sorted_replicas_query"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:  # "double  above_limit, below_limit": the type, then the declarators
            first, *more = decl.split(",")
            for d in [first.split()[-1]] + [m.strip() for m in more]:
                declared.append(re.sub(r"\[\d+\]", "", d).lstrip("*"))
    assert declared == [f for f, _ in ccmi.SortedReplicasQueryStruct._fields_]
    # the fields a shim reads at fixed offsets
    assert ccmi.SortedReplicasQueryStruct.priorities.offset == 8
    assert ccmi.SortedReplicasQueryStruct.above_limit.offset == 32
    assert ccmi.SortedReplicasQueryStruct.topic_excluded.offset == 48
    assert ccmi.SortedReplicasQueryStruct.topic_included.offset == 56


def test_emu_loads_without_the_symbol(emu_lib):
    assert emu_lib.lib.ccmi_abi_version() == 13
    assert emu_lib.has_sorted_replicas is False
    assert not hasattr(emu_lib.lib, "ccmi_sorted_replicas")


def test_emu_sorted_replicas_is_unsupported(emu_lib):
    buf = ccmi.RandomCluster.generate(emu_lib, **PROPS)
    cm = ccmi.ClusterModel.from_buffers(buf)
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.sorted_replicas()  # a fresh session
    with pytest.raises(ccmi.UnsupportedOperationException):
        cm.sorted_replicas([1, 0], leaders=True, priorities=("offline", "immigrants"), score="DISK", reverse=True,
                           above=("CPU", 0.5), excluded_topics=["T1"], with_scores=True)
    assert cm.actions() == []
    p = cm.perf()
    assert (p.accept_launches, p.accept_cells, p.accept_kernel_ms) == (0, 0, 0.0)


def test_restatement_on_a_hand_made_broker():
    """Tuples (priority offline, priority immigrants, score, offline, partition number, original broker id, topic) of one
    broker, written in the order SortedReplicas must give them; the restatement's comparator finds that order from any
    shuffle, and so does Python's sorted on an explicit key that spells the same rules another way."""
    ordered = [
        # class 1: offline and immigrant (0, 0): by score
        (0, 0, -3.0, True, 7, 1, "a"),
        (0, 0, 2.5, True, 1, 1, "a"),
        # class 2: offline, not immigrant: an offline replica with a large partition number and the smaller score first
        (0, 1, 1.0, True, 900, 2, "z"),
        (0, 1, 1.5, True, 0, 2, "a"),
        # class 3: online immigrants: -0.0 sorts below 0.0 whatever the tail says
        (1, 0, -0.0, False, 50, 9, "z"),
        (1, 0, 0.0, False, 1, 0, "a"),
        (1, 0, 0.0, False, 1, 0, "b"),    # equal up to the topic name
        (1, 0, 0.0, False, 1, 3, "a"),    # then the original broker id
        (1, 0, 0.0, False, 2, 0, "a"),    # then the partition number
        # class 4: online natives, equal scores: compareTo puts the offline one first (offline without the priority's
        # say-so cannot happen under prioritizeOfflineReplicas, so this class is checked again without priorities below)
        (1, 1, 4.0, False, 3, 5, "B"),    # "B" < "a": code units, not case-folded
        (1, 1, 4.0, False, 3, 5, "a"),
        (1, 1, 4.0, False, 3, 5, "ab"),   # a prefix sorts first
        # class 5: the largest score last
        (1, 1, 1e30, False, 0, 0, "a"),
    ]
    import random
    for seed in range(5):
        shuffled = ordered[:]
        random.Random(seed).shuffle(shuffled)
        assert sort_tuples(shuffled, 2, True) == ordered
        explicit = sorted(shuffled, key=lambda t: (t[0], t[1], (t[2], 0 if double_bits(t[2]) < 0 else 1), not t[3], t[4],
                                                   t[5], t[6].encode("utf-16-be")))
        assert explicit == ordered
    # no priorities, no score: Replica.compareTo alone, the offline replica first whatever its partition number
    plain = [(0.0, True, 100000, 9, "z"), (0.0, False, 0, 0, "a"), (0.0, False, 0, 1, "a"), (0.0, False, 1, 0, "a")]
    for seed in range(3):
        shuffled = plain[:]
        random.Random(seed).shuffle(shuffled)
        assert sort_tuples(shuffled, 0, False) == plain
    # the score is ignored without a score function
    assert sort_tuples([(5.0, False, 1, 0, "a"), (1.0, False, 0, 0, "a")], 0, False)[0][2] == 0
    assert double_compare(-0.0, 0.0) == -1 and double_compare(0.0, -0.0) == 1 and double_compare(0.0, 0.0) == 0
    assert double_compare(-1.0, -0.0) == -1 and double_compare(float("-inf"), -1e38) == -1
    assert string_compare("B", "a") == -1 and string_compare("a", "ab") == -1 and string_compare("b", "ab") == 1
