"""The reference of the proposal diff tests.

Where the oracle ran the chain itself, the expected proposals are OracleCluster.proposals(): its own getDiff over the
optimization. The oracle computes that list only inside optimize(), against the placement the call started from, so for
actions applied from outside (oc.apply) the expected proposals are `restated_diff`: AnalyzerUtils.getDiff
(AnalyzerUtils.java:63-93) restated in a few lines over the oracle's own replica, disk and leader distributions before
and after, with the partition size from partition_load_support.Restatement (which test_partition_load_reference.py pins
to the oracle). The chain tests assert restated_diff == OracleCluster.proposals(), which pins the restatement.

`classify` and `movement_stats` restate ExecutionProposal.java:72-78, :212-221 and OptimizerResult.getMovementStats
(OptimizerResult.java:258-278) over a list of ExecutionProposals.
"""
import ctypes as C

import numpy as np

import ccmi
from partition_load_support import DEFAULT, DISK, Restatement

RECORD = np.dtype(ccmi.ProposalRecordStruct)
SENTINEL = 0xA5
SUMMARY_FIELDS = [f for f, _ in ccmi.ProposalSummaryStruct._fields_ if f != "reserved"]


class OracleState:
    """The oracle's placement now: brokers and disks of every slot in Partition._replicas order, the leaders' brokers."""

    def __init__(self, oc):
        self.dist, self.disks, self.leaders = oc.replica_distribution(), oc.replica_disks(), oc.leader_distribution()


def restated_diff(desc, init, oc):
    """getDiff of the oracle's current placement against `init` (an OracleState taken before any action)."""
    now = OracleState(oc)
    sizes = Restatement(desc).apply(oc.actions())
    off = list(desc.partition_offset[:desc.num_partitions + 1])
    out = []
    for p in range(desc.num_partitions):
        a, b = off[p], off[p + 1]
        old_r, new_r, old_d, new_d = init.dist[a:b], now.dist[a:b], init.disks[a:b], now.disks[a:b]
        old_leader, leader = (init.leaders[p], old_d[old_r.index(init.leaders[p])]), \
                             (now.leaders[p], new_d[new_r.index(now.leaders[p])])
        if old_r == new_r and old_d == new_d and old_leader == leader:  # :80
            continue
        pos = list(zip(new_r, new_d)).index(leader)  # :84-88: indexOf, then positions 0 and pos swap
        new_r[0], new_r[pos] = new_r[pos], new_r[0]
        new_d[0], new_d[pos] = new_d[pos], new_d[0]
        out.append(ccmi.ExecutionProposal(p, int(sizes.util(p, DISK, DEFAULT)), old_leader[0], old_r, new_r, old_d, new_d))
    return out


def classify(p):
    """(flags, num_to_add, num_to_remove, num_between_disks, old_leader_disk) of one ExecutionProposal."""
    old_pl, new_pl = list(zip(p.old_replicas, p.old_disks)), list(zip(p.new_replicas, p.new_disks))
    old_b, new_b = set(p.old_replicas), set(p.new_replicas)
    to_add = {pl for pl in new_pl if pl[0] not in old_b}
    to_remove = {pl for pl in old_pl if pl[0] not in new_b}
    between = {pl[0] for pl in new_pl if pl not in to_add and pl not in old_pl}
    old_leader_disk = p.old_disks[p.old_replicas.index(p.old_leader)]
    flags = (1 if set(old_pl) != set(new_pl) else 0) | (2 if (p.old_leader, old_leader_disk) != new_pl[0] else 0)
    return flags, len(to_add), len(to_remove), len(between), old_leader_disk


def movement_stats(proposals):
    """[inter-broker movements, inter MB, intra-broker movements, intra MB, leadership movements]."""
    n_inter = mb_inter = n_intra = mb_intra = n_lead = 0
    for p in proposals:
        _, add, remove, between, _ = classify(p)
        if add or remove:
            n_inter += 1
            mb_inter += add * p.partition_size
        elif between:
            n_intra += between
            mb_intra += p.partition_size * between
        else:
            n_lead += 1
    return [n_inter, mb_inter, n_intra, mb_intra, n_lead]


def columns(records):
    """The records field by field as seven columns: partition, size, old leader, old replicas, new replicas, old disks,
    new disks (the lists cut to num_replicas; the slots past it must be -1)."""
    cols = ([], [], [], [], [], [], [])
    for r in records:
        n = int(r["num_replicas"])
        assert 1 <= n <= 8
        for name in ("old_replicas", "new_replicas", "old_disks", "new_disks"):
            assert [int(x) for x in r[name][n:]] == [-1] * (8 - n), (int(r["partition"]), name)
        cols[0].append(int(r["partition"]))
        cols[1].append(int(r["size"]))
        cols[2].append(int(r["old_leader"]))
        for c, name in zip(cols[3:], ("old_replicas", "new_replicas", "old_disks", "new_disks")):
            c.append([int(x) for x in r[name][:n]])
    return cols


def columns_of(proposals):
    return ([p.partition for p in proposals], [p.partition_size for p in proposals], [p.old_leader for p in proposals],
            [list(p.old_replicas) for p in proposals], [list(p.new_replicas) for p in proposals],
            [list(p.old_disks) for p in proposals], [list(p.new_disks) for p in proposals])


def summary_tuple(s):
    assert list(s.reserved) == [0, 0]
    return tuple(int(getattr(s, f)) for f in SUMMARY_FIELDS)


def expected_summary(want):
    return tuple([len(want)] + movement_stats(want))


def check(cm, want):
    """Everything a full call returns against the expected proposals `want`: the seven columns in order, the host
    path, each record's flags and counts, the summary. Returns the ProposalDiff."""
    diff = cm.proposal_diff()
    got, exp = columns(diff.records), columns_of(want)
    for g, e, name in zip(got, exp, ("partition", "size", "old_leader", "old_replicas", "new_replicas", "old_disks",
                                     "new_disks")):
        assert g == e, name
    assert diff.proposals == want
    assert cm.proposals() == want  # the host path
    for r, p in zip(diff.records, want):
        flags, add, _, between, old_leader_disk = classify(p)
        assert (int(r["flags"]), int(r["num_to_add"]), int(r["num_between_disks"]), int(r["old_leader_disk"])) == \
               (flags, add, between, old_leader_disk), p
    assert summary_tuple(diff.summary) == expected_summary(want)
    assert diff.movement_stats() == movement_stats(want) and diff.num_proposals == len(want)
    assert summary_tuple(cm.proposal_diff(summary_only=True).summary) == expected_summary(want)
    return diff


def raw_call(cm, capacity, room=None, with_summary=True):
    """ccmi_proposal_diff through ctypes into a sentinel-filled buffer with room for `room` records (default: the
    capacity). Returns (status, the buffer as bytes, num_records, summary)."""
    room = capacity if room is None else room
    buf = np.full(max(1, room) * RECORD.itemsize, SENTINEL, dtype=np.uint8)
    n, summary = C.c_int64(-1), ccmi.ProposalSummaryStruct()
    st = cm.lib.lib.ccmi_proposal_diff(cm.handle, buf.ctypes.data, capacity, C.byref(n),
                                       C.byref(summary) if with_summary else None)
    return st, buf.tobytes(), n.value, summary
