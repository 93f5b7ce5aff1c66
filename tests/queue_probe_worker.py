"""Child process of test_queue_probe.py / test_queue_probe_gpu.py: one scenario of queue-scan probes
(ClusterModel._queue_probe, csrc/ccmi_queue_probe.cpp) in a fresh process, so the knobs in its environment
(CCMI_QUEUE_KEYED, CCMI_QUEUE_KEYED_STRIDE, CCMI_SERVER_BLOCKS) are the ones the library reads when it starts. A scenario
builds a seeded RandomCluster, optimizes a short chain so that the goals the probes name have device state, and runs its
probe lists; every probe goes to stdout as one JSON line {"name", "args", "rep"} and the parent does the asserting
(tests/queue_probe_support.py). Lists are chosen with the probe's host-loop-only mode (mode 2: nothing reaches the device),
so what is sent to the device does not depend on what the device answers.

usage: queue_probe_worker.py emu|gpu <scenario>"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "cruise-control_amd"))
sys.path.insert(0, HERE)

import ccmi  # noqa: E402

CHAIN = ["RackAwareGoal", "ReplicaCapacityGoal", "DiskCapacityGoal", "ReplicaDistributionGoal",
         "LeaderReplicaDistributionGoal"]
# the programs: the goal being optimized and its optimized goals, as the chain ran them
P_RD = ("ReplicaDistributionGoal", CHAIN[:3])
P_LRD = ("LeaderReplicaDistributionGoal", CHAIN[:4])
S_ALL = {}
S_LEAD = {"leaders": True, "score_res": 1}  # LeaderReplicaDistributionGoal's move-in view: leaders by NW_IN
S_EXCL = {"excl_topics": True}
S_LEAD_EXCL = {"leaders": True, "score_res": 1, "excl_topics": True}

WIDE = dict(num_racks=20, num_brokers=280, num_replicas=15000, num_topics=500)
DEAD = dict(num_racks=5, num_brokers=12, num_replicas=600, num_topics=30, num_dead_brokers=2)
HUGE = dict(num_racks=4, num_brokers=2800, num_replicas=8400, num_topics=300)
NS = (1, 2, 63, 64, 65, 255, 256, 257)


class Session:
    def __init__(self, which, props, excl_every=0, excl_lead=()):
        path = os.path.join(REPO, "tests", "emu", "libccmi_emu.so") if which == "emu" else \
            os.path.join(REPO, "cruise-control_amd", "libccmi.so")
        self.lib = ccmi.Library.get(path)
        self.buf = ccmi.RandomCluster.generate(self.lib, **props)
        self.cm = ccmi.ClusterModel(self.buf.desc, device=0, lib=self.lib, keepalive=self.buf)
        self.B = props["num_brokers"]
        T = self.buf.desc.num_topics
        # every topic but each excl_every-th is excluded: the *_EXCL Specs then select a few rows per broker
        excl = [t for t in range(T) if excl_every and t % excl_every != 0]
        opts = ccmi.OptimizationOptions(excluded_topics=excl, excluded_brokers_for_leadership=list(excl_lead))
        done = []
        for g in ccmi.goals_from_names(CHAIN, ccmi.BalancingConstraint()):
            g.optimize(self.cm, done, opts)
            done.append(g)
        self.count = 0

    def view(self, spec, b):
        return self.cm._queue_probe_view(spec, b)

    def sizes(self, spec):
        return [len(self.view(spec, b)) for b in range(self.B)]

    def ref(self, spec, prog, **kw):
        """The host loop's answer alone (mode 2): how the lists are chosen."""
        return self.cm._queue_probe(spec, prog[0], prog[1], mode=2, **kw)

    def probe(self, name, spec, prog, head=-1, skip_key=None, tail=(), cands=(), audit=True, **facts):
        tail, cands = [int(b) for b in tail], [int(b) for b in cands]
        rep = self.cm._queue_probe(spec, prog[0], prog[1], head=head, skip_key=skip_key, tail=tail, cands=cands,
                                   mode=0 if audit else 1)
        args = dict(spec=spec, prog=prog, head=head, skip_key=skip_key, tail=tail, cands=cands)
        if len(tail) > 64:
            args["tail"] = tail[:8] + ["...", len(tail)]
        print(json.dumps(dict(name=name, args=args, rep=rep, N=len(cands), n=len(tail) + (head >= 0), **facts)),
              flush=True)
        self.count += 1
        return rep

    def settle(self, spec, prog):
        """After many applied moves: the next scan carries more changed rows than a server command stages, so it is
        flattened and launched (Device::scanQueueImpl); the probes after it are served again. The parent does not ask
        this one for `served`."""
        self.probe("settle", spec, prog, tail=[0, 1], cands=[2])

    def rejecting(self, spec, prog):
        """The candidate brokers that accept no row of any other broker, and the rest."""
        rej = [c for c in range(self.B)
               if self.ref(spec, prog, tail=[b for b in range(self.B) if b != c], cands=[c])["ref"] is None]
        return rej, [c for c in range(self.B) if c not in set(rej)]

    def accepts(self, spec, prog, b, cands):
        return self.ref(spec, prog, tail=[b], cands=cands)["ref"] is not None


def pad(pool, k):
    return [pool[i % len(pool)] for i in range(k)]


def first_with(sizes, want):
    return next(b for b, s in enumerate(sizes) if s == want)


# ------------------------------------------------------------------------------------------------------ scenarios
def columns(which, prog="rd"):
    """One entry of 1, 3, 4, 5 and about 50 rows against N columns on both sides of the 256-slot tile and of the
    candidates' LDS limit: the natural list, lists whose only accepting column is the first or the last (the others
    are brokers that accept nothing, repeated as often as the list needs), and a list that accepts nothing."""
    s = Session(which, WIDE, excl_every=16)
    program, small, big = (P_RD, S_EXCL, S_ALL) if prog == "rd" else (P_LRD, S_LEAD_EXCL, S_LEAD)
    rej, acc = s.rejecting(big, program)
    assert len(rej) >= 2 and len(acc) >= 8, (len(rej), len(acc))
    sz_small, sz_big = s.sizes(small), s.sizes(big)
    by_size = sorted(range(s.B), key=lambda b: sz_big[b])
    if prog == "rd":
        blocks = [(small, first_with(sz_small, k)) for k in (1, 3, 4, 5)] + [(big, by_size[-1])]
    else:  # (no column accepts a leader of the few-row blocks: the leaders-only blocks as they are, 13 to 33 rows)
        blocks = [(big, by_size[0]), (big, by_size[len(by_size) // 2]), (big, by_size[-1])]
    for spec, b in blocks:
        rows = len(s.view(spec, b))
        one = next((c for c in acc if c != b and s.accepts(spec, program, b, [c])), None)
        for N in NS:
            tag = f"len{rows}_N{N}"
            s.probe(f"natural_{tag}", spec, program, tail=[b], cands=[c for c in range(s.B) if c != b][:N])
            s.probe(f"spread_{tag}", spec, program, tail=[b], cands=[c for c in range(s.B) if c != b][::-1][:N])
            s.probe(f"none_{tag}", spec, program, tail=[b], cands=pad(rej, N))
            if one is not None:
                s.probe(f"last_{tag}", spec, program, tail=[b], cands=pad(rej, N - 1) + [one])
                s.probe(f"first_{tag}", spec, program, tail=[b], cands=[one] + pad(rej, N - 1))
    # the largest block against single accepting columns among rejecting ones: which rows are accepted, and so where
    # the winner's slot lies among the accepted slots, changes with the column
    spec, b = blocks[-1]
    for i, c in enumerate([c for c in acc if c != b][:24]):
        for N in (65, 257):
            s.probe(f"one_column_{i}_N{N}", spec, program, tail=[b], cands=pad(rej, N // 2) + [c] + pad(rej, N - N // 2 - 1))
    return s


def single(which):
    """A single entry of 0, 1 and 2 rows; a winner in the entry's lowest-key, a higher-key and its highest-key row
    (asserted from the report's win_rank); no winner. Then the
    head continuation: skip_key at the head's lowest, a middle and its highest key (every head row masked: the tail
    wins), a head whose only accepted row is masked, and a head of one row."""
    s = Session(which, WIDE, excl_every=16)
    rej, acc = s.rejecting(S_ALL, P_RD)
    sz = s.sizes(S_EXCL)
    for k in (0, 1, 2):
        b = first_with(sz, k)
        s.probe(f"len{k}_all", S_EXCL, P_RD, tail=[b], cands=[c for c in range(s.B) if c != b][:5])
        s.probe(f"len{k}_none", S_EXCL, P_RD, tail=[b], cands=rej[:3])
    # a block of some rows and single columns: which row wins depends on the column
    b = max(range(s.B), key=lambda x: sz[x])
    keys = [k for k, _ in s.view(S_EXCL, b)]
    seen = {}
    for c in acc:
        r = s.ref(S_EXCL, P_RD, tail=[b], cands=[c])
        if r["ref"] is not None:
            seen.setdefault(keys.index(r["win_key"]), c)
    assert 0 in seen and len(seen) >= 2, seen
    top = max(seen)
    s.probe("winner_lowest_row", S_EXCL, P_RD, tail=[b], cands=[seen[0]])
    s.probe("winner_higher_row", S_EXCL, P_RD, tail=[b], cands=[seen[top]])
    s.probe("winner_rows_mixed", S_EXCL, P_RD, tail=[b], cands=[seen[top], rej[0], seen[0]])
    # the winner in the entry's highest-key row: every row before it is rejected, so the reduction ends on the last key.
    # The longest blocks of this Spec that have such a column, one of them with rejecting columns around it.
    last = []
    for hb in sorted((x for x in range(s.B) if sz[x] >= 2), key=lambda x: -sz[x]):
        c = next((c for c in acc if c != hb and (lambda r: r["ref"] is not None and r["win_rank"] == r["win_len"] - 1)(
            s.ref(S_EXCL, P_RD, tail=[hb], cands=[c]))), None)
        if c is not None:
            last.append((hb, c))
        if len(last) == 3:
            break
    assert last, "no block of two or more rows has a column that accepts only its highest-key row"
    for i, (hb, c) in enumerate(last):
        s.probe(f"winner_highest_row_{i}", S_EXCL, P_RD, tail=[hb], cands=[c], rows=sz[hb])
    hb, c = last[0]
    s.probe("winner_highest_row_N65", S_EXCL, P_RD, tail=[hb], cands=pad(rej, 40) + [c] + pad(rej, 24), rows=sz[hb])
    # continuation on a head of many rows (the all-replicas view), tail of two brokers
    hs = s.sizes(S_ALL)
    head = max(range(s.B), key=lambda x: hs[x])
    hk = [k for k, _ in s.view(S_ALL, head)]
    tail = [c for c in acc if c != head][:2]
    cands = [c for c in acc if c != head and c not in tail][:3]
    for name, key in (("lowest", hk[0]), ("middle", hk[len(hk) // 2]), ("highest", hk[-1]), ("below_all", 0)):
        s.probe(f"head_skip_{name}", S_ALL, P_RD, head=head, skip_key=key, tail=tail, cands=cands)
        s.probe(f"head_skip_{name}_N65", S_ALL, P_RD, head=head, skip_key=key, tail=tail,
                cands=[c for c in range(s.B) if c != head and c not in tail][:65])
    s.probe("head_no_skip", S_ALL, P_RD, head=head, tail=tail, cands=cands)
    # the head's only accepted row is masked: a block of several rows and a column that accepts exactly one of them
    found = None
    for hb in (x for x in range(s.B) if 2 <= sz[x] <= 6):
        for c in acc[:80]:
            r = s.ref(S_EXCL, P_RD, tail=[hb], cands=[c])
            if c != hb and r["ref"] is not None and r["accepted_rows"] == 1:
                found = (hb, c, r["win_key"])
                break
        if found:
            break
    assert found, "no column accepts exactly one row of a small block"
    hb, c, key = found
    other = [x for x in acc if x not in (hb, c)][:2]
    s.probe("head_only_accept_masked", S_EXCL, P_RD, head=hb, skip_key=key, tail=other, cands=[c])
    s.probe("head_only_accept_kept", S_EXCL, P_RD, head=hb, skip_key=key - 1, tail=other, cands=[c])
    b1 = first_with(sz, 1)
    k1 = s.view(S_EXCL, b1)[0][0]
    t1 = [c for c in acc if c != b1][:3]
    for name, key in (("masked", k1), ("kept", k1 - 1)):
        s.probe(f"head_len1_{name}", S_EXCL, P_RD, head=b1, skip_key=key, tail=t1, cands=[c for c in acc if c != b1][3:8])
    return s


def multi(which, only_heads=False):
    """Several entries per workgroup (CCMI_SERVER_BLOCKS=8): n of 9, 16, 17 and 40 entries with empty ones between the
    others, the one accepting entry first in its workgroup, later in it (entry 8, workgroup 0's second; from n = 17 on
    entry 16 follows it on that workgroup with rows of its own, so the tile that ends entry 8 also holds rows of the
    next entry) and last of all; two accepting entries on different workgroups, the lower-numbered one winning; a head
    whose rows are all masked by the largest skip_key. only_heads: those head probes alone."""
    s = Session(which, WIDE, excl_every=16)
    spec, prog = S_LEAD, P_LRD
    # four brokers give their leaderships away: their blocks are empty under the leaders-only Spec
    lead = s.cm.leader_distribution()
    byp, byb = _placement(s)
    empty = [276, 277, 278, 279]
    for e in empty:
        for p in byb[e]:
            if lead[p] == e:
                s.cm.apply([(1, p, e, next(b for b in byp[p] if b not in empty), -1, -1, -1)])
    sz = s.sizes(spec)
    assert all(sz[e] == 0 for e in empty)
    s.settle(spec, prog)
    _, acc = s.rejecting(spec, prog)
    for N in (1, 3, 70):
        cands = acc[:N]
        rest = [b for b in range(s.B) if b not in cands and sz[b] > 0]
        yes = [b for b in rest if s.accepts(spec, prog, b, cands)]
        no = [b for b in rest if b not in set(yes)]
        assert len(yes) >= 2 and len(no) >= 40, (N, len(yes), len(no))
        for n in (9, 16, 17, 40):
            fill = no[:n]
            for k, e in enumerate(empty[:4]):  # empty entries between the others
                if 2 + 3 * k < n - 1:
                    fill[2 + 3 * k] = e
            q = list(fill)
            q[8] = yes[0]  # every row of the head masked: the tail's entry 8 (entry 9 of the queue) wins
            s.probe(f"N{N}_n{n}_head", spec, prog, head=yes[1], skip_key=(1 << 64) - 1, tail=q[:n - 1],
                    cands=cands)
            if only_heads:
                continue
            for name, pos in (("first_of_wg", 3), ("later_in_wg", 8), ("last", n - 1)):
                q = list(fill)
                q[pos] = yes[0]
                # rows of the entry that follows `pos` on its workgroup (8 workgroups), 0: none follows
                s.probe(f"N{N}_n{n}_{name}", spec, prog, tail=q, cands=cands,
                        next_rows=sz[q[pos + 8]] if pos + 8 < n else 0)
            q = list(fill)
            q[8], q[5] = yes[0], yes[1]  # entry 8 is workgroup 0's second, entry 5 workgroup 5's first: 5 wins
            s.probe(f"N{N}_n{n}_other_wg_wins", spec, prog, tail=q, cands=cands)
            s.probe(f"N{N}_n{n}_none", spec, prog, tail=fill, cands=cands)
    if only_heads:
        return s
    # the natural queue: every entry may accept
    order = [b for b in range(s.B) if b not in acc[:2]]
    for n in (17, 40):
        s.probe(f"natural_n{n}", spec, prog, tail=order[:n], cands=acc[:2])
        s.probe(f"natural_n{n}_rev", S_ALL, P_RD, tail=order[::-1][:n], cands=acc[:2][::-1])
    return s


def batch2(which):
    """More than 256 entries per workgroup (CCMI_SERVER_BLOCKS=8 and 2,049 or more entries): the winner beyond entry
    2,048, which only the second batch of the workgroup's loop reaches, and in the first batch."""
    t0 = time.perf_counter()
    s = Session(which, HUGE)
    sz = s.sizes(S_ALL)
    order = [b for b in range(s.B) if sz[b] <= 8]  # (a few brokers of this cluster hold hundreds of rows)
    for c in order[8:200:16]:  # a column that 2,049 or more brokers' leaders are not accepted by, and some are
        yes = [b for b in order if b != c and s.accepts(S_LEAD, P_LRD, b, [c])]
        no = [b for b in order if b != c and b not in set(yes)]
        if len(no) >= 2049 and len(yes) >= 2:
            break
    assert len(no) >= 2049 and len(yes) >= 2, (len(no), len(yes))
    other = next(x for x in order[9:] if x != c and not s.accepts(S_LEAD, P_LRD, yes[0], [x]))
    s.probe(f"winner_entry_{len(no)}", S_LEAD, P_LRD, tail=no + yes, cands=[c])
    s.probe("winner_entry_2049", S_LEAD, P_LRD, tail=no[:2049] + yes[:1], cands=[c], audit=False)
    s.probe("winner_entry_2049_of_N2", S_LEAD, P_LRD, tail=[b for b in no if b != other][:2049] + yes[:1],
            cands=[other, c], audit=False)
    s.probe("winner_first_batch", S_LEAD, P_LRD, tail=no[:900] + yes[:1] + no[900:], cands=[c], audit=False)
    s.probe("winner_first_entry", S_LEAD, P_LRD, tail=yes[1:2] + no, cands=[c], audit=False)
    s.probe("no_winner", S_LEAD, P_LRD, tail=no, cands=[c], audit=False)
    s.probe("all_rows_N1", S_ALL, P_RD, tail=[b for b in order if b != c][::-1], cands=[c], audit=False)
    print(json.dumps(dict(seconds=time.perf_counter() - t0)), flush=True)
    return s


def highbits(which):
    """Keys with bit 63 or 62 set next to keys without: prio_offline on a cluster with dead brokers (the rows of a dead
    broker sort first), prio_immigrants after applied moves (the moved replicas sort first on their new broker)."""
    s = Session(which, DEAD)
    B = s.B
    spec = {"prio_offline": True, "score_res": 3}
    for N in (1, 3, 11):
        for prog, pn in ((P_RD, "rd"), (P_LRD, "lrd")):
            s.probe(f"offline_{pn}_N{N}", spec, prog, tail=list(range(B))[::-1], cands=list(range(B))[:N])
            s.probe(f"offline_leaders_{pn}_N{N}", dict(spec, leaders=True), prog, tail=list(range(B)),
                    cands=list(range(B))[::-1][:N])
    imm = {"prio_immigrants": True, "score_res": 0, "reverse": True}
    moves = _some_moves(s, 6)
    s.cm.apply(moves)
    for N in (1, 4, 12):
        s.probe(f"immigrants_N{N}", imm, P_RD, tail=list(range(B)), cands=list(range(B))[::-1][:N])
        s.probe(f"immigrants_offline_N{N}", dict(imm, prio_offline=True), P_LRD, tail=list(range(B))[::-1],
                cands=list(range(B))[:N])
    # replicas moved onto a dead broker are offline there: their keys have bit 63 clear under prio_offline
    dead = [b for b in range(B) if s.buf.desc.broker_state[b] != 0]
    byp, _ = _placement(s)
    onto = [(0, p, byp[p][0], dead[0], -1, -1, -1) for p in sorted(byp)[1:13:3] if dead[0] not in byp[p]]
    s.cm.apply(onto)
    for N in (2, 12):
        s.probe(f"offline_rows_N{N}", dict(imm, prio_offline=True), P_RD, tail=list(range(B)),
                cands=list(range(B))[::-1][:N])
        s.probe(f"offline_rows_leaders_N{N}", {"prio_offline": True, "leaders": True, "score_res": 1}, P_LRD,
                tail=list(range(B))[::-1], cands=list(range(B))[:N])
    keys = [k for b in range(B) for k, _ in s.view(dict(imm, prio_offline=True), b)]
    print(json.dumps(dict(key_bits=[sum(1 for k in keys if k >> 63), sum(1 for k in keys if (k >> 62) & 1),
                                    sum(1 for k in keys if not k >> 62)])), flush=True)
    return s


def _placement(s):
    """{partition: brokers} and {broker: partitions} of the session's current model."""
    dist = s.cm.replica_distribution()
    d = s.buf.desc
    byp, byb = {}, {}
    for p in range(d.num_partitions):
        for i in range(d.partition_offset[p], d.partition_offset[p + 1]):
            byp.setdefault(p, []).append(dist[i])
            byb.setdefault(dist[i], []).append(p)
    return byp, byb


def _some_moves(s, k):
    byp, byb = _placement(s)
    moves = []
    for p in sorted(byp)[:k * 3:3]:
        dst = next(b for b in range(s.B - 1, -1, -1) if b not in byp[p])
        moves.append((0, p, byp[p][-1], dst, -1, -1, -1))
    return moves


def changes(which):
    """Probes and table audits between applied moves: a replica away from its block's last slot, from slot 0 and from a
    middle slot, a move that empties a broker's block, one that grows a block, a leadership move under the leaders-only
    Spec (there it makes one row leave a block and another join one: a leaders-only block holds no row whose key a
    leadership move changes); then another Spec (a full rebuild), all replicas by NW_OUT, under which a leadership move
    does rewrite two keys in place, and back."""
    s = Session(which, WIDE, excl_every=16)
    B = s.B
    _, acc = s.rejecting(S_ALL, P_RD)
    _, acc_l = s.rejecting(S_LEAD, P_LRD)
    src = 7
    focus = [src]  # the brokers whose blocks changed: the probes' first entries

    def both(name):
        rest = [b for b in range(B) if b not in focus]
        for tag, spec, prog, pool in (("all", S_ALL, P_RD, acc), ("leaders", S_LEAD, P_LRD, acc_l),
                                      ("few", S_LEAD_EXCL, P_LRD, acc_l)):
            cands = [c for c in pool if c not in focus][:6]
            tail = focus + [b for b in rest if b not in cands][:20]
            s.probe(f"{name}_{tag}", spec, prog, tail=tail, cands=cands)
            s.probe(f"{name}_{tag}_rev", spec, prog, tail=tail[::-1], cands=cands[::-1])

    both("start")
    part_of = s.buf.desc.replica_partition
    for name, pick in (("last_slot", -1), ("slot0", 0), ("middle_slot", None)):
        byp, byb = _placement(s)
        # the block's rows by slot (the table holds S_ALL's rows after the probe before; without a table: by key)
        s.probe(f"before_{name}", S_ALL, P_RD, tail=focus, cands=acc[:3])
        rows = sorted(s.cm._queue_probe_view(S_ALL, src, slots=True), key=lambda x: (x[2], x[0]))
        p = part_of[rows[pick if pick is not None else len(rows) // 2][1]]
        dst = next(b for b in acc if b not in byp[p] and b not in focus)
        s.cm.apply([(0, p, src, dst, -1, -1, -1)])  # the destination's block grows by one
        focus.append(dst)
        assert len(s.view(S_ALL, src)) == len(rows) - 1
        both(f"after_{name}")
    # empty a broker's leaders-only excluded-topics block (a few rows)
    sz = s.sizes(S_LEAD_EXCL)
    e = next(b for b in range(B) if 1 <= sz[b] <= 3 and b not in focus)
    focus.insert(0, e)
    both("before_emptying")
    for _, r in s.view(S_LEAD_EXCL, e):
        byp, _ = _placement(s)
        p = part_of[r]
        s.cm.apply([(0, p, e, next(b for b in acc if b not in byp[p] and b not in focus), -1, -1, -1)])
        both("while_emptying")
    assert len(s.view(S_LEAD_EXCL, e)) == 0
    # a leadership move: a follower on `src` becomes the leader (its row joins the leaders-only block with a new key),
    # the old leader's row leaves its broker's block; under S_ALL neither row moves
    lead = s.cm.leader_distribution()
    byp, byb = _placement(s)
    p = next(p for p in byb[src] if lead[p] != src)
    focus.insert(0, lead[p])
    both("before_leadership")
    s.cm.apply([(1, p, lead[p], src, -1, -1, -1)])
    both("after_leadership")
    # another Spec (a full rebuild): every replica by NW_OUT, where a leadership move changes both replicas' scores, so
    # the next sync rewrites two keys in place
    nw_out = {"score_res": 2, "reverse": True}
    s.probe("other_spec", nw_out, P_RD, tail=focus, cands=acc[:4])
    lead = s.cm.leader_distribution()
    p = next(p for p in byb[src] if lead[p] != src)
    before = dict((r, k) for b in (src, lead[p]) for k, r in s.view(nw_out, b))
    s.cm.apply([(1, p, lead[p], src, -1, -1, -1)])
    after = dict((r, k) for b in (src, lead[p]) for k, r in s.view(nw_out, b))
    assert set(before) == set(after) and sum(1 for r in before if before[r] != after[r]) == 2
    s.probe("other_spec_keys_rewritten", nw_out, P_RD, tail=focus, cands=acc[:4])
    s.probe("other_spec_keys_rewritten_rev", nw_out, P_RD, tail=focus[::-1], cands=acc[:4][::-1])
    both("back_after_rebuild")
    return s


def excl_lead(which):
    """Brokers excluded for leadership in the last optimization: a leader row's move into one of them is blocked on
    the device (exclLeadBlocked) and in the host loop (Engine::blocked), so columns are filtered per row."""
    ex = list(range(0, 280, 2))
    s = Session(which, WIDE, excl_every=16, excl_lead=ex)
    _, acc = s.rejecting(S_ALL, P_RD)  # excluded and other brokers alternate in it
    assert sum(1 for c in acc[:64] if c % 2 == 0) >= 8
    for N in (1, 2, 65, 257):
        for spec, sn in ((S_ALL, "all"), (S_LEAD, "leaders"), (S_LEAD_EXCL, "few")):
            cands = acc[:N]
            tail = [b for b in range(s.B) if b not in cands[:64]][:30]
            s.probe(f"excl_{sn}_N{N}", spec, P_RD, tail=tail, cands=cands)
            s.probe(f"excl_{sn}_N{N}_rev", spec, P_RD, tail=tail[::-1], cands=cands[::-1])
    return s


def full_block(which):
    """The all-replicas view whose longest block is exactly the table's stride (CCMI_QUEUE_KEYED_STRIDE, set by the
    parent from the `longest` this scenario printed on an earlier run), or one more than it: the Spec is then refused and
    the snapshot directory serves the scan."""
    s = Session(which, WIDE, excl_every=16)
    sz = s.sizes(S_ALL)
    big = max(range(s.B), key=lambda b: sz[b])
    print(json.dumps(dict(longest=sz[big])), flush=True)
    others = [b for b in range(s.B) if b != big]
    for N in (1, 5, 257):
        s.probe(f"full_block_alone_N{N}", S_ALL, P_RD, tail=[big], cands=others[:N])
        s.probe(f"full_block_in_queue_N{N}", S_ALL, P_RD, tail=others[-3:] + [big] + others[-6:-3], cands=others[:N])
    s.probe("full_block_head", S_ALL, P_RD, head=big, skip_key=s.view(S_ALL, big)[sz[big] // 2][0], tail=others[-3:],
            cands=others[:7])
    return s


SCENARIOS = dict(columns_rd=lambda w: columns(w, "rd"), columns_lrd=lambda w: columns(w, "lrd"), single=single,
                 multi=multi, multi_heads=lambda w: multi(w, only_heads=True), batch2=batch2, highbits=highbits, changes=changes, excl_lead=excl_lead,
                 full_block=full_block)


def main():
    which, name = sys.argv[1], sys.argv[2]
    s = SCENARIOS[name](which)
    print(json.dumps(dict(done=s.count)), flush=True)
    del s


if __name__ == "__main__":
    main()
