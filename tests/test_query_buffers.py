"""The device memory of the session queries and of the aggregator family across calls (engine/devbuf.h): outputs that
regrow between calls, queries whose blocks are neighbours interleaved with changes of the model, and every user of the
aggregator's small block in one sequence.

Nothing new is computed here, so nothing new is the reference: every answer is compared with the reference of the
query's own test file (test_broker_stats.Expected, partition_load_support.Restatement, proposal_diff_support
.restated_diff over the oracle, sorted_replicas_support.SortedModel, execution_plan_support.build_plan,
metric_aggregator_support and metric_anomaly_support), byte for byte as there. One props(20) session serves the session
queries; the actions between the calls go to the product, the oracle and the restatements alike.
"""
import random
import re

import numpy as np
import pytest

import ccmi
import metric_aggregator_support as S
from acceptance_support import MOVE, REPO, props
from execution_plan_support import LARGE, build_plan, from_ccmi, in_collection_order, raw_call, summary_dict
from execution_plan_support import check as check_plan
from partition_load_support import DEFAULT, DISK, NW_OUT, Restatement
from partition_load_support import assert_same as assert_same_load
from proposal_diff_support import OracleState, restated_diff
from proposal_diff_support import check as check_diff
from sorted_replicas_support import SortedModel
from sorted_replicas_support import check as check_sorted
from test_broker_stats import Case
from test_metric_aggregator import Pair as AggregatorPair
from test_metric_anomaly import M as ANOMALY_METRICS
from test_metric_anomaly import build as build_anomaly_pair
from test_metric_anomaly import check_percentile

pytestmark = pytest.mark.gpu

with open(REPO + "/cruise-control_amd/csrc/engine/devtypes.h") as _f:
    AGG_TILE = int(re.search(r"constexpr int kAggTile = (\d+);", _f.read()).group(1))


class Session:
    """The props(20) session with every query's reference kept in step with it."""

    def __init__(self, lib):
        self.c = Case.random(lib, **props(20))
        self.cm, self.oc, self.desc = self.c.cm, self.c.oc, self.c.desc
        self.init = OracleState(self.oc)
        self.loads = Restatement(self.desc)
        self.sorted = SortedModel(self.desc)
        self.rng = random.Random(20261021)
        d = self.desc
        self.P, self.B = d.num_partitions, d.num_brokers
        self.off = list(d.partition_offset[:self.P + 1])
        self.moved = set()

    def move(self, k=1):
        """k replica moves of partitions not moved before, applied to the product and to every reference."""
        dist = self.oc.replica_distribution()
        actions = []
        for p in self.rng.sample(range(self.P), self.P):
            if p in self.moved:
                continue
            here = dist[self.off[p]:self.off[p + 1]]
            dst = self.rng.choice([b for b in range(self.B) if b not in here])
            actions.append((MOVE, p, here[0], dst, -1, -1, -1))
            self.moved.add(p)
            if len(actions) == k:
                break
        assert self.cm.apply(actions) == k
        self.oc.apply(actions)
        assert self.cm.actions() == self.oc.actions()
        self.loads.apply(actions)
        self.sorted.apply(actions)

    def proposals(self):
        return restated_diff(self.desc, self.init, self.oc)

    # one checked call of each query
    def broker_stats(self):
        self.c.expected().check(self.cm.broker_stats())

    def partition_load(self, entries, res=DISK):
        want, n = self.loads.expected(res, DEFAULT, entries=entries)
        got = self.cm.partition_load(ccmi.RESOURCES[res], entries=entries)
        assert_same_load(got, want, n)
        return got

    def proposal_diff(self):
        return check_diff(self.cm, self.proposals())

    def sorted_replicas(self, brokers=None, **spec):
        return check_sorted(self.cm, self.sorted, brokers, **spec)

    def execution_plan(self, rank=None):
        return check_plan(self.cm, [from_ccmi(p) for p in self.proposals()], [LARGE], rank)


@pytest.fixture(scope="module")
def session(gpu_lib, oracle_lib):
    return Session(gpu_lib)


# ------------------------------------------------------------------------------------------------ regrowth
def test_partition_load_entries_regrow(session):
    s = session
    assert len(s.partition_load(3).records) == 3  # an odd record count
    assert len(s.partition_load(2 ** 31 - 1).records) == s.P > 3  # the output block regrows
    assert len(s.partition_load(5).records) == 5
    assert len(s.partition_load(s.P - 1, NW_OUT).records) == s.P - 1


def test_proposal_diff_capacity_regrow(session):
    s = session
    s.move(41)
    want = s.proposals()
    assert len(want) >= 41 and len(want) % 2 == 1  # an odd record count
    whole = None
    for capacity in (1, None, 3, len(want) - 1):  # small, every record (the output block regrows), small again
        if capacity is None:
            whole = s.proposal_diff().records
            assert len(whole) == len(want)
        else:
            cut = s.cm.proposal_diff(capacity=capacity)
            assert cut.num_proposals == len(want) and len(cut.records) == capacity
            if whole is not None:
                assert cut.records.tobytes() == whole[:capacity].tobytes()
    first = s.cm.proposal_diff(capacity=1).records
    assert first.tobytes() == whole[:1].tobytes()


def test_sorted_replicas_totals_regrow(session):
    s = session
    lengths = [len(rows) for rows, _ in s.sorted.expected(None, leaders=True)]
    odd = next(b for b in range(s.B) if lengths[b] % 2 == 1)  # an odd record count: the gather's last pair is half
    small = s.sorted_replicas([odd], leaders=True, score="DISK")
    assert len(small[0]) == lengths[odd] and lengths[odd] % 2 == 1
    everything = s.sorted_replicas(None, score="NW_IN", reverse=True)  # every replica: the output block regrows
    assert sum(len(x) for x in everything) == s.desc.num_replicas > lengths[odd]
    again = s.sorted_replicas([odd], leaders=True, score="DISK")
    assert again[0].tobytes() == small[0].tobytes()
    two = s.sorted_replicas([odd, (odd + 1) % s.B], followers=True)
    assert sum(len(x) for x in two) > 0


def test_execution_plan_capacities_regrow(session):
    s = session
    B = s.B

    def reference():
        return build_plan(in_collection_order([from_ccmi(p) for p in s.proposals()]), B, [LARGE])

    def need(ref):
        x = ref.summary
        return (x["num_inter_tasks"], x["num_inter_entries"], x["num_intra_tasks"], x["num_leader_tasks"])

    s.move(3)
    for _ in range(8):  # on the reference, beforehand: an odd task count and an int32 list that is no whole quads
        small = need(reference())
        if small[0] % 2 == 1 and small[1] % 4 != 0:
            break
        s.move(1)
    assert small[0] % 2 == 1 and small[1] % 4 != 0 and small[2] == 0
    plan, _ = s.execution_plan()
    assert (len(plan.tasks), plan.summary.num_inter_entries) == small[:2]
    s.move(60)  # every list longer: the entry buffers and each output list regrow
    ref = reference()
    large = need(ref)
    assert all(a > b for a, b in zip(large[:2], small[:2]))
    st, summary, bufs = raw_call(s.cm, [LARGE])  # no room: the sizing call writes the offsets and the summary only
    assert st == 0 and summary_dict(summary) == ref.summary
    assert set(bufs["inter"]) == set(bufs["order"]) == set(bufs["leaders"]) == {-7}
    rank = np.random.default_rng(3).permutation(s.P).astype(np.int32)
    plan, _ = s.execution_plan(rank)
    assert len(plan.tasks) == large[0]
    caps = list(large)
    caps[1] -= 1  # one list one entry short after the regrowth: nothing but the offsets and the summary again
    st, summary, bufs = raw_call(s.cm, [LARGE], caps, rooms=large)
    assert st == 0 and summary_dict(summary) == ref.summary
    assert set(bufs["inter"]) == set(bufs["order"]) == set(bufs["leaders"]) == {-7}
    s.execution_plan()


# ------------------------------------------------------------------------------------------------ neighbours
def test_queries_interleaved_with_changes(session):
    """A B C D E A B C D E with a ccmi_session_apply before every call: a piece that overran into a neighbour's piece
    or static table would change a later answer. The second round holds the reference as the first did."""
    s = session
    for round_ in range(2):
        s.move(2)
        s.broker_stats()
        s.move(1)
        s.partition_load(2 ** 31 - 1, NW_OUT)
        s.move(2)
        diff = s.proposal_diff()
        s.move(1)
        s.sorted_replicas(None, score="CPU", priorities=("immigrants",))
        s.move(2)
        plan, _ = s.execution_plan(np.random.default_rng(round_).permutation(s.P).astype(np.int32))
        assert plan.summary.num_inter_tasks > len(diff.records) > 0  # two more partitions moved since the diff


# ------------------------------------------------------------------------------------------------ the aggregator
class _Both(AggregatorPair):
    """test_metric_anomaly's pair with test_metric_aggregator's checked calls on it."""

    def __init__(self, pair):
        self.dev, self.ref = pair.dev, pair.ref
        self.E, self.G, self.M = self.dev.E, self.dev.G, self.dev.M
        self.window_ms = S.WINDOW_MS


def test_every_user_of_the_aggregators_small_block(gpu_lib):
    """One more entity than a tile of the cover pass, so two tile offsets and their total. The walk's mask, the state
    sums, the tile offsets and the window list are pieces of one block: this order crosses all of them."""
    E = AGG_TILE + 1
    rng = random.Random(5)
    pair, _ = build_anomaly_pair(gpu_lib, rng, E, 10)
    p = _Both(pair)
    mask = np.array([1 if rng.random() < 0.6 else 0 for _ in range(E)], dtype=np.uint8)
    mask[[0, AGG_TILE - 1, AGG_TILE]] = 1  # both sides of the tile boundary
    options = S.AggregationOptions(0.0, 0.0, 1, 5, S.ENTITY, True)
    for _ in range(2):
        want = p.completeness(-1, S.LONG_MAX, options, mask)
        assert len(want.valid_window_indices) == 10
        p.check_state()
        rows = p.aggregate(-1, S.LONG_MAX, options, mask)
        assert len(rows.entities) == int(mask.sum()) > AGG_TILE // 2
        ents, _ = p.peek()
        assert len(ents) > AGG_TILE // 2
        check_percentile(pair, 90.0, 10.0, 0.5, 0.2, range(ANOMALY_METRICS), interested=mask)
