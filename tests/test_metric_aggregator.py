"""ccmi_aggregator: MetricSampleAggregator on the device (kernels/aggregator.hip) against the plain-Python restatement of
the reference's classes (tests/metric_aggregator_support.py). Every output is compared: floats as bit patterns, integers
and masks exactly. There is no tolerance.
"""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import ccmi
import metric_aggregator_support as S

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "cruise-control_amd", "csrc", "engine", "devtypes.h")) as _f:
    _DEVTYPES = _f.read()
BLOCK = int(re.search(r"constexpr int kAggBlock = (\d+);", _DEVTYPES).group(1))
MAX_BLOCKS = int(re.search(r"constexpr int kAggMaxBlocks = (\d+);", _DEVTYPES).group(1))
TILE = int(re.search(r"constexpr int kAggTile = (\d+);", _DEVTYPES).group(1))
KAT = json.load(open(os.path.join(REPO, "tests", "golden", "metric_aggregator_kat.json")))["aggregator"]
SENTINEL = 0xAB
ALL_TIME = (-1, S.LONG_MAX)
SEEDS = {3: 11, 9: 12}  # by M; picked on the CPU so that the coverage asserted in test_random_scripts holds


class Pair:
    """One device aggregator and the restatement, fed the same calls."""

    def __init__(self, lib, num_windows, window_ms, min_samples, fns, group, num_groups=None):
        self.dev = ccmi.MetricSampleAggregator(num_windows, window_ms, min_samples, fns, group, num_groups, lib=lib)
        self.ref = S.MetricSampleAggregator(num_windows, window_ms, min_samples, fns, group)
        self.E, self.G, self.M = self.dev.E, self.dev.G, self.dev.M
        self.window_ms = window_ms

    def add(self, entities, times, values):
        got = self.dev.add_samples(entities, times, values)
        want = self.ref.add_samples(entities, times, values)
        assert got.tolist() == [1 if a else 0 for a in want]
        self.check_state()

    def remove(self, ids):
        self.dev.remove_entities(ids)
        self.ref.remove_entities(ids)
        self.check_state()

    def clear(self):
        self.dev.clear()
        self.ref.clear()
        self.check_state()

    def check_state(self):
        s, r = self.dev.state(), self.ref
        assert (s.generation, s.oldest_window_index, s.current_window_index, s.num_samples, s.num_present_entities,
                s.num_available_windows) == (r.generation, r.oldest, r.current, r.num_samples(), len(r.raw),
                                             r.num_available_windows())

    def check_completeness(self, got, want):
        assert got.generation == want.generation
        assert got.windows.tolist() == want.windows
        assert got.included.tolist() == [1 if i else 0 for i in want.included]
        assert got.valid_window_indices.tolist() == want.valid_window_indices
        for g, w in ((got.valid_entity_ratio_by_window, want.valid_entity_ratio_by_window),
                     (got.valid_entity_ratio_with_group_granularity_by_window,
                      want.valid_entity_ratio_with_group_granularity_by_window),
                     (got.valid_entity_group_ratio_by_window, want.valid_entity_group_ratio_by_window),
                     (got.extrapolated_entity_ratio_by_window, want.extrapolated_entities_by_window)):
            assert S.float_bits(g).tolist() == S.float_bits(w).tolist()
        if want.windows:  # the range was not empty: the totals are those of the interpreted options
            assert (got.num_interested_entities, got.num_interested_groups) == (want.num_interested_entities,
                                                                                want.num_interested_groups)
        assert (got.num_valid_entities, got.num_valid_groups) == (len(want.valid_entities),
                                                                  len(want.valid_entity_groups))
        assert S.float_bits([got.valid_entity_ratio, got.valid_entity_group_ratio]).tolist() == \
            S.float_bits([want.valid_entity_ratio, want.valid_entity_group_ratio]).tolist()

    def completeness(self, frm, to, options, interested=None):
        o = ccmi.AggregationOptions(options.min_valid_entity_ratio, options.min_valid_entity_group_ratio,
                                    options.min_valid_windows, options.max_allowed_extrapolations_per_entity,
                                    options.granularity, options.include_invalid_entities)
        got = self.dev.completeness(frm, to, o, interested)
        ids = None if interested is None else [e for e, f in enumerate(interested) if f]
        want = self.ref.completeness(frm, to, options, ids)
        self.check_completeness(got, want)
        assert got.failure == S.FAIL_NONE
        assert np.flatnonzero(got.valid_entities).tolist() == sorted(want.valid_entities)
        assert np.flatnonzero(got.valid_groups).tolist() == sorted(want.valid_entity_groups)
        return want

    def aggregate(self, frm, to, options, interested=None, capacity=None, want=None):
        """-> the restatement's result (`want` when the caller has it already), None for NotEnoughValidWindows, or the
        IllegalStateException it raised."""
        o = ccmi.AggregationOptions(options.min_valid_entity_ratio, options.min_valid_entity_group_ratio,
                                    options.min_valid_windows, options.max_allowed_extrapolations_per_entity,
                                    options.granularity, options.include_invalid_entities)
        ids = None if interested is None else [e for e, f in enumerate(interested) if f]
        try:
            want = want or self.ref.aggregate(frm, to, options, ids)
        except S.NotEnoughValidWindowsException as e:
            got = self.dev.aggregate(frm, to, o, interested, capacity)
            assert got.completeness.failure == e.failure and got.num_entities == 0 and len(got.entities) == 0
            return None
        except S.IllegalStateException as e:
            with pytest.raises(ccmi.IllegalStateException) as info:
                self.dev.aggregate(frm, to, o, interested, capacity)
            assert str(info.value).startswith(str(e))
            return e
        got = self.dev.aggregate(frm, to, o, interested, capacity)
        assert got.completeness.failure == S.FAIL_NONE
        self.check_completeness(got.completeness, want.completeness)
        k = len(want.entities) if capacity is None else min(capacity, len(want.entities))
        assert got.num_entities == len(want.entities)
        assert got.entities.tolist() == want.entities[:k].tolist()
        assert got.values.shape == want.values[:k].shape
        assert np.array_equal(S.float_bits(got.values), S.float_bits(want.values[:k]))
        assert np.array_equal(got.extrapolations, want.extrapolations[:k])
        assert got.invalid.tolist() == want.invalid[:k].tolist()
        return want

    def peek(self):
        ents, values, ext, n = self.dev.peek_current_window()
        w_ents, w_values, w_ext = self.ref.peek_current_window()
        assert n == len(w_ents) and ents.tolist() == w_ents.tolist() and ext.tolist() == w_ext.tolist()
        assert np.array_equal(S.float_bits(values), S.float_bits(w_values))
        return w_ents, w_ext


def options_of(o):
    return S.AggregationOptions(o["min_valid_entity_ratio"], o["min_valid_entity_group_ratio"], o["min_valid_windows"],
                                o["max_allowed_extrapolations"], o["granularity"], o["include_invalid"])


def mask_of(ids, num_entities):
    if ids is None:
        return None
    m = np.zeros(num_entities, dtype=np.uint8)
    m[list(ids)] = 1
    return m


# ---------------------------------------------------------------------------------------------- 1. the KAT scripts
@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_kat_scripts(gpu_lib, case):
    p = Pair(gpu_lib, KAT["num_windows"], KAT["window_ms"], KAT["min_samples"], KAT["functions"], KAT["entity_group"])
    for step in case["steps"]:
        (kind, body), = step.items()
        if kind == "add":  # one batch per populateSampleAggregator call
            p.add([s[0] for s in body], [s[1] for s in body], [s[2:] for s in body])
        elif kind == "remove":
            p.remove(body)
        elif kind == "state":
            p.check_state()
            if "generation" in body:
                assert p.dev.generation == body["generation"]
            if "num_available_windows" in body:
                assert p.dev.num_available_windows == body["num_available_windows"]
        elif kind == "completeness":
            want = p.completeness(body["from"], body["to"], options_of(body["options"]),
                                  mask_of(body["interested"], p.E))
            assert len(want.valid_window_indices) == body["num_valid_windows"]
        elif kind == "aggregate":
            want = p.aggregate(body["from"], body["to"], options_of(body["options"]), mask_of(body["interested"], p.E))
            assert len(want.entities) == body["num_entities"]
        elif kind == "peek":
            ents, ext = p.peek()
            assert {str(e): int(x) for e, x in zip(ents, ext)} == body["extrapolations"]
    p.peek()


# ---------------------------------------------------------------------------------------------- 2. seeded scripts
def script_features(group, steps, num_windows=5):
    """What a script contains, found on the restatement alone."""
    ref = S.MetricSampleAggregator(num_windows, S.WINDOW_MS, 4, [S.AVG], group)
    f = dict(twice=False, old=False, dropped=False, two_rollouts=False, leap=False, removed_then_sampled=False)
    removed = set()
    for step in steps:
        if step[0] == "add":
            ents, times = step[1], step[2]
            f["twice"] |= len(set(ents)) < len(ents)
            rollouts = 0
            for e, t in zip(ents, times):
                before = ref.current
                accepted = ref.add_sample(e, t, [0.0])
                f["dropped"] |= not accepted
                f["old"] |= accepted and ref.window_index(t) < ref.current
                if ref.current != before:
                    rollouts += 1
                    f["leap"] |= before > 0 and ref.current - before > 6
                f["removed_then_sampled"] |= accepted and e in removed
            f["two_rollouts"] |= rollouts >= 2
        elif step[0] == "remove":
            removed |= set(step[1])
    f["wraps_twice"] = ref.current > 12
    f["never_sampled"] = S.NEVER_SAMPLED not in ref.raw
    return f


@pytest.mark.parametrize("num_metrics", [3, 9])
def test_random_scripts(gpu_lib, num_metrics):
    group, steps = S.random_script(SEEDS[num_metrics], num_metrics)
    assert len(group) == 300 and sorted(np.bincount(group).tolist()) == sorted(S.GROUP_SIZES)
    assert 35 <= sum(1 for s in steps if s[0] == "add") <= 50 and all(len(s[1]) <= 500 for s in steps if s[0] == "add")
    assert all(script_features(group, steps).values()), script_features(group, steps)
    fns = [(S.AVG, S.MAX, S.LATEST)[m % 3] for m in range(num_metrics)]
    p = Pair(gpu_lib, 5, S.WINDOW_MS, 4, fns, group)
    rng = random.Random(num_metrics)
    codes, excluded, included, group_by_one = set(), False, False, False
    for step in steps:
        if step[0] == "add":
            p.add(step[1], step[2], step[3])
        elif step[0] == "remove":
            p.remove(step[1])
        else:
            p.peek()
            for options, interested in S.query_matrix(p.E, rng):
                c = p.completeness(*ALL_TIME, options, interested)
                excluded |= any(not i for i in c.included)
                included |= any(c.included)
                r = p.aggregate(*ALL_TIME, options, interested)
                if isinstance(r, S.AggregationResult):
                    codes |= set(np.unique(r.extrapolations).tolist())
            # a narrower range, clamped at both ends
            p.aggregate((p.ref.current - 3) * S.WINDOW_MS, (p.ref.current - 2) * S.WINDOW_MS,
                        S.AggregationOptions(0.0, 0.0, 1, 5, S.ENTITY, True))
            for w in range(p.ref.oldest, p.ref.current):
                for g in range(p.G):
                    members = [e for e in range(p.E) if group[e] == g]
                    bad = [e for e in members if e not in p.ref.raw or not p.ref.raw[e].is_valid_at_window_index(w)]
                    group_by_one |= len(members) > 1 and len(bad) == 1
    # asserted on the restatement alone: the scripts reach what the comparison is there for
    assert codes == {0, 1, 2, 3, 4}
    assert excluded and included and group_by_one


# ---------------------------------------------------------------------------------------------- 3. edges
def small_script(rng, num_entities, num_metrics, windows=(1, 2, 3, 4, 5, 6, 7, 8)):
    batches = []
    for w in windows:
        ents, times, vals = [], [], []
        for e in range(num_entities):
            # the two windows before the last get a sample from everyone, so that a single group can be valid there
            for _ in range(rng.choice([1, 2, 4, 5] if w in windows[-3:-1] else [0, 1, 2, 4, 4, 4, 5])):
                ents.append(e)
                times.append((w - 1) * S.WINDOW_MS + rng.randrange(S.WINDOW_MS))
                vals.append([rng.uniform(0, 100) for _ in range(num_metrics)])
        order = list(range(len(ents)))
        rng.shuffle(order)
        batches.append(([ents[i] for i in order], [times[i] for i in order], [vals[i] for i in order]))
    return batches


def raw_aggregate(p, options, capacity, windows_bound):
    """ccmi_aggregator_aggregate on sentinel-filled arrays one row longer than `capacity`."""
    rows = capacity + 1
    ent = np.full(rows, -0x54545455, dtype=np.int32)
    val = np.full(rows * p.M * windows_bound, np.float32(-7.25), dtype=np.float32)
    ext = np.full(rows * windows_bound, SENTINEL, dtype=np.uint8)
    inv = np.full(rows, SENTINEL, dtype=np.uint8)
    s, arrays = p.dev._completeness_struct(np)
    n = C.c_int64(-1)
    o = options.struct()
    p.dev.lib.check(p.dev.lib.lib.ccmi_aggregator_aggregate(p.dev.handle, -1, S.LONG_MAX, C.byref(o), None, C.byref(s),
                                                            ent.ctypes.data, val.ctypes.data, ext.ctypes.data,
                                                            inv.ctypes.data, capacity, C.byref(n)))
    return s, n.value, ent, val, ext, inv


@pytest.mark.parametrize("num_entities", [1, 63, 64, 65])
@pytest.mark.parametrize("one_group", [True, False], ids=["G1", "GE"])
def test_edge_shapes(gpu_lib, num_entities, one_group):
    rng = random.Random(num_entities * 2 + one_group)
    group = [0] * num_entities if one_group else list(range(num_entities))
    rng.shuffle(group)
    p = Pair(gpu_lib, 5, S.WINDOW_MS, 4, [S.AVG, S.MAX, S.LATEST], group)
    lenient = S.AggregationOptions(0.0, 0.0, 1, 5, S.ENTITY, True)
    # no sample at all
    p.check_state()
    p.completeness(*ALL_TIME, lenient)
    assert p.aggregate(*ALL_TIME, lenient) is None
    p.peek()
    for ents, times, vals in small_script(rng, num_entities, 3):
        p.add(ents, times, vals)
    nothing = np.zeros(num_entities, dtype=np.uint8)
    for options in (lenient, S.AggregationOptions(0.0, 0.0, 1, 1, S.ENTITY_GROUP, False),
                    S.AggregationOptions(0.4, 0.4, 2, 0, S.ENTITY, False)):
        for interested in (None, nothing):  # a mask selecting nothing is the empty set: every present entity
            p.completeness(*ALL_TIME, options, interested)
            p.aggregate(*ALL_TIME, options, interested)
    want = p.aggregate(*ALL_TIME, lenient)
    total, wv = len(want.entities), len(want.completeness.valid_window_indices)
    assert total >= 1 and wv >= 1
    o = ccmi.AggregationOptions(0.0, 0.0, 1, 5, S.ENTITY, True)
    for capacity in sorted({0, 1, total}):
        p.aggregate(*ALL_TIME, lenient, capacity=capacity)
        s, n, ent, val, ext, inv = raw_aggregate(p, o, capacity, wv)
        k = min(capacity, total)
        assert n == total and s.num_valid_windows == wv
        assert ent[:k].tolist() == want.entities[:k].tolist()
        assert np.array_equal(S.float_bits(val[:k * p.M * wv]), S.float_bits(want.values[:k].reshape(-1)))
        # rows beyond the count stay untouched
        assert (ent[k:] == -0x54545455).all() and (inv[k:] == SENTINEL).all() and (ext[k * wv:] == SENTINEL).all()
        assert (val[k * p.M * wv:] == np.float32(-7.25)).all()
    p.peek()
    p.clear()
    p.completeness(*ALL_TIME, lenient)
    assert p.aggregate(*ALL_TIME, lenient) is None


# ---------------------------------------------------------------------------------------------- 4. the larger case
def test_every_tile_and_grid_boundary(gpu_lib):
    """E = 70,000 in 2,000 groups, three batches of E samples: more entities than one grid-stride pass has lanes
    (kAggMaxBlocks * kAggBlock) plus a compaction tile, and no multiple of the tile or of the block."""
    num_entities, num_groups = 70000, 2000
    assert num_entities > MAX_BLOCKS * BLOCK + TILE and num_entities % TILE and num_entities % BLOCK
    assert num_entities // TILE + 1 > 64
    rng = np.random.default_rng(7)
    group = rng.integers(0, num_groups, num_entities).tolist()
    p = Pair(gpu_lib, 3, S.WINDOW_MS, 1, [S.AVG, S.MAX, S.LATEST], group, num_groups)
    for w in (1, 2, 3):
        ents = rng.permutation(num_entities)
        again = rng.random(num_entities) < 0.1
        ents[again] = rng.integers(0, num_entities, int(again.sum()))  # gaps, and entities twice or more
        times = (w - 1) * S.WINDOW_MS + rng.integers(0, S.WINDOW_MS, num_entities)
        times[:50] += S.WINDOW_MS  # a roll-out at the head of the batch, the rest lands in the window before
        vals = rng.uniform(0.0, 1e6, (num_entities, 3))
        p.add(ents.tolist(), times.tolist(), vals.tolist())
    mask = (rng.random(num_entities) < 0.5).astype(np.uint8)
    everything = S.AggregationOptions(0.0, 0.0, 1, 3, S.ENTITY, True)
    want = p.aggregate(*ALL_TIME, everything)
    assert isinstance(want, S.AggregationResult) and len(want.entities) > MAX_BLOCKS * BLOCK + TILE
    p.aggregate(*ALL_TIME, everything, capacity=TILE + 1, want=want)
    by_group = S.AggregationOptions(0.5, 0.2, 1, 1, S.ENTITY_GROUP, False)
    p.completeness(*ALL_TIME, by_group, mask)
    want = p.aggregate(*ALL_TIME, by_group, mask)
    assert isinstance(want, S.AggregationResult) and len(want.entities) > TILE
    p.peek()


# ---------------------------------------------------------------------------------------------- 5. errors, two at once
def test_failures_and_errors(gpu_lib):
    group = [0, 0, 1, 1]
    p = Pair(gpu_lib, 3, S.WINDOW_MS, 2, [S.AVG], group)
    q = Pair(gpu_lib, 5, 500, 1, [S.MAX, S.LATEST], [0, 1, 2])  # a second aggregator alive on the same device
    lenient = S.AggregationOptions(0.0, 0.0, 1, 5, S.ENTITY, True)
    assert p.aggregate(*ALL_TIME, lenient) is None  # no window in range
    p.add([0, 0, 1], [10, 20, 30], [[1.0], [2.0], [3.0]])
    q.add([2, 1], [100, 700], [[1.0, 2.0], [3.0, 4.0]])
    p.add([0, 0, 1, 2], [1010, 1020, 1030, 2040], [[1.0], [2.0], [3.0], [4.0]])
    q.add([0], [1300], [[5.0, 6.0]])
    got = p.dev.aggregate(*ALL_TIME, ccmi.AggregationOptions(0.0, 0.0, 3, 5))
    assert got.completeness.failure == ccmi.AGG_FAILURE_NOT_ENOUGH_VALID_WINDOWS == S.FAIL_NOT_ENOUGH_VALID_WINDOWS
    assert p.aggregate(*ALL_TIME, S.AggregationOptions(0.0, 0.0, 3, 5, S.ENTITY, True)) is None
    got = p.dev.aggregate(5000, 9000, ccmi.AggregationOptions())
    assert got.completeness.failure == ccmi.AGG_FAILURE_NO_WINDOW_IN_RANGE and got.num_entities == 0
    # The two coverage IllegalStateExceptions of validateCompleteness cannot be reached through aggregate: a window is
    # included only if the merged ratios meet the two minima, the final ratios are those of the last included window's
    # merge (the same float compared with the same double), and without an included window NotEnoughValidWindows comes
    # first. Thresholds no window meets therefore end in the failure field, on both sides:
    everyone = np.ones(4, dtype=np.uint8)
    for ratios in ((0.2, 0.9), (0.9, 0.0)):
        assert p.aggregate(*ALL_TIME, S.AggregationOptions(*ratios, 1, 5, S.ENTITY, True), everyone) is None
    assert isinstance(p.aggregate(*ALL_TIME, S.AggregationOptions(0.5, 0.5, 1, 5, S.ENTITY, True), everyone),
                      S.AggregationResult)
    q.completeness(*ALL_TIME, lenient)
    q.aggregate(*ALL_TIME, lenient)
    q.peek()
    p.peek()
    # CCMI_E_INVALID
    for kwargs in (dict(num_windows=0), dict(num_windows=32), dict(group=[0, 2]), dict(group=[-1, 0]),
                   dict(min_samples=0), dict(min_samples=128), dict(fns=[3])):
        a = dict(num_windows=3, min_samples=2, fns=[S.AVG], group=[0, 1])
        a.update(kwargs)
        with pytest.raises(ccmi.IllegalArgumentException):
            ccmi.MetricSampleAggregator(a["num_windows"], 1000, a["min_samples"], a["fns"], a["group"], 2, lib=gpu_lib)
    before = p.dev.state()
    for ents, times in (([4], [10]), ([-1], [10]), ([0], [-5])):
        with pytest.raises(ccmi.IllegalArgumentException):
            p.dev.add_samples(ents, times, [[1.0]])
    with pytest.raises(ccmi.IllegalArgumentException):
        gpu_lib.check(gpu_lib.lib.ccmi_aggregator_add_samples(p.dev.handle, None, None, None, -1, None, None))
    with pytest.raises(ccmi.IllegalArgumentException):
        p.dev.completeness(*ALL_TIME, ccmi.AggregationOptions(min_valid_windows=0))
    with pytest.raises(ccmi.IllegalArgumentException):
        p.dev.aggregate(*ALL_TIME, ccmi.AggregationOptions(min_valid_windows=0))
    with pytest.raises(ccmi.IllegalArgumentException):
        p.dev.remove_entities([4])
    after = p.dev.state()
    assert (before.generation, before.num_samples) == (after.generation, after.num_samples)
    p.check_state()
    q.check_state()


# ---------------------------------------------------------------------------------------------- 6. the builder helper
def test_aggregate_feeds_the_builder(gpu_lib):
    """An aggregate over KafkaMetricDef's common metrics, fed to ccmi_builder_populate_partition through the helper,
    gives the loads that feeding the restatement's rows gives."""
    rng = random.Random(5)
    fns = [f for _, f in ccmi.KAFKA_COMMON_METRICS]
    num_partitions, topics = 24, 4
    group = [i % topics for i in range(num_partitions)]
    p = Pair(gpu_lib, 3, S.WINDOW_MS, 2, fns, group)
    for ents, times, vals in small_script(rng, num_partitions, len(fns), windows=(1, 2, 3, 4, 5)):
        vals = [[v[0] / 100.0] + v[1:] for v in vals]  # CPU_USAGE is a unit interval
        p.add(ents, times, vals)
    options = S.AggregationOptions(0.0, 0.0, 1, 5, S.ENTITY, True)
    want = p.aggregate(*ALL_TIME, options)
    got = p.dev.aggregate(*ALL_TIME, ccmi.AggregationOptions(0.0, 0.0, 1, 5, ccmi.GRANULARITY_ENTITY, True))
    wv = got.values.shape[2]
    assert wv == 3 and got.num_entities == num_partitions
    pick = [[n for n, _ in ccmi.KAFKA_COMMON_METRICS].index(m) for m in ccmi.LoadMonitorModel.METRICS]
    assert pick == [0, 1, 2, 3, 7, 8]

    def model(rows_from_helper):
        m = ccmi.LoadMonitorModel(num_windows=wv, lib=gpu_lib)
        for b in range(4):
            m.create_broker("r%d" % (b % 2), "h%d" % b, b, {"CPU": 100.0, "NW_IN": 1e6, "NW_OUT": 1e6, "DISK": 1e7})
        for row in range(num_partitions):
            e = int(want.entities[row])
            replicas = [e % 4, (e + 1) % 4]
            if rows_from_helper:
                got.populate_partition(m, row, "T%d" % group[e], e, replicas, replicas[0])
            else:
                m.populate_partition("T%d" % group[e], e, replicas, replicas[0],
                                     {name: want.values[row][pick[i]].tolist()
                                      for i, name in enumerate(ccmi.LoadMonitorModel.METRICS)})
        return m

    a, b = model(True), model(False)
    la, lb = np.array(a.replica_loads(), dtype=np.float32), np.array(b.replica_loads(), dtype=np.float32)
    assert la.shape == (2 * num_partitions, 6, wv) and la.any()
    assert np.array_equal(S.float_bits(la), S.float_bits(lb))
    assert np.array_equal(got.leader_metrics(0), want.values[0][pick].reshape(-1))
