"""The restatement of the metric sample aggregator (tests/metric_aggregator_support.py) against the values the
reference's own unit tests assert, recorded in tests/golden/metric_aggregator_kat.json: MetricSampleAggregatorTest and
RawMetricValuesTest. CPU only."""
import json
import os

import numpy as np
import pytest

import metric_aggregator_support as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(REPO, "tests", "golden", "metric_aggregator_kat.json")))
AGG, RAW = KAT["aggregator"], KAT["raw"]


def options_of(o):
    return S.AggregationOptions(o["min_valid_entity_ratio"], o["min_valid_entity_group_ratio"], o["min_valid_windows"],
                                o["max_allowed_extrapolations"], o["granularity"], o["include_invalid"])


def check_state(agg, exp):
    if "generation" in exp:
        assert agg.generation == exp["generation"]
    if "earliest_window" in exp:
        assert agg.earliest_window() == exp["earliest_window"]
    if "all_windows" in exp:
        assert agg.all_windows() == exp["all_windows"]
    if "available_windows" in exp:
        assert agg.available_windows() == exp["available_windows"]
    if "num_all_windows" in exp:
        assert len(agg.all_windows()) == exp["num_all_windows"]
    if "num_available_windows" in exp:
        assert agg.num_available_windows() == exp["num_available_windows"]


def check_completeness(c, q):
    eps = q["epsilon"]
    assert len(c.valid_window_indices) == q["num_valid_windows"]
    for w in q.get("excluded_windows", []):
        assert w not in c.valid_window_indices
    assert sorted(c.valid_entities) == q["valid_entities"]
    if "valid_groups" in q:
        assert sorted(c.valid_entity_groups) == q["valid_groups"]
    for g in q.get("valid_groups_contain", []):
        assert g in c.valid_entity_groups
    for w, (valid, gran, group, extrapolated) in q["by_window"].items():
        i = c.windows.index(int(w))
        assert abs(c.valid_entity_ratio_by_window[i] - valid) <= eps, w
        assert abs(c.valid_entity_ratio_with_group_granularity_by_window[i] - gran) <= eps, w
        assert abs(c.valid_entity_group_ratio_by_window[i] - group) <= eps, w
        assert abs(c.extrapolated_entities_by_window[i] - extrapolated) <= eps, w


@pytest.mark.parametrize("case", AGG["cases"], ids=[c["name"] for c in AGG["cases"]])
def test_aggregator_case(case):
    agg = S.MetricSampleAggregator(AGG["num_windows"], AGG["window_ms"], AGG["min_samples"], AGG["functions"],
                                   AGG["entity_group"])
    for step in case["steps"]:
        (kind, body), = step.items()
        if kind == "add":
            for e, t, *v in body:
                assert agg.add_sample(e, t, v)
        elif kind == "remove":
            agg.remove_entities(body)
        elif kind == "state":
            check_state(agg, body)
        elif kind == "completeness":
            check_completeness(agg.completeness(body["from"], body["to"], options_of(body["options"]),
                                                body["interested"]), body)
        elif kind == "aggregate":
            r = agg.aggregate(body["from"], body["to"], options_of(body["options"]), body["interested"])
            assert len(r.entities) == body["num_entities"]
            assert [w * AGG["window_ms"] for w in r.completeness.valid_window_indices] == body["windows_ms"]
            for m, expected in body["values_exact"].items():
                for k in range(len(r.entities)):
                    assert r.values[k, int(m)].tolist() == expected
        elif kind == "peek":
            ents, _, ext = agg.peek_current_window()
            assert {str(e): int(x) for e, x in zip(ents, ext)} == body["extrapolations"]
        else:
            raise AssertionError(kind)


@pytest.mark.parametrize("case", RAW["cases"], ids=[c["name"] for c in RAW["cases"]])
def test_raw_metric_values_case(case):
    raw = S.RawMetricValues(case["keep"], case["min_samples"], RAW["functions"])
    eps = RAW["epsilon"]
    for op in case["ops"]:
        name = op[0]
        if name == "oldest":
            raw.update_oldest_window_index(op[1])
        elif name == "add":
            raw.add_sample(op[2:], op[1])
        elif name == "add_refused":
            with pytest.raises(ValueError):
                raw.add_sample(op[2:], op[1])
        elif name == "reset":
            raw.reset_window_indices(op[1], op[2])
        elif name == "num_samples":
            assert raw.num_samples() == op[1]
        elif name == "valid":
            assert raw.is_valid_at_window_index(op[1]) == op[2]
        elif name == "extrapolated":
            assert raw.is_extrapolated_at_window_index(op[1]) == op[2]
        elif name == "is_valid":
            assert raw.is_valid(op[1]) == op[2]
        elif name == "agg":
            values, ext = raw.aggregate(op[1])
            exp = op[2]
            for m, by_index in exp["values"].items():
                for i, v in by_index.items():
                    assert abs(values[int(m)][int(i)] - v) <= eps, (m, i)
            if "extrapolations" in exp:
                got = {str(i): x for i, x in enumerate(ext) if x != S.NONE}
                assert got == exp["extrapolations"] and len(got) == exp["num_extrapolations"]
        else:
            raise AssertionError(name)


def test_float_arithmetic_is_javas():
    """The three places where the type of an expression shows: the (float) of a double sum, the float division of the
    AVG value, and the AVG_ADJACENT float total divided in double."""
    raw = S.RawMetricValues(6, 1, [S.AVG])
    raw.update_oldest_window_index(0)
    raw.add_sample([0.1], 0)
    raw.add_sample([0.2], 0)
    assert raw.values[0][0] == float(np.float32(float(np.float32(0.1)) + 0.2))
    assert raw.aggregate([0])[0][0][0] == float(np.float32(raw.values[0][0]) / np.float32(2))
    raw = S.RawMetricValues(6, 1, [S.AVG, S.MAX])
    raw.update_oldest_window_index(0)
    for w, v in ((0, 0.1), (2, 16777216.0)):
        raw.add_sample([v, v], w)
    values, ext = raw.aggregate([1])
    assert ext == [S.AVG_ADJACENT]
    total = np.float32(np.float32(0.1) + np.float32(0.0)) + np.float32(16777216.0)  # the float sum drops the 0.1
    assert float(total) == 16777216.0
    assert values[0][0] == float(np.float32(float(total) / 2)) and values[1][0] == float(np.float32(float(total) / 2))
    assert S.float_bits([np.nan, -np.nan]).tolist() == [0x7FC00000, 0x7FC00000]
