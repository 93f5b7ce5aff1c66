"""engine/broker_load.h compiled for the host (tests/cpp/test_broker_load.cpp) against the known answers of
tests/golden/metrics_processor_kat.json, which the restatement reproduces too (test_metrics_processor_reference.py).
CPU only; doubles are compared as bit patterns."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(REPO, "tests", "golden", "metrics_processor_kat.json")))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("broker_load") / "test_broker_load")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                    os.path.join(REPO, "cruise-control_amd", "csrc", "engine"),
                    os.path.join(REPO, "tests", "cpp", "test_broker_load.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out

    return run


def canonical(h):
    """hex bits of a double, every NaN the same"""
    v = int(h, 16)
    return "nan" if (v & 0x7FF0000000000000) == 0x7FF0000000000000 and v & 0xFFFFFFFFFFFFF else h


def test_holders(ask):
    got = ask(["avg %d %s" % (len(c["values"]), " ".join(c["values"])) for c in KAT["avg"]])
    assert got == [c["result"] for c in KAT["avg"]]
    got = ask(["latest %d %s" % (len(c["records"]), " ".join("%d %s" % (t, v) for t, v in c["records"]))
               for c in KAT["latest"]])
    assert got == [c["result"] for c in KAT["latest"]]


def test_convert_unit_and_metric_ids(ask):
    assert ask(["convert %d %s" % (c["type"], c["value"]) for c in KAT["convert"]]) == [c["result"] for c in KAT["convert"]]
    assert ask(["def %d" % c["type"] for c in KAT["def"]]) == [str(c["result"]) for c in KAT["def"]]


def test_cpu_estimate(ask):
    got = ask(["cpu %s %s" % (" ".join(c["weights"]), " ".join(c["args"])) for c in KAT["cpu"]])
    assert [g if g == "null" else canonical(g) for g in got] == \
           ["null" if c["result"] is None else canonical(c["result"]) for c in KAT["cpu"]]
    assert any(c["result"] is None for c in KAT["cpu"])


def test_version_logic_and_ratios(ask):
    got = ask(["version %d %d %s" % (c["follower_required"], c["enough"], c["avail"]) for c in KAT["version"]])
    assert got == ["%d %d %s" % (c["version"], c["min_required"], c["avail_after"]) for c in KAT["version"]]
    assert {c["version"] for c in KAT["version"]} == {-1, 4, 5}
    assert ask(["enough %d %d %d %d" % tuple(c["args"]) for c in KAT["enough"]]) == [str(c["result"]) for c in KAT["enough"]]


def test_hashes_and_list_bin_order(ask):
    got = ask(["tphash %d %d" % (c["topic_hash"], c["partition"]) for c in KAT["tphash"]])
    assert got == [str(c["result"]) for c in KAT["tphash"]]
    got = ask(["order %d %s" % (len(c["hashes"]), " ".join(map(str, c["hashes"]))) for c in KAT["order"]])
    for line, c in zip(got, KAT["order"]):
        words = [int(x) for x in line.split()]
        assert words[0] == c["flagged"], c["names"][:3]
        if not c["flagged"]:
            assert words[1:] == c["order"]
    assert {c["flagged"] for c in KAT["order"]} == {0, 1}
