"""What test_queue_probe.py (CPU emulation) and test_queue_probe_gpu.py (the HIP kernel) share: running one scenario of
tests/queue_probe_worker.py in a child process and checking its probes. A probe passes when the device's winner equals
the host loop's as (entry, replica, column) — exactly, there is no tolerance — and, where the keyed membership table was
audited, no broker's rows differ between the model, the mirror and the table."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "queue_probe_worker.py")
TILE = 256  # scan_server's kBlock: pairs per tile with one wave per candidate

SCENARIOS = ["columns_rd", "columns_lrd", "single", "multi", "batch2", "highbits", "changes", "excl_lead"]


def run_scenario(which, name, timeout=120, **env):
    """(probes, extras, seconds): the worker's {"name", "args", "rep"} records, its other JSON lines merged, wall time."""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, WORKER, which, name], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **env))
    seconds = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    probes, extras = [], {}
    for line in r.stdout.splitlines():
        if not line.startswith("{"):
            continue
        d = json.loads(line)
        if "rep" in d:
            probes.append(d)
        else:
            extras.update(d)
    assert extras.get("done") == len(probes) and probes, (extras, len(probes))
    return probes, extras, seconds


def check_probes(probes, which, keyed):
    """Every probe's triples agree; the path is the one the knobs select; audited tables are clean. Returns how many
    probes a scan-server queue command answered; `settle` probes are not counted (see expected_served)."""
    served = 0
    for d in probes:
        rep, what = d["rep"], json.dumps(d)
        assert rep["dev"] == rep["ref"], f"device {rep['dev']} != host loop {rep['ref']}: {what}"
        if keyed is not None:
            assert rep["keyed"] == int(keyed), what
        if rep["audited"]:
            assert rep["audit"] == 0, f"{rep['audit']} brokers' rows differ: {what}"
        if d["name"] == "settle":  # the scan after many applied moves is flattened (queue_probe_worker.Session.settle)
            if which == "gpu":
                assert rep["served"] == 0, what
            continue
        if which == "gpu" and rep["keyed"]:
            assert rep["served"] == 1, what
            assert rep["audited"] in (0, 3), what  # the device table was read back whenever the probe audited
        served += rep["served"]
    return served


def expected_served(probes):
    """Every probe but the `settle` ones, which are flattened by design."""
    return sum(1 for d in probes if d["name"] != "settle")


def reset_before(d):
    """Two or more accepted rows in the winner's entry, the lowest accepted slot a full tile or more before the
    winner's: the tile with the winner lowers the entry's least key and resets its best pair (least < before)."""
    r = d["rep"]
    return r["keyed"] and r["accepted_rows"] >= 2 and \
        (r["win_slot"] - r["lowest_accepted_slot"] - 1) * d["N"] + 1 >= TILE


def reset_after(d):
    """The other way round: the winner in the lowest accepted slot, another accepted row a full tile or more later."""
    r = d["rep"]
    return r["keyed"] and r["accepted_rows"] >= 2 and r["win_slot"] == r["lowest_accepted_slot"] and \
        (r["highest_accepted_slot"] - r["win_slot"] - 1) * d["N"] + 1 >= TILE


def by_name(probes):
    return {d["name"]: d for d in probes}


def check_coverage(name, probes, extras, which, keyed):
    """What a scenario has to reach, asserted from the probes' own reports (the lists were chosen for it)."""
    p = by_name(probes)
    if name == "columns_rd":
        assert {d["N"] for d in probes} >= {1, 2, 63, 64, 65, 255, 256, 257}
        assert {d["rep"]["win_len"] for d in probes if d["rep"]["ref"]} >= {1, 3, 4, 5}
        assert any(d["rep"]["ref"] and d["rep"]["ref"][2] == d["N"] - 1 and d["N"] == 257 for d in probes)
        assert any(d["rep"]["ref"] is None for d in probes)
        if keyed == "1":
            assert any(reset_before(d) for d in probes) and any(reset_after(d) for d in probes)
    elif name == "single":
        top = p["head_skip_highest"]["rep"]
        assert top["head_masked"] > 1 and top["ref"][0] >= 1  # every head row masked: the tail wins
        assert p["head_skip_lowest"]["rep"]["head_masked"] == 1 and p["head_skip_lowest"]["rep"]["ref"][0] == 0
        assert 1 < p["head_skip_middle"]["rep"]["head_masked"] < top["head_masked"]
        assert p["head_only_accept_masked"]["rep"]["ref"] is None or p["head_only_accept_masked"]["rep"]["ref"][0] >= 1
        assert p["head_only_accept_kept"]["rep"]["ref"][0] == 0
        assert p["head_len1_masked"]["rep"]["head_masked"] == 1 and p["head_len1_kept"]["rep"]["head_masked"] == 0
        assert p["len0_all"]["rep"]["ref"] is None and p["len1_all"]["rep"]["ref"] and p["len2_all"]["rep"]["ref"]
        assert p["winner_lowest_row"]["rep"]["win_rank"] == 0
        assert 0 < p["winner_higher_row"]["rep"]["win_rank"]
        highest = [d for d in probes if d["name"].startswith("winner_highest_row")]
        assert len(highest) >= 2
        for d in highest:  # a single entry, no head: the winner is the last row of a block of two or more rows
            r = d["rep"]
            assert d["n"] == 1 and d["args"]["head"] == -1 and r["win_len"] == d["rows"] >= 2, d
            assert r["ref"][0] == 0 and r["win_rank"] == r["win_len"] - 1 and r["accepted_rows"] == 1, d
    elif name == "multi":
        for N in (1, 3, 70):
            for n in (9, 16, 17, 40):
                assert p[f"N{N}_n{n}_first_of_wg"]["rep"]["ref"][0] == 3
                later = p[f"N{N}_n{n}_later_in_wg"]
                assert later["rep"]["ref"][0] == 8
                if n >= 17:  # entry 16 follows entry 8 on workgroup 0 and has rows: a tile holds rows of both
                    assert later["next_rows"] > 0, later
                assert p[f"N{N}_n{n}_last"]["rep"]["ref"][0] == n - 1
                assert p[f"N{N}_n{n}_other_wg_wins"]["rep"]["ref"][0] == 5
                assert p[f"N{N}_n{n}_none"]["rep"]["ref"] is None
        if which == "gpu":
            assert all(d["rep"]["n_active"] == 8 for d in probes if d["rep"]["served"])
    elif name == "batch2":
        assert any(d["rep"]["ref"] and d["rep"]["ref"][0] > 2048 for d in probes)
        assert any(d["rep"]["ref"] and 0 < d["rep"]["ref"][0] <= 2048 for d in probes)
        assert all(d["n"] >= 2049 for d in probes)
        if which == "gpu":
            assert all(d["rep"]["n_active"] == 8 for d in probes if d["rep"]["served"])
    elif name == "highbits":
        assert all(k > 0 for k in extras["key_bits"]), extras  # rows with bit 63, with bit 62, with neither
    elif name == "changes":
        assert sum(1 for d in probes if d["rep"]["audited"]) == len(probes) or keyed != "1"
