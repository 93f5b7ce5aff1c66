"""Queue scans over the keyed membership table (engine/keyed_table.h, CCMI_QUEUE_KEYED) on the CPU emulation: the same
decisions, candidate counts and statistics as the oracle with the table on and off, the paths it adds taken, and the
fall-back to the snapshot directory when a broker outgrows its block. The emulated Device has no device table
(Device::hasKeyedTable() is false there): these runs cover the engine's side — the mirror's incremental sync from the
relocation log, the skipKey continuation, the slot decoding and the candidate counts — with the mirror's blocks scanned
in key order (Device::scanQueueKeyedFlat); the device's reading of the table is covered by test_queue_keyed_gpu.py.
Each run is a child process
(tests/queue_keyed_worker.py): the knobs and CCMI_PROFILE are read when the library starts."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "queue_keyed_worker.py")


def run_worker(which, case, **env):
    e = dict(os.environ, CCMI_PROFILE="1", **env)
    r = subprocess.run([sys.executable, WORKER, which, case], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "parity ok" in r.stdout
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#(\S+)\s+(-?\d+)", r.stderr)}


def check_counters(c, keyed):
    """The path the run's queue scans took, from the session's CCMI_PROFILE counters."""
    if keyed:
        assert c.get("queue.keyed.scans", 0) > 0 and c.get("queue.keyed.changes", 0) > 0
        assert "queue.ns.snapshots" not in c and "queue.sync.brokers" not in c  # no sorted snapshot for the queue path
        assert c.get("queue.keyed.overflow", 0) == 0
    else:
        assert c.get("queue.keyed.scans", 0) == 0 and c.get("queue.sync.brokers", 0) > 0


@pytest.fixture(scope="module")
def built(emu_lib, oracle_lib):
    return True


@pytest.mark.parametrize("keyed", ["1", "0"])
@pytest.mark.parametrize("case", ["b20_default", "b300_c1", "b300_default", "dead2"])
def test_emu_keyed_queue_matches_oracle(built, case, keyed):
    c = run_worker("emu", case, CCMI_QUEUE_KEYED=keyed)
    if case == "b300_default":
        return  # (this chain ends in a hard goal's failure before any queue scan: parity of the failure only)
    check_counters(c, keyed == "1")
    # the continuation on the head entry (skipKey) and the re-add both fired
    assert c.get("in.move.continue", 0) > 0 and c.get("in.move.readd", 0) > 0


@pytest.mark.parametrize("case,stride", [("b20_default", "200"), ("b20_default", "300"), ("dead2", "64"),
                                         ("b300_c1", "100")])
def test_emu_keyed_stride_overflow_falls_back(built, case, stride):
    """A stride below the largest broker (CCMI_QUEUE_KEYED_STRIDE, tests only): the table is refused for the Specs
    whose rows do not fit (a Spec with a utilization limit selects few replicas and may still fit) and their scans take
    the snapshot directory; same decisions as the oracle."""
    c = run_worker("emu", case, CCMI_QUEUE_KEYED="1", CCMI_QUEUE_KEYED_STRIDE=stride)
    assert c.get("queue.keyed.overflow", 0) > 0
    assert c.get("queue.sync.brokers", 0) > 0  # scans went through the snapshot directory
