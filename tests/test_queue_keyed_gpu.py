"""Queue scans over the keyed membership table on the device (scan_server's SOP_QUEUE over KeyedRow blocks): parity with
the oracle with the table on and off, with the run's other scans split over the waves (CCMI_GOAL_SPLIT=1; queue commands
stay unsplit) and with a small
snapshot pool (CCMI_SNAPSHOT_POOL_ROWS: the segment path still uses the pool). Child processes, as test_queue_keyed.py."""
import pytest

from test_queue_keyed import check_counters, run_worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(gpu_lib, oracle_lib):
    return True


@pytest.mark.parametrize("keyed", ["1", "0"])
@pytest.mark.parametrize("case", ["b20_default", "b300_c1", "b300_default", "dead2"])
def test_gpu_keyed_queue_matches_oracle(built, case, keyed):
    c = run_worker("gpu", case, CCMI_QUEUE_KEYED=keyed)
    if case != "b300_default":  # (that chain ends in a hard goal's failure before any queue scan)
        check_counters(c, keyed == "1")


def test_gpu_keyed_queue_goal_split(built):
    """The whole run with CCMI_GOAL_SPLIT=1: the split (several waves per candidate) applies to the run's cross, segment
    and pair scans. Queue commands always carry goalParts = 1 (Device::scanQueueImpl), so the keyed queue scans
    themselves run unsplit here; what this covers is that they stay correct next to split scans on the same server."""
    check_counters(run_worker("gpu", "b300_c1", CCMI_QUEUE_KEYED="1", CCMI_GOAL_SPLIT="1"), True)


def test_gpu_keyed_queue_small_pool(built):
    check_counters(run_worker("gpu", "b20_default", CCMI_QUEUE_KEYED="1", CCMI_SNAPSHOT_POOL_ROWS="65536"), True)
