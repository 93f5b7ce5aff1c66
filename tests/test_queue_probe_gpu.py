"""The scan server's SOP_QUEUE branch (kernels/scan.hip) probed one scan at a time against a plain host loop
(ClusterModel._queue_probe, csrc/ccmi_queue_probe.cpp): the lists of test_queue_probe.py sent to the HIP kernel, with the
keyed membership table (CCMI_QUEUE_KEYED=1) and with the snapshot directory (=0). Every keyed probe must be answered by
a queue command (served == 1), leave the table equal to the model (audit 0, read back through its host mapping) and
name the host loop's (entry, replica, column); equality is exact. What each scenario reaches in the branch:

* columns_rd / columns_lrd: N in {1, 2, 63, 64, 65, 255, 256, 257} against blocks of 1, 3, 4, 5 and 61 rows (13 to 33
  leader rows for the leaders-only program): len * N on both sides of the 256-slot tile, N on both sides of the
  candidates' LDS limit (kBlock), the only accepting column first or last, nothing accepted; columns_rd also asserts from
  the probes' coverage facts that sMinPub's reset fired (an accepted row a tile or more before the winner's slot) and
  that it did not (the winner first, another accepted row a tile later).
* single: entries of 0, 1 and 2 rows, the winner in the lowest-key row, in a higher-key row and in the highest-key row of
  its block (every row before it rejected; asserted from the report's win_rank), the head continuation with skip_key at
  the head's lowest, a middle and its highest key, a head whose only accepted row is masked, a head of one row.
* multi and batch2 run with CCMI_SERVER_BLOCKS=8 (asserted: nActive == 8), which is the only way to give a workgroup
  several entries at these sizes: 9, 16, 17 and 40 entries with empty ones between, the winner first in its workgroup,
  later in it (entry 8; from 17 entries on entry 16 follows it on that workgroup with rows, asserted, so a tile holds
  rows of both), last, and on another workgroup with a lower entry (the blockBest exit); the first scan after multi's
  ~80 applied moves carries more rows than a command stages and is flattened (asserted served == 0, not counted);
  2,049 and more entries, the winner beyond entry 2,048 (the second batch of the kb loop) and in the first batch.
* highbits: prio_offline and prio_immigrants keys (bits 63 and 62) next to keys without them in one block.
* changes: probes and table audits between applied moves (a row leaving its block's last, first and a middle slot, a
  block emptied, blocks grown, a leadership move) and after another Spec was bound (a full rebuild). Under the
  leaders-only Spec a leadership move makes one row leave a block and another join one; a key is rewritten in place only
  where both replicas stay selected, so that is probed under an all-replicas NW_OUT Spec.
* excl_lead: brokers excluded for leadership, so exclLeadBlocked filters columns per row.
* full_block (keyed only): CCMI_QUEUE_KEYED_STRIDE equal to the longest block, and one less (the directory serves it).
Each scenario is a child process under a time-out (the knobs are read when the library starts)."""
import pytest

from queue_probe_support import SCENARIOS, check_coverage, check_probes, expected_served, run_scenario

pytestmark = pytest.mark.gpu

EIGHT_WORKGROUPS = ("multi", "multi_heads", "batch2")


@pytest.fixture(scope="module")
def built(gpu_lib):
    return True


def run(scenario, **env):
    if scenario in EIGHT_WORKGROUPS:
        env["CCMI_SERVER_BLOCKS"] = "8"
    return run_scenario("gpu", scenario, timeout=120, **env)


@pytest.mark.parametrize("keyed", ["1", "0"])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_gpu_queue_probes(built, scenario, keyed):
    probes, extras, seconds = run(scenario, CCMI_QUEUE_KEYED=keyed)
    served = check_probes(probes, "gpu", keyed)
    flattened = len(probes) - expected_served(probes)  # `settle` probes, asserted unserved by check_probes
    print(f"{scenario} keyed={keyed}: {len(probes)} probes, {served} served by SOP_QUEUE, {flattened} flattened by "
          f"design, {seconds:.1f} s")
    check_coverage(scenario, probes, extras, "gpu", keyed)
    assert served == expected_served(probes)  # the directory path is served by queue commands too


def test_gpu_queue_probe_skip_key_at_the_largest_key(built):
    """The kernel masks the head's rows with key <= skip_key; at the largest key that is every row (the multi scenario's
    *_head probes, run alone as multi_heads), and the host side's count of the masked rows must agree
    (test_queue_probe.py has the host half)."""
    probes, _, _ = run("multi_heads", CCMI_QUEUE_KEYED="1")
    heads = [d for d in probes if d["name"].endswith("_head")]
    assert len(heads) == 12 and all(d["rep"]["head_masked"] > 0 for d in heads)
    assert check_probes(probes, "gpu", "1") == len(heads)
    assert any(d["rep"]["ref"] for d in heads)


def test_gpu_queue_probe_full_block(built):
    _, extras, _ = run("full_block", CCMI_QUEUE_KEYED="1")
    longest = extras["longest"]
    fits, _, seconds = run("full_block", CCMI_QUEUE_KEYED="1", CCMI_QUEUE_KEYED_STRIDE=str(longest))
    served = check_probes(fits, "gpu", "1")
    print(f"full_block stride={longest}: {len(fits)} probes, {served} served by SOP_QUEUE, {seconds:.1f} s")
    assert all(d["rep"]["stride"] == longest for d in fits) and any(d["rep"]["win_len"] == longest for d in fits)
    tight, _, _ = run("full_block", CCMI_QUEUE_KEYED="1", CCMI_QUEUE_KEYED_STRIDE=str(longest - 1))
    check_probes(tight, "gpu", "0")
    assert [d["rep"]["ref"] for d in tight] == [d["rep"]["ref"] for d in fits]
