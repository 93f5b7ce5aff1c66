"""One queue scan at a time against a plain host loop (ClusterModel._queue_probe, csrc/ccmi_queue_probe.cpp), on the CPU
emulation. The probe runs the call Engine::queueScan makes for a queue, a column list, a Spec and a program chosen by
the test, and compares its winner, as (entry, replica, column), with the first accepted pair of a row-major walk over the
model's own rows. With CCMI_QUEUE_KEYED=1 the emulated answer comes from Device::scanQueueKeyedFlat over the keyed
mirror, with =0 from the emulation's scanQueue over the snapshot directory; test_queue_probe_gpu.py sends the same
lists to the HIP kernel, so three implementations have to agree with the host loop. Each scenario
(tests/queue_probe_worker.py) is a child process: the knobs are read when the library starts.

The scenarios: column counts on both sides of the kernel's tile and LDS limits against blocks of 1 to 61 rows
(columns_*), single entries with the winner in the lowest-key, a higher-key and the highest-key row, and the head
continuation (single), several entries per workgroup (multi), more than 2,048 entries (batch2: 2,800 brokers of 1 to 3
leader rows; with fewer brokers no column of this generator's clusters leaves 2,049 entries without an accept; about 2 s
on the CPU, so it is kept), keys with bits 63 and 62 (highbits), probes between applied moves, with keys rewritten in
place under an all-replicas NW_OUT Spec (changes), columns filtered per row by brokers excluded for leadership
(excl_lead), and a block as long as the table's stride (full_block)."""
import pytest

from queue_probe_support import SCENARIOS, check_coverage, check_probes, run_scenario


@pytest.fixture(scope="module")
def built(emu_lib):
    return True


@pytest.mark.parametrize("keyed", ["1", "0"])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_emu_queue_probes(built, scenario, keyed):
    probes, extras, _ = run_scenario("emu", scenario, CCMI_QUEUE_KEYED=keyed)
    check_probes(probes, "emu", keyed)
    check_coverage(scenario, probes, extras, "emu", keyed)


def test_emu_queue_probe_skip_key_at_the_largest_key(built):
    """A continuation whose skip_key is the largest 64-bit key masks every head row. The flattened scan used to count
    the masked rows as below(skip_key + 1), which wraps to 0 there and masked none (the kernel compares key <= skip_key).
    The multi scenario's *_head probes send that key; multi_heads runs them alone."""
    probes, _, _ = run_scenario("emu", "multi_heads", CCMI_QUEUE_KEYED="1")
    heads = [d for d in probes if d["name"].endswith("_head")]
    assert len(heads) == 12
    assert all(d["args"]["skip_key"] == (1 << 64) - 1 and d["rep"]["head_masked"] > 0 for d in heads)
    check_probes(probes, "emu", "1")
    assert all(d["rep"]["ref"] is None or d["rep"]["ref"][0] >= 1 for d in heads)
    assert any(d["rep"]["ref"] for d in heads)


def test_emu_queue_probe_full_block(built):
    """The all-replicas Spec with CCMI_QUEUE_KEYED_STRIDE equal to its longest block: the block fills its stride. With one
    slot less the Spec is refused and the snapshot directory serves the same probes with the same winners."""
    _, extras, _ = run_scenario("emu", "full_block", CCMI_QUEUE_KEYED="1")
    longest = extras["longest"]
    fits, _, _ = run_scenario("emu", "full_block", CCMI_QUEUE_KEYED="1", CCMI_QUEUE_KEYED_STRIDE=str(longest))
    check_probes(fits, "emu", "1")
    assert all(d["rep"]["stride"] == longest for d in fits)
    assert any(d["rep"]["win_len"] == longest for d in fits)
    tight, _, _ = run_scenario("emu", "full_block", CCMI_QUEUE_KEYED="1", CCMI_QUEUE_KEYED_STRIDE=str(longest - 1))
    check_probes(tight, "emu", "0")
    assert [d["rep"]["ref"] for d in tight] == [d["rep"]["ref"] for d in fits]


def test_emu_queue_probe_refuses_bad_queues(built, emu_lib):
    """Indices are checked before anything reaches the device: a broker out of range, a broker queued twice and a
    continuation without a head are CCMI_E_INVALID."""
    import ccmi

    buf = ccmi.RandomCluster.generate(emu_lib, num_racks=3, num_brokers=6, num_replicas=300, num_topics=10)
    cm = ccmi.ClusterModel(buf.desc, device=0, lib=emu_lib, keepalive=buf)
    ccmi.Goal("ReplicaDistributionGoal", ccmi.BalancingConstraint()).optimize(cm, [])
    ok = cm._queue_probe({}, tail=[0, 1], cands=[2])
    assert ok["dev"] == ok["ref"]
    for kw in (dict(tail=[0, 6], cands=[2]), dict(tail=[0, 1], cands=[-1]), dict(tail=[0, 1, 0], cands=[2]),
               dict(head=1, tail=[0, 1], cands=[2]), dict(tail=[0], cands=[2], skip_key=5),
               dict(tail=[0], cands=[2], self_goal="RackAwareGoal")):
        with pytest.raises(ccmi.IllegalArgumentException):
            cm._queue_probe({}, **kw)
