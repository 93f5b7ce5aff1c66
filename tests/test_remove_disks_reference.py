"""The yardstick of test_remove_disks.py (remove_disks_support.Yardstick) pinned to the reference's own test and to
the pieces of Java semantics it restates. No library is loaded here.

RemoveDisksTest (src/test/java/.../analyzer/RemoveDisksTest.java:62-133): 3 brokers with logdirs /mnt/i00 and /mnt/i01
of 150000 each (TestConstants.DISK_CAPACITY), broker DISK capacity 300000, one replica of topic-0 on broker 0
/mnt/i00, /mnt/i00 marked for removal, IntraBrokerDiskCapacityGoal(true) with the default capacity threshold 0.8.
  DISK load 300000 / 4 = 75000        -> one proposal, the replica moves to /mnt/i01 on broker 0 (:122-128)
  DISK load 0.0                       -> the same (:69-70: the flag moves empty replicas too)
  DISK load 300000 / 2 * 0.8 = 120000 -> OptimizationFailureException (:129-132)
"""
import pytest

from remove_disks_support import (INTRA_MOVE, LOGDIR0, LOGDIR1, REMOVE_DISKS_TEST_ROWS, IllegalArgument, Yardstick,
                                  double_int_value, java_fixed, remove_disks_test_model, tim_sort_small)


@pytest.mark.parametrize("name,load,optimizes", REMOVE_DISKS_TEST_ROWS, ids=[r[0] for r in REMOVE_DISKS_TEST_ROWS])
def test_remove_disks_test_rows(name, load, optimizes):
    flat = remove_disks_test_model(load)
    y = Yardstick(flat.desc)
    (d0,), (d1,) = y.disks_named({0: [LOGDIR0]}), y.disks_named({0: [LOGDIR1]})
    y.mark([d0])  # the reference test marks without checkCanRemoveDisks
    out = y.outcome(0.8)
    if optimizes:
        assert out == ("ok",)
        assert y.actions == [(INTRA_MOVE, 0, 0, 0, -1, d0, d1)]
        assert y.proposals() == {0: (frozenset({(0, d0)}), frozenset({(0, d1)}))}
    else:
        assert out[0] == "fail" and y.actions == []
        # 0 + 120000 < 150000 * 0.8 is false: the replica stays and the zero-capacity disk is over its limit
        assert out[1] == ("[IntraBrokerDiskCapacityGoal] Utilization (120000.00) for disk Disk[logdir=/mnt/i00,"
                          "state=ALIVE,capacity=0.000000,replicaCount=1] on broker 0 is above capacity limit.")
        assert out[2:] == (1, 120000.0 / 0.8)


def test_without_the_flag_the_empty_replica_stays():
    """selfSatisfied without the flag is `> 0` (:168-171) and a zero-capacity disk of utilization 0 is not over."""
    flat = remove_disks_test_model(0.0)
    y = Yardstick(flat.desc)
    y.mark(y.disks_named({0: [LOGDIR0]}))
    assert y.outcome(0.8, empty_zero=False) == ("ok",) and y.actions == []


def test_check_can_remove_disks():
    flat = remove_disks_test_model(75000.0)
    y = Yardstick(flat.desc)
    with pytest.raises(IllegalArgument, match=r"^Invalid log dirs provided for broker 1\.$"):
        y.disks_named({1: ["/mnt/i07"]})
    with pytest.raises(IllegalArgument, match=r"^No log dir remaining to move replicas to for broker 2\.$"):
        y.check_can_remove(y.disks_named({0: [LOGDIR0], 2: [LOGDIR0, LOGDIR1]}), 0.8)
    # 75000 / 150000 = 0.5: over 0.4, not over 0.5 (the comparison is >)
    with pytest.raises(IllegalArgument, match=r"^Not enough remaining capacity to move replicas to for broker 0\.$"):
        y.check_can_remove(y.disks_named({0: [LOGDIR0]}), 0.4)
    y.check_can_remove(y.disks_named({0: [LOGDIR0]}), 0.5)


def test_java_pieces():
    assert [double_int_value(x) for x in (0.9, -0.9, -1.5, float("nan"), 1e300, -1e300)] == \
        [0, 0, -1, 0, 2147483647, -2147483648]
    assert java_fixed(4.668254405260086e-08, 2) == "0.00" and java_fixed(0.0, 6) == "0.000000"
    assert java_fixed(0.125, 2) == "0.13" and java_fixed(120000.0, 2) == "120000.00"  # HALF_UP
    a = [5, 3, 9, 1, 7]
    tim_sort_small(a, lambda x, y: x - y)
    assert a == [1, 3, 5, 7, 9]
    # a comparator that calls everything within 1.0 equal keeps such neighbours in place (binary insertion is stable)
    b = [0.2, 0.9, 0.1, 3.0, 2.5]
    tim_sort_small(b, lambda x, y: double_int_value(x - y))
    assert b == [0.2, 0.9, 0.1, 3.0, 2.5]
    c = [4, 3, 2, 1]  # a strictly descending run is reversed in place
    tim_sort_small(c, lambda x, y: x - y)
    assert c == [1, 2, 3, 4]
