"""Pins the restatement the partition load tests compare with (partition_load_support.Restatement) to the oracle.

The oracle has no per-replica load accessor, but it has every broker's utilization. Followers carry no NW_OUT
(Replica.makeFollower clears it), so a broker's NW_OUT load is the sum of the loads of the partitions it leads:

    sum over the partitions led on b of the restatement's nw_out (default mode)  ~  oc.broker_util(b, NW_OUT) = u

within 2^-22 |u| + (2R + 2A) 2^-53 S, A the action count and S the sum of the absolute LEADER_BYTES_OUT and
REPLICATION_BYTES_OUT window values of all replicas: two float32 roundings on each side (the broker's two avg() values
against each partition's), and double running-sum error as in test_broker_stats.py (at most R + 2A updates of the
broker's running sums in the reference plus R additions here). The replay of LEADERSHIP actions is what moves NW_OUT
between brokers, so a wrong replay shows here. Worst error / bound on these clusters: 0.20 (20 brokers, 2532 actions,
376 LEADERSHIP) and 0.19 (130 brokers, 4582 actions, 942 LEADERSHIP).
"""
import pytest

import ccmi
from oracle_binding import ArrayDesc, OracleCluster
from parity import constraint
from partition_load_support import DEFAULT, LEADERSHIP, NW_OUT, Restatement


@pytest.mark.parametrize("num_brokers", [20, 130], ids=["b20", "b130"])
def test_restatement_matches_the_oracle_broker_nw_out(oracle_lib, num_brokers):
    oc = OracleCluster.random(num_racks=5, num_brokers=num_brokers, num_replicas=6000, num_topics=300)
    flat = ArrayDesc(oc.export(), oc.W)
    rs = Restatement(flat.desc)
    oc.optimize(list(ccmi.DEFAULT_GOALS), constraint(1.05, max_replicas=3000))
    actions = oc.actions()
    assert sum(1 for a in actions if a[0] == LEADERSHIP) > 0
    rs.apply(actions)
    assert [rs.broker[r] for r in rs.leader] == oc.leader_distribution()
    slack = (2 * rs.R + 2 * len(actions)) * 2.0 ** -53 * rs.abs_nw_out
    key = rs.keys(NW_OUT, DEFAULT)
    led = [0.0] * rs.B
    for p in range(rs.P):
        led[rs.broker[rs.leader[p]]] += key[p]
    worst = 0.0
    for b in range(rs.B):
        u = oc.broker_util(b, NW_OUT)
        bound = 2.0 ** -22 * abs(u) + slack
        worst = max(worst, abs(led[b] - u) / bound)
        assert abs(led[b] - u) <= bound, (b, led[b], u, bound)
    print(f"brokers {num_brokers}: P {rs.P} W {rs.W} actions {len(actions)} leaderships {rs.leaderships} "
          f"worst error / bound {worst:.2f}")
