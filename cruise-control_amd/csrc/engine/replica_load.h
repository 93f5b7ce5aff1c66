// The per-replica half of K18 (ccmi_builder_populate_from_aggregator), written once for the device kernels
// (kernels/load_model.hip) and for the host unit test (tests/cpp/test_replica_load.cpp): the loads
// MonitorUtils.populatePartitionLoad hands to setReplicaLoad, restating
//   MonitorUtils.getAggregatedMetricValues / adjustCpuUsage / fillInReplicationBytesOut / toFollowerMetricValues
//                                                monitor/MonitorUtils.java:83-107,198-265
//   ModelUtils.getFollowerCpuUtilFromLeaderLoad  model/ModelUtils.java:64-80 (static weights, ModelParameters.java:23-31)
// The reference walks a partition's replicas in PartitionInfo.replicas() order over ONE shared values object and
// mutates it on the way: the first replica turns CPU into a percentage, the leader fills in REPLICATION_BYTES_OUT. A
// replica's load therefore depends on where it stands relative to the leader; replicaLoadWindow reproduces that from
// the replica's index alone, so every replica (and every window) is computed independently:
//   * CPU is (float)((double) cpu * 100), rounded once, for every replica;
//   * the leader's REPLICATION_BYTES_OUT is (float)((double) LEADER_BYTES_IN * (n - 1));
//   * a follower after the leader sees that filled value in its NW_OUT group sum, a follower before it the reported one;
//   * a group sum (AggregatedMetricValues.valuesForGroup) adds the group's metrics into a zeroed float in metric-id order;
//   * the follower's CPU is the double expression of getFollowerCpuUtilFromLeaderLoad, then (float); its two outbound
//     metrics are 0.
// Compile with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define CCMI_RLOAD __host__ __device__ __forceinline__
#else
#define CCMI_RLOAD inline
#endif

namespace ccmi {
namespace rload {

// ccmi_metric (include/ccmi.h)
constexpr int kCpu = 0, kDisk = 1, kLeaderBytesIn = 2, kLeaderBytesOut = 3, kReplicationBytesIn = 4,
              kReplicationBytesOut = 5, kMetrics = 6;
constexpr int kMaxReplicas = 8;                      // replicas of one partition (ccmi_builder_populate_partition)
constexpr double kUnitIntervalToPercentage = 100.0;  // MonitorUtils.UNIT_INTERVAL_TO_PERCENTAGE
constexpr double kCpuWeightLeaderBytesIn = 0.7;      // ModelParameters defaults
constexpr double kCpuWeightLeaderBytesOut = 0.15;
constexpr double kCpuWeightFollowerBytesIn = 0.15;

// One window of one replica. lead[6]: the partition's aggregated leader values of that window in ccmi_metric order;
// idx: the replica's position among the partition's n replicas; leaderIdx: the leader's. out[6]: the replica's load.
CCMI_RLOAD void replicaLoadWindow(const float lead[kMetrics], int idx, int leaderIdx, int n, float out[kMetrics]) {
  const float cpu = (float)((double)lead[kCpu] * kUnitIntervalToPercentage);                // adjustCpuUsage
  const float filled = (float)((double)lead[kLeaderBytesIn] * (double)(n - 1));             // fillInReplicationBytesOut
  out[kDisk] = lead[kDisk];
  out[kLeaderBytesIn] = lead[kLeaderBytesIn];
  out[kReplicationBytesIn] = lead[kReplicationBytesIn];
  if (idx == leaderIdx) {
    out[kCpu] = cpu;
    out[kLeaderBytesOut] = lead[kLeaderBytesOut];
    out[kReplicationBytesOut] = filled;
    return;
  }
  // toFollowerMetricValues over the shared values as this follower finds them
  const float rbo = idx > leaderIdx ? filled : lead[kReplicationBytesOut];
  float in = 0.0f, outb = 0.0f;  // valuesForGroup(NW_IN), valuesForGroup(NW_OUT)
  in += lead[kLeaderBytesIn];
  in += lead[kReplicationBytesIn];
  outb += lead[kLeaderBytesOut];
  outb += rbo;
  const double lbi = in, lbo = outb, c = cpu;
  double f;
  if (lbi == 0.0 && lbo == 0.0)
    f = 0.0;
  else
    f = c * (kCpuWeightFollowerBytesIn * lbi) / (kCpuWeightLeaderBytesIn * lbi + kCpuWeightLeaderBytesOut * lbo);
  out[kCpu] = (float)f;
  out[kLeaderBytesOut] = 0.0f;
  out[kReplicationBytesOut] = 0.0f;
}

}  // namespace rload
}  // namespace ccmi
