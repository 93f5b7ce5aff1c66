"""Python binding of libccmi.so (include/ccmi.h) mirroring the reference's optimizer interface.

Names follow the reference so parity tests read like the reference's own tests:

  ClusterModel            <- com.linkedin.kafka.cruisecontrol.model.ClusterModel (a device session)
  GoalOptimizer           <- analyzer/GoalOptimizer.java  (optimizations(), GoalOptimizer.java:435-524)
  <Goal>                  <- analyzer/goals/*Goal.java     (name(), optimize(), actionAcceptance())
  OptimizationOptions     <- analyzer/OptimizationOptions.java
  BalancingConstraint     <- analyzer/BalancingConstraint.java (AnalyzerConfig.java defaults)
  OptimizerResult         <- analyzer/OptimizerResult.java  (proposals, per-goal stats)
  ExecutionProposal       <- executor/ExecutionProposal.java
  RandomCluster           <- src/test/.../model/RandomCluster.java (fixture generator)

Errors map to the reference's exceptions: OptimizationFailureException, IllegalStateException,
IllegalArgumentException; a missing/unsupported device raises DeviceError (no CPU fallback exists).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libccmi.so")

RESOURCES = ("CPU", "NW_IN", "NW_OUT", "DISK")
CPU, NW_IN, NW_OUT, DISK = range(4)

GOAL_KINDS: Dict[str, int] = {
    "RackAwareGoal": 0,
    "MinTopicLeadersPerBrokerGoal": 1,
    "ReplicaCapacityGoal": 2,
    "DiskCapacityGoal": 3,
    "NetworkInboundCapacityGoal": 4,
    "NetworkOutboundCapacityGoal": 5,
    "CpuCapacityGoal": 6,
    "ReplicaDistributionGoal": 7,
    "PotentialNwOutGoal": 8,
    "DiskUsageDistributionGoal": 9,
    "NetworkInboundUsageDistributionGoal": 10,
    "NetworkOutboundUsageDistributionGoal": 11,
    "CpuUsageDistributionGoal": 12,
    "TopicReplicaDistributionGoal": 13,
    "LeaderReplicaDistributionGoal": 14,
    "LeaderBytesInDistributionGoal": 15,
    "IntraBrokerDiskCapacityGoal": 16,
    "IntraBrokerDiskUsageDistributionGoal": 17,
    "PreferredLeaderElectionGoal": 18,
    "RackAwareDistributionGoal": 19,
    "BrokerSetAwareGoal": 20,
    "TopicLeaderReplicaDistributionGoal": 21,
    "KafkaAssignerEvenRackAwareGoal": 22,
    "KafkaAssignerDiskUsageDistributionGoal": 23,
}
GOAL_NAMES = {v: k for k, v in GOAL_KINDS.items()}
# new IntraBrokerDiskCapacityGoal(true), the goal of RemoveDisksRunnable (:65-67): goal kind 24 of the library. It is
# the same class, so Goal.name() stays IntraBrokerDiskCapacityGoal and GOAL_KINDS (simple class name -> kind) has no
# entry of its own; goals_from_names and the by-name acceptance calls know it by this spelling.
REMOVE_DISKS_GOAL = "IntraBrokerDiskCapacityGoal(true)"
REMOVE_DISKS_GOAL_KIND = 24
GOAL_NAMES[REMOVE_DISKS_GOAL_KIND] = "IntraBrokerDiskCapacityGoal"


def goal_kind(name: str) -> int:
    """The library's goal kind of a goal name: a simple class name, or REMOVE_DISKS_GOAL."""
    return REMOVE_DISKS_GOAL_KIND if name == REMOVE_DISKS_GOAL else GOAL_KINDS[name]
# default.goals in priority order (config/constants/AnalyzerConfig.java:352-367, TestConstants.DEFAULT_GOALS_VALUES)
DEFAULT_GOALS = ("RackAwareGoal", "MinTopicLeadersPerBrokerGoal", "ReplicaCapacityGoal", "DiskCapacityGoal",
                 "NetworkInboundCapacityGoal", "NetworkOutboundCapacityGoal", "CpuCapacityGoal",
                 "ReplicaDistributionGoal", "PotentialNwOutGoal", "DiskUsageDistributionGoal",
                 "NetworkInboundUsageDistributionGoal", "NetworkOutboundUsageDistributionGoal",
                 "CpuUsageDistributionGoal", "TopicReplicaDistributionGoal", "LeaderReplicaDistributionGoal",
                 "LeaderBytesInDistributionGoal")
# config C1's chain
C1_GOALS = ("ReplicaDistributionGoal", "DiskUsageDistributionGoal", "NetworkInboundUsageDistributionGoal",
            "NetworkOutboundUsageDistributionGoal", "CpuUsageDistributionGoal")
# intra.broker.goals (AnalyzerConfig INTRA_BROKER_GOALS default, IntraBrokerRebalanceTest.java:105-106)
INTRA_BROKER_GOALS = ("IntraBrokerDiskCapacityGoal", "IntraBrokerDiskUsageDistributionGoal")
# Goals whose drivers are implemented in this build.
IMPLEMENTED = DEFAULT_GOALS + INTRA_BROKER_GOALS + ("PreferredLeaderElectionGoal", "RackAwareDistributionGoal",
                                                   "BrokerSetAwareGoal", "TopicLeaderReplicaDistributionGoal",
                                                   "KafkaAssignerEvenRackAwareGoal",
                                                   "KafkaAssignerDiskUsageDistributionGoal")
# replica.to.broker.set.mapping.policy.class values (include/ccmi.h ccmi_broker_set_policy)
BROKER_SET_POLICIES = {"TopicNameHashBrokerSetMappingPolicy": 0, "ReplicaToOriginalBrokerSetMappingPolicy": 1}

ACTION_TYPES = ("INTER_BROKER_REPLICA_MOVEMENT", "LEADERSHIP_MOVEMENT", "INTER_BROKER_REPLICA_SWAP",
                "INTRA_BROKER_REPLICA_MOVEMENT", "INTRA_BROKER_REPLICA_SWAP")
ACCEPTANCE = ("ACCEPT", "REPLICA_REJECT", "BROKER_REJECT")
# ccmi_swap_code: the cells of ClusterModel.swaps_acceptance_grid
SWAP_CODES = ["ACCEPT", "REPLICA_REJECT", "BROKER_REJECT", "SOURCE_NOT_LEGIT", "CANDIDATE_NOT_LEGIT"]


# ----------------------------------------------------------------------------------------------- ctypes layouts
class ClusterDesc(C.Structure):
    _fields_ = [("num_windows", C.c_int32), ("num_racks", C.c_int32), ("num_brokers", C.c_int32),
                ("broker_id", C.POINTER(C.c_int32)), ("broker_rack", C.POINTER(C.c_int32)),
                ("broker_state", C.POINTER(C.c_int32)), ("broker_capacity", C.POINTER(C.c_double)),
                ("num_topics", C.c_int32), ("topic_names", C.POINTER(C.c_char_p)),
                ("num_partitions", C.c_int32), ("partition_topic", C.POINTER(C.c_int32)),
                ("partition_number", C.POINTER(C.c_int32)), ("partition_offset", C.POINTER(C.c_int32)),
                ("partition_replicas", C.POINTER(C.c_int32)), ("num_replicas", C.c_int32),
                ("replica_partition", C.POINTER(C.c_int32)), ("replica_broker", C.POINTER(C.c_int32)),
                ("replica_is_leader", C.POINTER(C.c_uint8)), ("replica_offline", C.POINTER(C.c_uint8)),
                ("replica_load", C.POINTER(C.c_float)), ("replica_load_order", C.POINTER(C.c_int32)),
                ("num_disks", C.c_int32), ("disk_broker", C.POINTER(C.c_int32)),
                ("disk_logdir", C.POINTER(C.c_char_p)), ("disk_capacity", C.POINTER(C.c_double)),
                ("replica_disk", C.POINTER(C.c_int32)), ("num_disk_assignments", C.c_int32),
                ("disk_assign_replica", C.POINTER(C.c_int32)), ("disk_assign_disk", C.POINTER(C.c_int32)),
                ("num_replica_loads", C.c_int32), ("broker_host", C.POINTER(C.c_int32)),
                ("disk_demoted", C.POINTER(C.c_uint8))]


class ConstraintStruct(C.Structure):
    _fields_ = [("resource_balance_percentage", C.c_double * 4), ("capacity_threshold", C.c_double * 4),
                ("low_utilization_threshold", C.c_double * 4), ("replica_balance_percentage", C.c_double),
                ("leader_replica_balance_percentage", C.c_double), ("topic_replica_balance_percentage", C.c_double),
                ("topic_replica_balance_min_gap", C.c_int32), ("topic_replica_balance_max_gap", C.c_int32),
                ("goal_violation_distribution_threshold_multiplier", C.c_double),
                ("max_replicas_per_broker", C.c_int64), ("overprovisioned_max_replicas_per_broker", C.c_int64),
                ("overprovisioned_min_brokers", C.c_int32), ("overprovisioned_min_extra_racks", C.c_int32),
                ("num_broker_sets", C.c_int32), ("broker_set_policy", C.c_int32),
                ("broker_set_names", C.POINTER(C.c_char_p)), ("broker_set_offset", C.POINTER(C.c_int32)),
                ("broker_set_members", C.POINTER(C.c_int32)), ("min_leader_topics", C.POINTER(C.c_int32)),
                ("num_min_leader_topics", C.c_int32), ("min_topic_leaders_per_broker", C.c_int32),
                ("topic_leader_replica_balance_percentage", C.c_double),
                ("topic_leader_replica_balance_min_gap", C.c_int32), ("topic_leader_replica_balance_max_gap", C.c_int32),
                ("topic_leader_replica_balance_margin", C.c_double)]


class OptionsStruct(C.Structure):
    _fields_ = [("excluded_topics", C.POINTER(C.c_int32)), ("num_excluded_topics", C.c_int32),
                ("excluded_brokers_for_leadership", C.POINTER(C.c_int32)),
                ("num_excluded_brokers_for_leadership", C.c_int32),
                ("excluded_brokers_for_replica_move", C.POINTER(C.c_int32)),
                ("num_excluded_brokers_for_replica_move", C.c_int32), ("triggered_by_goal_violation", C.c_int32),
                ("requested_destination_broker_ids", C.POINTER(C.c_int32)),
                ("num_requested_destination_broker_ids", C.c_int32), ("only_move_immigrant_replicas", C.c_int32),
                ("fast_mode", C.c_int32)]


class ActionStruct(C.Structure):
    _fields_ = [("type", C.c_int32), ("partition", C.c_int32), ("source_broker", C.c_int32),
                ("destination_broker", C.c_int32), ("destination_partition", C.c_int32),
                ("source_disk", C.c_int32), ("destination_disk", C.c_int32)]


class StatsStruct(C.Structure):
    _fields_ = [("resource_avg", C.c_double * 4), ("resource_max", C.c_double * 4),
                ("resource_min", C.c_double * 4), ("resource_std", C.c_double * 4),
                ("num_balanced_brokers_by_resource", C.c_int32 * 4), ("potential_nw_out_avg", C.c_double),
                ("potential_nw_out_max", C.c_double), ("potential_nw_out_min", C.c_double),
                ("potential_nw_out_std", C.c_double), ("num_brokers_under_potential_nw_out", C.c_int32),
                ("replica_avg", C.c_double), ("replica_std", C.c_double), ("replica_max", C.c_int32),
                ("replica_min", C.c_int32), ("leader_avg", C.c_double), ("leader_std", C.c_double),
                ("leader_max", C.c_int32), ("leader_min", C.c_int32), ("topic_replica_avg", C.c_double),
                ("topic_replica_std", C.c_double), ("topic_replica_max", C.c_int32), ("topic_replica_min", C.c_int32),
                ("num_brokers", C.c_int32), ("num_replicas_in_cluster", C.c_int32),
                ("num_partitions_with_offline_replicas", C.c_int32), ("num_topics", C.c_int32),
                ("num_unbalanced_disks", C.c_int32), ("disk_utilization_std", C.c_double)]


class ProvisionRecStruct(C.Structure):
    _fields_ = [("status", C.c_int32), ("num_brokers", C.c_int32), ("num_racks", C.c_int32), ("num_disks", C.c_int32),
                ("num_partitions", C.c_int32), ("typical_broker_id", C.c_int32), ("resource", C.c_int32),
                ("pad", C.c_int32), ("typical_broker_capacity", C.c_double), ("total_capacity", C.c_double)]


class ProvisionRespStruct(C.Structure):
    _fields_ = [("status", C.c_int32), ("has_recommendation", C.c_int32), ("recommendation", ProvisionRecStruct)]


class GoalResultStruct(C.Structure):
    _fields_ = [("goal_kind", C.c_int32), ("succeeded", C.c_int32), ("has_diff", C.c_int32), ("seconds", C.c_double),
                ("candidates", C.c_int64), ("device_candidates", C.c_int64), ("device_launches", C.c_int64),
                ("actions", C.c_int64), ("stats", StatsStruct), ("provision", ProvisionRespStruct)]


class RandomClusterProps(C.Structure):
    _fields_ = [("num_racks", C.c_int32), ("num_brokers", C.c_int32), ("num_dead_brokers", C.c_int32),
                ("num_brokers_with_bad_disk", C.c_int32), ("num_replicas", C.c_int32), ("num_topics", C.c_int32),
                ("min_replication", C.c_int32), ("max_replication", C.c_int32), ("mean_cpu", C.c_double),
                ("mean_disk", C.c_double), ("mean_nw_in", C.c_double), ("mean_nw_out", C.c_double),
                ("distribution", C.c_int32), ("rack_aware", C.c_int32), ("leader_in_first_position", C.c_int32),
                ("jbod", C.c_int32), ("num_logdirs", C.c_int32), ("logdir_capacity", C.c_double * 8)]


class PerfStruct(C.Structure):
    _fields_ = [("scan_launches", C.c_int64), ("scan_kernel_ms", C.c_double), ("scan_bytes", C.c_int64),
                ("stats_launches", C.c_int64), ("stats_kernel_ms", C.c_double), ("stats_bytes", C.c_int64),
                ("host_syncs", C.c_int64), ("scan_required", C.c_int64), ("chain_launches", C.c_int64),
                ("intra_launches", C.c_int64), ("intra_kernel_ms", C.c_double), ("intra_bytes", C.c_int64),
                ("cross_launches", C.c_int64), ("cross_required", C.c_int64), ("cross_kernel_ms", C.c_double),
                ("combines", C.c_int64), ("server_launches", C.c_int64), ("server_scans", C.c_int64),
                ("server_required", C.c_int64), ("server_busy_ms", C.c_double),
                ("server_payload_bytes", C.c_int64), ("server_chains", C.c_int64),
                ("server_idle_exits", C.c_int64), ("server_resident_ms", C.c_double),
                ("intra_sort_launches", C.c_int64), ("intra_sort_ms", C.c_double),
                ("accept_launches", C.c_int64), ("accept_cells", C.c_int64), ("accept_kernel_ms", C.c_double)]


class HostPrefixPerfStruct(C.Structure):  # ccmi_host_prefix_counters
    _fields_ = [("host_scans", C.c_int64), ("host_candidates", C.c_int64)]


class HostCrossPerfStruct(C.Structure):  # ccmi_host_cross_counters
    _fields_ = [("host_cross_scans", C.c_int64), ("host_cross_candidates", C.c_int64)]


class BasicStatsStruct(C.Structure):  # ccmi_basic_stats: one broker's or one host's BasicStats, 128 bytes
    _fields_ = [("disk_mb", C.c_double), ("disk_pct", C.c_double), ("cpu_pct", C.c_double),
                ("leader_nw_in_rate", C.c_double), ("follower_nw_in_rate", C.c_double), ("nw_out_rate", C.c_double),
                ("pnw_out_rate", C.c_double), ("disk_capacity_mb", C.c_double), ("network_in_capacity", C.c_double),
                ("network_out_capacity", C.c_double), ("num_core", C.c_double),
                ("replicas", C.c_int32), ("leaders", C.c_int32), ("broker", C.c_int32), ("state", C.c_int32),
                ("host", C.c_int32), ("rack", C.c_int32), ("reserved", C.c_int32 * 4)]


class DiskStatsStruct(C.Structure):  # ccmi_disk_stats: one disk's DiskStats, 40 bytes
    _fields_ = [("disk_mb", C.c_double), ("disk_pct", C.c_double), ("capacity", C.c_double),
                ("num_replicas", C.c_int32), ("num_leader_replicas", C.c_int32), ("disk", C.c_int32),
                ("broker", C.c_int32)]


class PartitionLoadQueryStruct(C.Structure):  # ccmi_partition_load_query, 64 bytes
    _fields_ = [("resource", C.c_int32), ("want_max_load", C.c_int32), ("want_avg_load", C.c_int32),
                ("entries", C.c_int32), ("partition_lower", C.c_int32), ("partition_upper", C.c_int32),
                ("reserved", C.c_int32 * 4), ("topic_selected", C.POINTER(C.c_uint8)),
                ("broker_selected", C.POINTER(C.c_uint8)), ("tie_rank", C.POINTER(C.c_int32))]


class PartitionLoadRecordStruct(C.Structure):  # ccmi_partition_load_record, 80 bytes
    _fields_ = [("util", C.c_double * 4), ("partition", C.c_int32), ("num_replicas", C.c_int32),
                ("brokers", C.c_int32 * 8), ("reserved", C.c_int32 * 2)]


class ProposalRecordStruct(C.Structure):  # ccmi_proposal_record, 160 bytes
    _fields_ = [("partition", C.c_int32), ("size", C.c_int32), ("old_leader", C.c_int32),
                ("old_leader_disk", C.c_int32), ("num_replicas", C.c_int32), ("flags", C.c_int32),
                ("num_to_add", C.c_int32), ("num_between_disks", C.c_int32),
                ("old_replicas", C.c_int32 * 8), ("new_replicas", C.c_int32 * 8),
                ("old_disks", C.c_int32 * 8), ("new_disks", C.c_int32 * 8)]


class ProposalSummaryStruct(C.Structure):  # ccmi_proposal_summary, 64 bytes
    _fields_ = [("num_proposals", C.c_int64), ("num_inter_broker_replica_movements", C.c_int64),
                ("inter_broker_data_to_move_mb", C.c_int64), ("num_intra_broker_replica_movements", C.c_int64),
                ("intra_broker_data_to_move_mb", C.c_int64), ("num_leadership_movements", C.c_int64),
                ("reserved", C.c_int64 * 2)]


class SortedReplicasQueryStruct(C.Structure):  # ccmi_sorted_replicas_query, 64 bytes
    _fields_ = [("select_mask", C.c_int32), ("num_priorities", C.c_int32), ("priorities", C.c_int32 * 2),
                ("score_resource", C.c_int32), ("score_reverse", C.c_int32), ("above_resource", C.c_int32),
                ("below_resource", C.c_int32), ("above_limit", C.c_double), ("below_limit", C.c_double),
                ("topic_excluded", C.POINTER(C.c_uint8)), ("topic_included", C.POINTER(C.c_uint8))]


class ExecutionPlanQueryStruct(C.Structure):  # ccmi_execution_plan_query, 64 bytes
    _fields_ = [("num_strategies", C.c_int32), ("strategies", C.c_int32 * 4), ("reserved", C.c_int32 * 7),
                ("proposal_rank", C.POINTER(C.c_int32)), ("partition_state", C.POINTER(C.c_uint8))]


class PlanTaskStruct(C.Structure):  # ccmi_plan_task, 16 bytes
    _fields_ = [("partition", C.c_int32), ("num_to_add", C.c_int32), ("data_to_move_mb", C.c_int64)]


class PlanSummaryStruct(C.Structure):  # ccmi_plan_summary, 64 bytes
    _fields_ = [("num_inter_tasks", C.c_int64), ("num_inter_entries", C.c_int64), ("num_intra_tasks", C.c_int64),
                ("num_leader_tasks", C.c_int64), ("num_brokers_with_tasks", C.c_int64), ("size_overflow", C.c_int64),
                ("mingled", C.c_int64), ("reserved", C.c_int64)]


class QueueProbeArgsStruct(C.Structure):  # ccmi_queue_probe_args (csrc/ccmi_session.h: diagnostics, not in the ABI)
    _fields_ = [("sel_leaders", C.c_int32), ("score_res", C.c_int32), ("score_reverse", C.c_int32),
                ("prio_offline", C.c_int32), ("prio_immigrants", C.c_int32), ("sel_excl_topics", C.c_int32),
                ("self_kind", C.c_int32), ("num_accept", C.c_int32), ("accept_kinds", C.POINTER(C.c_int32)),
                ("head", C.c_int32), ("has_skip", C.c_int32), ("skip_key", C.c_uint64),
                ("tail", C.POINTER(C.c_int32)), ("n_tail", C.c_int32), ("cands", C.POINTER(C.c_int32)),
                ("n_cands", C.c_int32), ("mode", C.c_int32)]


class QueueProbeReportStruct(C.Structure):  # ccmi_queue_probe_report
    _fields_ = [(f, C.c_int32) for f in (
        "dev_entry", "dev_replica", "dev_column", "ref_entry", "ref_replica", "ref_column", "served", "keyed", "stride",
        "n_active", "audit", "audited", "win_slot", "accepted_rows", "lowest_accepted_slot", "highest_accepted_slot",
        "win_len", "win_rank", "head_masked", "pad")] + [("win_key", C.c_uint64)]


class AggregatorConfigStruct(C.Structure):  # ccmi_aggregator_config, 32 bytes
    _fields_ = [("window_ms", C.c_int64), ("num_windows", C.c_int32), ("min_samples_per_window", C.c_int32),
                ("num_metrics", C.c_int32), ("num_entities", C.c_int32), ("num_groups", C.c_int32),
                ("reserved", C.c_int32)]


class AggregatorStateStruct(C.Structure):  # ccmi_aggregator_state, 48 bytes
    _fields_ = [("generation", C.c_int64), ("oldest_window_index", C.c_int64), ("current_window_index", C.c_int64),
                ("num_samples", C.c_int64), ("num_present_entities", C.c_int64),
                ("num_available_windows", C.c_int32), ("reserved", C.c_int32)]


class AggregationOptionsStruct(C.Structure):  # ccmi_aggregation_options, 32 bytes
    _fields_ = [("min_valid_entity_ratio", C.c_double), ("min_valid_entity_group_ratio", C.c_double),
                ("min_valid_windows", C.c_int32), ("max_allowed_extrapolations_per_entity", C.c_int32),
                ("granularity", C.c_int32), ("include_invalid_entities", C.c_int32)]


class AggregatorCompletenessStruct(C.Structure):  # ccmi_aggregator_completeness, 96 bytes
    _fields_ = [("generation", C.c_int64), ("num_windows", C.c_int32), ("num_valid_windows", C.c_int32),
                ("failure", C.c_int32), ("window_capacity", C.c_int32),
                ("num_interested_entities", C.c_int32), ("num_interested_groups", C.c_int32),
                ("num_valid_entities", C.c_int32), ("num_valid_groups", C.c_int32),
                ("valid_entity_ratio", C.c_float), ("valid_entity_group_ratio", C.c_float),
                ("window_index", C.POINTER(C.c_int64)), ("window_included", C.POINTER(C.c_uint8)),
                ("valid_entity_ratio_by_window", C.POINTER(C.c_float)),
                ("valid_entity_ratio_with_group_granularity_by_window", C.POINTER(C.c_float)),
                ("valid_entity_group_ratio_by_window", C.POINTER(C.c_float)),
                ("extrapolated_entity_ratio_by_window", C.POINTER(C.c_float))]


class PartitionTopologyStruct(C.Structure):  # ccmi_partition_topology, 88 bytes
    _fields_ = [("num_partitions", C.c_int32), ("num_topics", C.c_int32), ("num_logdirs", C.c_int32),
                ("reserved", C.c_int32), ("topic_names", C.POINTER(C.c_char_p)),
                ("partition_topic", C.POINTER(C.c_int32)), ("partition_number", C.POINTER(C.c_int32)),
                ("replica_offset", C.POINTER(C.c_int32)), ("replica_broker_id", C.POINTER(C.c_int32)),
                ("leader_broker_id", C.POINTER(C.c_int32)), ("replica_offline", C.POINTER(C.c_uint8)),
                ("replica_logdir", C.POINTER(C.c_int32)), ("logdir_names", C.POINTER(C.c_char_p))]


class MetricAnomalyConfigStruct(C.Structure):  # ccmi_metric_anomaly_config, 32 bytes
    _fields_ = [("upper_percentile", C.c_double), ("lower_percentile", C.c_double), ("upper_margin", C.c_double),
                ("lower_margin", C.c_double)]


class MetricAnomalyStruct(C.Structure):  # ccmi_metric_anomaly, 32 bytes
    _fields_ = [("entity", C.c_int32), ("metric", C.c_int32), ("current", C.c_double),
                ("upper_threshold", C.c_double), ("lower_threshold", C.c_double)]


class SlowBrokerConfigStruct(C.Structure):  # ccmi_slow_broker_config, 80 bytes
    _fields_ = [("bytes_in_rate_detection_threshold", C.c_double), ("log_flush_time_threshold_ms", C.c_double),
                ("metric_history_percentile", C.c_double), ("metric_history_margin", C.c_double),
                ("peer_metric_percentile", C.c_double), ("peer_metric_margin", C.c_double),
                ("self_healing_unfixable_ratio", C.c_double), ("demotion_score", C.c_int32),
                ("decommission_score", C.c_int32), ("log_flush_metric", C.c_int32),
                ("leader_bytes_in_metric", C.c_int32), ("replication_bytes_in_metric", C.c_int32),
                ("removal_enabled", C.c_int32)]


class SlowBrokerSummaryStruct(C.Structure):  # ccmi_slow_broker_summary, 72 bytes
    _fields_ = [("current_window_index", C.c_int64), ("peer_base_log_flush", C.c_double),
                ("peer_base_per_byte", C.c_double), ("num_current", C.c_int32), ("num_skipped", C.c_int32),
                ("num_active", C.c_int32), ("cluster_size", C.c_int32), ("num_persistent", C.c_int32),
                ("num_recent", C.c_int32), ("num_suspect", C.c_int32), ("num_to_demote", C.c_int32),
                ("num_to_remove", C.c_int32), ("unfixable", C.c_int32), ("removal_enabled", C.c_int32),
                ("reserved", C.c_int32)]


class SlowBrokerStruct(C.Structure):  # ccmi_slow_broker, 24 bytes
    _fields_ = [("entity", C.c_int32), ("kind", C.c_int32), ("score", C.c_int32), ("reserved", C.c_int32),
                ("since_ms", C.c_int64)]


class MetricsProcessorConfigStruct(C.Structure):  # ccmi_metrics_processor_config, 32 bytes
    _fields_ = [("cpu_weight_of_leader_bytes_in_rate", C.c_double), ("cpu_weight_of_leader_bytes_out_rate", C.c_double),
                ("cpu_weight_of_follower_bytes_in_rate", C.c_double), ("reserved", C.c_int64)]


class RawMetricsStruct(C.Structure):  # ccmi_raw_metrics, 72 bytes
    _fields_ = [("n", C.c_int64), ("num_topics", C.c_int32), ("reserved", C.c_int32),
                ("topic_names", C.POINTER(C.c_char_p)), ("type", C.c_void_p), ("broker_id", C.c_void_p),
                ("time_ms", C.c_void_p), ("value", C.c_void_p), ("topic", C.c_void_p), ("partition", C.c_void_p)]


class ClusterNodesStruct(C.Structure):  # ccmi_cluster_nodes, 24 bytes
    _fields_ = [("num_nodes", C.c_int32), ("reserved", C.c_int32), ("broker_id", C.c_void_p),
                ("num_cores", C.c_void_p)]


class ProcessedSamplesStruct(C.Structure):  # ccmi_processed_samples, 120 bytes
    _fields_ = [("max_metric_timestamp", C.c_int64), ("partition_capacity", C.c_int64),
                ("num_partition_samples", C.c_int64), ("partition_entity", C.c_void_p),
                ("partition_values", C.c_void_p), ("broker_capacity", C.c_int64), ("num_broker_samples", C.c_int64),
                ("broker_node", C.c_void_p), ("broker_values", C.c_void_p), ("broker_version", C.c_void_p),
                ("partition_skip", C.c_void_p), ("broker_skip", C.c_void_p), ("skipped_by_node", C.c_void_p),
                ("num_skipped_brokers", C.c_int32), ("num_hash_fallback_brokers", C.c_int32),
                ("num_dropped_records", C.c_int64)]


METRICS_PROCESSOR_SYMBOLS = ("ccmi_metrics_processor_create", "ccmi_metrics_processor_destroy",
                             "ccmi_metrics_processor_add_metrics", "ccmi_metrics_processor_process",
                             "ccmi_metrics_processor_process_into", "ccmi_metrics_processor_cached_num_cores", "ccmi_metrics_processor_clear")
# RawMetricType in id order (cruise-control-metrics-reporter, RawMetricType.java); index = id
RAW_METRIC_TYPES = (
    "ALL_TOPIC_BYTES_IN", "ALL_TOPIC_BYTES_OUT", "TOPIC_BYTES_IN", "TOPIC_BYTES_OUT", "PARTITION_SIZE",
    "BROKER_CPU_UTIL", "ALL_TOPIC_REPLICATION_BYTES_IN", "ALL_TOPIC_REPLICATION_BYTES_OUT",
    "ALL_TOPIC_PRODUCE_REQUEST_RATE", "ALL_TOPIC_FETCH_REQUEST_RATE", "ALL_TOPIC_MESSAGES_IN_PER_SEC",
    "TOPIC_REPLICATION_BYTES_IN", "TOPIC_REPLICATION_BYTES_OUT", "TOPIC_PRODUCE_REQUEST_RATE",
    "TOPIC_FETCH_REQUEST_RATE", "TOPIC_MESSAGES_IN_PER_SEC", "BROKER_PRODUCE_REQUEST_RATE",
    "BROKER_CONSUMER_FETCH_REQUEST_RATE", "BROKER_FOLLOWER_FETCH_REQUEST_RATE",
    "BROKER_REQUEST_HANDLER_AVG_IDLE_PERCENT", "BROKER_REQUEST_QUEUE_SIZE", "BROKER_RESPONSE_QUEUE_SIZE",
    "BROKER_PRODUCE_REQUEST_QUEUE_TIME_MS_MAX", "BROKER_PRODUCE_REQUEST_QUEUE_TIME_MS_MEAN",
    "BROKER_CONSUMER_FETCH_REQUEST_QUEUE_TIME_MS_MAX", "BROKER_CONSUMER_FETCH_REQUEST_QUEUE_TIME_MS_MEAN",
    "BROKER_FOLLOWER_FETCH_REQUEST_QUEUE_TIME_MS_MAX", "BROKER_FOLLOWER_FETCH_REQUEST_QUEUE_TIME_MS_MEAN",
    "BROKER_PRODUCE_TOTAL_TIME_MS_MAX", "BROKER_PRODUCE_TOTAL_TIME_MS_MEAN",
    "BROKER_CONSUMER_FETCH_TOTAL_TIME_MS_MAX", "BROKER_CONSUMER_FETCH_TOTAL_TIME_MS_MEAN",
    "BROKER_FOLLOWER_FETCH_TOTAL_TIME_MS_MAX", "BROKER_FOLLOWER_FETCH_TOTAL_TIME_MS_MEAN",
    "BROKER_PRODUCE_LOCAL_TIME_MS_MAX", "BROKER_PRODUCE_LOCAL_TIME_MS_MEAN",
    "BROKER_CONSUMER_FETCH_LOCAL_TIME_MS_MAX", "BROKER_CONSUMER_FETCH_LOCAL_TIME_MS_MEAN",
    "BROKER_FOLLOWER_FETCH_LOCAL_TIME_MS_MAX", "BROKER_FOLLOWER_FETCH_LOCAL_TIME_MS_MEAN",
    "BROKER_LOG_FLUSH_RATE", "BROKER_LOG_FLUSH_TIME_MS_MAX", "BROKER_LOG_FLUSH_TIME_MS_MEAN",
    "BROKER_PRODUCE_REQUEST_QUEUE_TIME_MS_50TH", "BROKER_PRODUCE_REQUEST_QUEUE_TIME_MS_999TH",
    "BROKER_CONSUMER_FETCH_REQUEST_QUEUE_TIME_MS_50TH", "BROKER_CONSUMER_FETCH_REQUEST_QUEUE_TIME_MS_999TH",
    "BROKER_FOLLOWER_FETCH_REQUEST_QUEUE_TIME_MS_50TH", "BROKER_FOLLOWER_FETCH_REQUEST_QUEUE_TIME_MS_999TH",
    "BROKER_PRODUCE_TOTAL_TIME_MS_50TH", "BROKER_PRODUCE_TOTAL_TIME_MS_999TH",
    "BROKER_CONSUMER_FETCH_TOTAL_TIME_MS_50TH", "BROKER_CONSUMER_FETCH_TOTAL_TIME_MS_999TH",
    "BROKER_FOLLOWER_FETCH_TOTAL_TIME_MS_50TH", "BROKER_FOLLOWER_FETCH_TOTAL_TIME_MS_999TH",
    "BROKER_PRODUCE_LOCAL_TIME_MS_50TH", "BROKER_PRODUCE_LOCAL_TIME_MS_999TH",
    "BROKER_CONSUMER_FETCH_LOCAL_TIME_MS_50TH", "BROKER_CONSUMER_FETCH_LOCAL_TIME_MS_999TH",
    "BROKER_FOLLOWER_FETCH_LOCAL_TIME_MS_50TH", "BROKER_FOLLOWER_FETCH_LOCAL_TIME_MS_999TH",
    "BROKER_LOG_FLUSH_TIME_MS_50TH", "BROKER_LOG_FLUSH_TIME_MS_999TH")
RAW_METRIC_TYPE_ID = {name: i for i, name in enumerate(RAW_METRIC_TYPES)}
(SAMPLING_ALL, SAMPLING_BROKER_METRICS_ONLY, SAMPLING_PARTITION_METRICS_ONLY,
 SAMPLING_ONGOING_EXECUTION) = range(4)  # ccmi_sampling_mode

SLOW_BROKER_DEMOTE, SLOW_BROKER_REMOVE = 1, 2  # ccmi_slow_broker.kind
# CCMI_SLOW_DIAG_*: the bits of ccmi_slow_broker_finder_detect's per-entity diagnostic byte
(SLOW_DIAG_SKIPPED, SLOW_DIAG_FLUSH_HISTORY, SLOW_DIAG_FLUSH_PEERS, SLOW_DIAG_PER_BYTE_HISTORY,
 SLOW_DIAG_PER_BYTE_PEERS, SLOW_DIAG_OVER_THRESHOLD, SLOW_DIAG_SUSPECT) = 1, 2, 4, 8, 16, 32, 64
ANOMALY_SYMBOLS = ("ccmi_aggregator_metric_anomalies", "ccmi_slow_broker_finder_create",
                   "ccmi_slow_broker_finder_destroy", "ccmi_slow_broker_finder_detect",
                   "ccmi_slow_broker_finder_scores", "ccmi_slow_broker_finder_reset")

# ccmi_aggregation_function, ccmi_extrapolation (Extrapolation.java order), ccmi_granularity, ccmi_aggregation_failure
AGG_AVG, AGG_MAX, AGG_LATEST = range(3)
EXTRAPOLATIONS = ("NONE", "AVG_AVAILABLE", "AVG_ADJACENT", "FORCED_INSUFFICIENT", "NO_VALID_EXTRAPOLATION")
GRANULARITY_ENTITY, GRANULARITY_ENTITY_GROUP = 0, 1
AGG_FAILURE_NONE, AGG_FAILURE_NO_WINDOW_IN_RANGE, AGG_FAILURE_NOT_ENOUGH_VALID_WINDOWS = range(3)
# KafkaMetricDef's common metrics in id order with their aggregation functions (KafkaMetricDef.java:43-53): the metric
# set of a partition aggregator, and where the six metrics of ccmi_builder_populate_partition sit in it
KAFKA_COMMON_METRICS = (("CPU_USAGE", AGG_AVG), ("DISK_USAGE", AGG_LATEST), ("LEADER_BYTES_IN", AGG_AVG),
                        ("LEADER_BYTES_OUT", AGG_AVG), ("PRODUCE_RATE", AGG_AVG), ("FETCH_RATE", AGG_AVG),
                        ("MESSAGE_IN_RATE", AGG_AVG), ("REPLICATION_BYTES_IN_RATE", AGG_AVG),
                        ("REPLICATION_BYTES_OUT_RATE", AGG_AVG))


# CCMI_SEL_* (ReplicaSortFunctionFactory's selection functions) and CCMI_PRIO_* (its priority functions)
SEL_LEADERS, SEL_FOLLOWERS, SEL_ONLINE, SEL_OFFLINE, SEL_IMMIGRANTS, SEL_IMMIGRANT_OR_OFFLINE = 1, 2, 4, 8, 16, 32
SORT_PRIORITIES = ("offline", "immigrants")  # index = CCMI_PRIO_*
# CCMI_STRATEGY_* (index = value; the simple names of the executor/strategy classes) and CCMI_PSTATE_*
MOVEMENT_STRATEGIES = ("BaseReplicaMovementStrategy", "PrioritizeLargeReplicaMovementStrategy",
                       "PrioritizeSmallReplicaMovementStrategy", "PostponeUrpReplicaMovementStrategy",
                       "PrioritizeMinIsrWithOfflineReplicasStrategy",
                       "PrioritizeOneAboveMinIsrWithOfflineReplicasStrategy")
(STRATEGY_BASE, STRATEGY_PRIORITIZE_LARGE, STRATEGY_PRIORITIZE_SMALL, STRATEGY_POSTPONE_URP,
 STRATEGY_PRIORITIZE_MIN_ISR_WITH_OFFLINE, STRATEGY_PRIORITIZE_ONE_ABOVE_MIN_ISR_WITH_OFFLINE) = range(6)
PSTATE_UNDER_REPLICATED, PSTATE_UNDER_MIN_ISR, PSTATE_AT_MIN_ISR, PSTATE_ONE_ABOVE_MIN_ISR = 1, 2, 4, 8


# ----------------------------------------------------------------------------------------------- errors
class CruiseControlError(RuntimeError):
    pass


class OptimizationFailureException(CruiseControlError):
    pass


class IllegalStateException(CruiseControlError):
    pass


class IllegalArgumentException(CruiseControlError):
    pass


class UnsupportedOperationException(CruiseControlError):
    pass


class DeviceError(CruiseControlError):
    pass


_STATUS = {1: IllegalArgumentException, 2: DeviceError, 3: OptimizationFailureException, 4: IllegalStateException,
           5: UnsupportedOperationException}

ABI_VERSION = 13  # CCMI_ABI_VERSION of include/ccmi.h
EXPORTED_SYMBOLS = (
    "ccmi_last_error", "ccmi_abi_version", "ccmi_device_count", "ccmi_default_constraint", "ccmi_default_random_cluster_props",
    "ccmi_random_cluster", "ccmi_cluster_buffers_desc", "ccmi_cluster_buffers_free", "ccmi_session_create",
    "ccmi_session_destroy", "ccmi_optimizations", "ccmi_goal_optimize", "ccmi_action_acceptance",
    "ccmi_action_acceptance_by_kind", "ccmi_actions_acceptance", "ccmi_moves_acceptance_mask", "ccmi_swaps_acceptance_grid",
    "ccmi_session_apply", "ccmi_session_mark_disks_for_removal", "ccmi_last_failure_provision",
    "ccmi_compute_cluster_stats", "ccmi_broker_stats", "ccmi_partition_load", "ccmi_action_log_count", "ccmi_action_log_copy", "ccmi_replica_distribution",
    "ccmi_leader_distribution", "ccmi_replica_disks", "ccmi_proposal_count", "ccmi_proposals",
    "ccmi_proposal_disks", "ccmi_proposal_diff", "ccmi_sorted_replicas", "ccmi_execution_plan", "ccmi_perf", "ccmi_perf_reset", "ccmi_host_prefix_perf", "ccmi_host_cross_perf",
    "ccmi_set_kernel_timing", "ccmi_session_set_shard", "ccmi_rccl_unique_id", "ccmi_session_attach_rccl",
    "ccmi_session_attach_shm", "ccmi_session_attach_shm_job", "ccmi_shard_group_create", "ccmi_shard_group_destroy", "ccmi_session_attach_group",
    "ccmi_topic_broker_set",
    "ccmi_builder_create", "ccmi_builder_destroy", "ccmi_builder_create_broker", "ccmi_builder_add_disk",
    "ccmi_builder_populate_partition", "ccmi_builder_set_broker_state", "ccmi_builder_set_disk_state",
    "ccmi_builder_desc", "ccmi_builder_broker_ids",
    "ccmi_aggregator_create", "ccmi_aggregator_destroy", "ccmi_aggregator_add_samples", "ccmi_aggregator_state_query",
    "ccmi_aggregator_completeness_query", "ccmi_aggregator_aggregate", "ccmi_aggregator_peek_current_window",
    "ccmi_aggregator_remove_entities", "ccmi_aggregator_clear", "ccmi_builder_populate_from_aggregator",
    "ccmi_aggregator_metric_anomalies", "ccmi_slow_broker_finder_create", "ccmi_slow_broker_finder_destroy",
    "ccmi_slow_broker_finder_detect", "ccmi_slow_broker_finder_scores", "ccmi_slow_broker_finder_reset",
    "ccmi_metrics_processor_create", "ccmi_metrics_processor_destroy", "ccmi_metrics_processor_add_metrics",
    "ccmi_metrics_processor_process", "ccmi_metrics_processor_process_into", "ccmi_metrics_processor_cached_num_cores",
    "ccmi_metrics_processor_clear")

# int (*)(void* ctx, int64_t* key): replace *key by the MIN over all shards, return 0 (include/ccmi.h)
AllreduceMinFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64))


class Library:
    """Loaded libccmi.so (or, in CPU tests only, the emulation build from tests/emu)."""

    _cache: Dict[str, "Library"] = {}

    def __init__(self, path: str = DEFAULT_LIB):
        if not os.path.exists(path):
            raise DeviceError(f"{path} not found: build it with __graft_entry__.build() (no CPU fallback exists)")
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        if L.ccmi_abi_version() != ABI_VERSION:  # the struct layouts below are ABI_VERSION's (include/ccmi.h)
            raise DeviceError(f"{path} has ABI {L.ccmi_abi_version()}, this binding needs {ABI_VERSION}: rebuild it")
        L.ccmi_last_error.restype = C.c_char_p
        L.ccmi_random_cluster.argtypes = [C.POINTER(RandomClusterProps), C.POINTER(C.c_void_p)]
        L.ccmi_cluster_buffers_desc.restype = C.POINTER(ClusterDesc)
        L.ccmi_cluster_buffers_desc.argtypes = [C.c_void_p]
        L.ccmi_cluster_buffers_free.argtypes = [C.c_void_p]
        L.ccmi_session_create.argtypes = [C.c_int32, C.POINTER(ClusterDesc), C.POINTER(C.c_void_p)]
        L.ccmi_session_destroy.argtypes = [C.c_void_p]
        L.ccmi_optimizations.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(ConstraintStruct),
                                         C.POINTER(OptionsStruct), C.POINTER(GoalResultStruct)]
        L.ccmi_goal_optimize.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                         C.POINTER(ConstraintStruct), C.POINTER(OptionsStruct),
                                         C.POINTER(GoalResultStruct)]
        L.ccmi_action_acceptance.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ActionStruct), C.POINTER(C.c_int32)]
        L.ccmi_action_acceptance_by_kind.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ActionStruct),
                                                     C.POINTER(C.c_int32)]
        # the batched call runs on the device only: the CPU tests' emulation build reports the same ABI without it
        self.has_actions_acceptance = hasattr(L, "ccmi_actions_acceptance")
        if self.has_actions_acceptance:
            L.ccmi_actions_acceptance.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(ActionStruct),
                                                  C.c_int64, C.POINTER(C.c_int8), C.POINTER(C.c_int64)]
        self.has_moves_acceptance_mask = hasattr(L, "ccmi_moves_acceptance_mask")
        if self.has_moves_acceptance_mask:
            L.ccmi_moves_acceptance_mask.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int64,
                                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
        self.has_swaps_acceptance_grid = hasattr(L, "ccmi_swaps_acceptance_grid")
        if self.has_swaps_acceptance_grid:
            L.ccmi_swaps_acceptance_grid.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int64,
                                                     C.c_void_p, C.c_int64, C.POINTER(C.c_int8), C.POINTER(C.c_int64)]
        self.has_broker_stats = hasattr(L, "ccmi_broker_stats")
        if self.has_broker_stats:
            L.ccmi_broker_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
        self.has_host_prefix_perf = hasattr(L, "ccmi_host_prefix_perf")
        if self.has_host_prefix_perf:
            L.ccmi_host_prefix_perf.argtypes = [C.c_void_p, C.POINTER(HostPrefixPerfStruct)]
        self.has_host_cross_perf = hasattr(L, "ccmi_host_cross_perf")
        if self.has_host_cross_perf:
            L.ccmi_host_cross_perf.argtypes = [C.c_void_p, C.POINTER(HostCrossPerfStruct)]
        self.has_partition_load = hasattr(L, "ccmi_partition_load")
        if self.has_partition_load:
            L.ccmi_partition_load.argtypes = [C.c_void_p, C.POINTER(PartitionLoadQueryStruct), C.c_void_p,
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self.has_proposal_diff = hasattr(L, "ccmi_proposal_diff")
        if self.has_proposal_diff:
            L.ccmi_proposal_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                             C.POINTER(ProposalSummaryStruct)]
        self.has_sorted_replicas = hasattr(L, "ccmi_sorted_replicas")
        if self.has_sorted_replicas:
            L.ccmi_sorted_replicas.argtypes = [C.c_void_p, C.POINTER(SortedReplicasQueryStruct), C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int64)]
        self.has_execution_plan = hasattr(L, "ccmi_execution_plan")
        if self.has_execution_plan:
            L.ccmi_execution_plan.argtypes = [C.c_void_p, C.POINTER(ExecutionPlanQueryStruct),
                                              C.POINTER(PlanSummaryStruct), C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_int64]
        # MetricSampleAggregator on the device: all nine symbols or none
        self.has_aggregator = hasattr(L, "ccmi_aggregator_create")
        if self.has_aggregator:
            L.ccmi_aggregator_create.argtypes = [C.c_int32, C.POINTER(AggregatorConfigStruct), C.c_void_p, C.c_void_p,
                                                 C.POINTER(C.c_void_p)]
            L.ccmi_aggregator_destroy.argtypes = [C.c_void_p]
            L.ccmi_aggregator_destroy.restype = None
            L.ccmi_aggregator_add_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                      C.c_void_p, C.POINTER(C.c_int64)]
            L.ccmi_aggregator_state_query.argtypes = [C.c_void_p, C.POINTER(AggregatorStateStruct)]
            L.ccmi_aggregator_completeness_query.argtypes = [C.c_void_p, C.c_int64, C.c_int64,
                                                             C.POINTER(AggregationOptionsStruct), C.c_void_p,
                                                             C.POINTER(AggregatorCompletenessStruct), C.c_void_p,
                                                             C.c_void_p]
            L.ccmi_aggregator_aggregate.argtypes = [C.c_void_p, C.c_int64, C.c_int64,
                                                    C.POINTER(AggregationOptionsStruct), C.c_void_p,
                                                    C.POINTER(AggregatorCompletenessStruct), C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            L.ccmi_aggregator_peek_current_window.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                              C.POINTER(C.c_int64)]
            L.ccmi_aggregator_remove_entities.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
            L.ccmi_aggregator_clear.argtypes = [C.c_void_p]
        # the metric anomaly finders over an aggregator's device rows (K19): all six symbols or none, device only
        self.has_metric_anomalies = hasattr(L, "ccmi_aggregator_metric_anomalies")
        if self.has_metric_anomalies:
            L.ccmi_aggregator_metric_anomalies.argtypes = [
                C.c_void_p, C.c_int64, C.c_int64, C.POINTER(AggregationOptionsStruct), C.c_void_p,
                C.POINTER(MetricAnomalyConfigStruct), C.c_void_p, C.POINTER(AggregatorCompletenessStruct),
                C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            L.ccmi_slow_broker_finder_create.argtypes = [C.c_void_p, C.POINTER(SlowBrokerConfigStruct),
                                                         C.POINTER(C.c_void_p)]
            L.ccmi_slow_broker_finder_destroy.argtypes = [C.c_void_p]
            L.ccmi_slow_broker_finder_destroy.restype = None
            L.ccmi_slow_broker_finder_detect.argtypes = [
                C.c_void_p, C.c_int64, C.c_int64, C.POINTER(AggregationOptionsStruct), C.c_void_p, C.c_int64,
                C.POINTER(AggregatorCompletenessStruct), C.POINTER(SlowBrokerSummaryStruct), C.c_void_p, C.c_int64,
                C.POINTER(C.c_int64), C.c_void_p]
            L.ccmi_slow_broker_finder_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            L.ccmi_slow_broker_finder_reset.argtypes = [C.c_void_p]
        # LoadMonitor.clusterModel's bulk load from an aggregator's device rows (K18): device only as well
        self.has_metrics_processor = hasattr(L, "ccmi_metrics_processor_create")
        if self.has_metrics_processor:
            L.ccmi_metrics_processor_create.argtypes = [C.c_int32, C.POINTER(MetricsProcessorConfigStruct),
                                                        C.POINTER(C.c_void_p)]
            L.ccmi_metrics_processor_destroy.argtypes = [C.c_void_p]
            L.ccmi_metrics_processor_destroy.restype = None
            L.ccmi_metrics_processor_add_metrics.argtypes = [C.c_void_p, C.POINTER(RawMetricsStruct)]
            L.ccmi_metrics_processor_process.argtypes = [C.c_void_p, C.POINTER(PartitionTopologyStruct),
                                                         C.POINTER(ClusterNodesStruct), C.c_void_p, C.c_int32,
                                                         C.POINTER(ProcessedSamplesStruct)]
            L.ccmi_metrics_processor_process_into.argtypes = [C.c_void_p, C.POINTER(PartitionTopologyStruct),
                                                              C.POINTER(ClusterNodesStruct), C.c_void_p, C.c_int32,
                                                              C.c_void_p, C.c_void_p, C.POINTER(ProcessedSamplesStruct)]
            L.ccmi_metrics_processor_cached_num_cores.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
            L.ccmi_metrics_processor_clear.argtypes = [C.c_void_p]
        self.has_load_model = hasattr(L, "ccmi_builder_populate_from_aggregator")
        if self.has_load_model:
            L.ccmi_builder_populate_from_aggregator.argtypes = [
                C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(AggregationOptionsStruct), C.c_void_p,
                C.POINTER(C.c_int32), C.POINTER(PartitionTopologyStruct), C.POINTER(AggregatorCompletenessStruct),
                C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            if hasattr(L, "ccmi_load_model_timing"):  # diagnostics, outside the ABI (csrc/ccmi_load_model.cpp)
                L.ccmi_load_model_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.ccmi_session_apply.argtypes = [C.c_void_p, C.POINTER(ActionStruct), C.c_int64, C.POINTER(C.c_int64)]
        # diagnostics, outside the ABI (csrc/ccmi_session.h)
        self.has_queue_probe = hasattr(L, "ccmi_queue_probe")
        if self.has_queue_probe:
            L.ccmi_queue_probe.argtypes = [C.c_void_p, C.POINTER(QueueProbeArgsStruct),
                                           C.POINTER(QueueProbeReportStruct)]
            L.ccmi_queue_probe_view.argtypes = [C.c_void_p, C.POINTER(QueueProbeArgsStruct), C.c_int32,
                                                C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                C.c_int32, C.POINTER(C.c_int32)]
        # additive at ABI v13: the symbol's presence is the capability flag (also of goal kind 24)
        self.has_remove_disks = hasattr(L, "ccmi_session_mark_disks_for_removal")
        if self.has_remove_disks:
            L.ccmi_session_mark_disks_for_removal.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_double,
                                                              C.POINTER(C.c_int32)]
        L.ccmi_last_failure_provision.argtypes = [C.c_void_p, C.POINTER(ProvisionRespStruct)]
        L.ccmi_compute_cluster_stats.argtypes = [C.c_void_p, C.POINTER(ConstraintStruct), C.POINTER(OptionsStruct),
                                                 C.POINTER(StatsStruct)]
        L.ccmi_action_log_count.restype = C.c_int64
        L.ccmi_action_log_count.argtypes = [C.c_void_p]
        L.ccmi_action_log_copy.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(ActionStruct)]
        L.ccmi_replica_distribution.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.ccmi_leader_distribution.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.ccmi_proposal_count.restype = C.c_int64
        L.ccmi_proposal_count.argtypes = [C.c_void_p]
        L.ccmi_proposals.argtypes = [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 5
        L.ccmi_proposal_disks.argtypes = [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 2
        L.ccmi_replica_disks.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.ccmi_builder_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        L.ccmi_builder_destroy.argtypes = [C.c_void_p]
        L.ccmi_builder_destroy.restype = None
        L.ccmi_builder_create_broker.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int32,
                                                 C.POINTER(C.c_double), C.c_int32]
        L.ccmi_builder_add_disk.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_double]
        L.ccmi_builder_populate_partition.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_int32),
                                                      C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                                      C.POINTER(C.c_char_p), C.POINTER(C.c_float)]
        L.ccmi_builder_set_broker_state.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.ccmi_builder_set_disk_state.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32]
        L.ccmi_builder_desc.argtypes = [C.c_void_p, C.POINTER(ClusterDesc)]
        L.ccmi_builder_broker_ids.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.ccmi_perf.argtypes = [C.c_void_p, C.POINTER(PerfStruct)]
        L.ccmi_perf_reset.argtypes = [C.c_void_p]
        L.ccmi_set_kernel_timing.argtypes = [C.c_void_p, C.c_int32]
        L.ccmi_session_set_shard.argtypes = [C.c_void_p, C.c_int32, C.c_int32, AllreduceMinFn, C.c_void_p]
        L.ccmi_rccl_unique_id.argtypes = [C.POINTER(C.c_uint8)]
        L.ccmi_session_attach_rccl.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
        L.ccmi_session_attach_shm.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p]
        L.ccmi_session_attach_shm_job.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_uint64, C.c_double]
        L.ccmi_shard_group_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        L.ccmi_shard_group_destroy.argtypes = [C.c_void_p]
        L.ccmi_session_attach_group.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.ccmi_default_constraint.argtypes = [C.POINTER(ConstraintStruct)]
        L.ccmi_topic_broker_set.restype = C.c_int32
        L.ccmi_topic_broker_set.argtypes = [C.c_char_p, C.c_int32]
        L.ccmi_default_random_cluster_props.argtypes = [C.POINTER(RandomClusterProps)]
        L.ccmi_device_count.restype = C.c_int32
        L.ccmi_device_count.argtypes = []

    def device_count(self) -> int:
        """Visible gfx950 devices (ccmi_device_count)."""
        return int(self.lib.ccmi_device_count())

    @classmethod
    def get(cls, path: str = DEFAULT_LIB) -> "Library":
        if path not in cls._cache:
            cls._cache[path] = Library(path)
        return cls._cache[path]

    def check(self, status: int) -> None:
        if status != 0:
            msg = self.lib.ccmi_last_error().decode(errors="replace")
            raise _STATUS.get(status, CruiseControlError)(msg)


# ----------------------------------------------------------------------------------------------- options / constraint
@dataclass
class BalancingConstraint:
    resource_balance_percentage: Sequence[float] = (1.10, 1.10, 1.10, 1.10)
    capacity_threshold: Sequence[float] = (0.7, 0.8, 0.8, 0.8)
    low_utilization_threshold: Sequence[float] = (0.0, 0.0, 0.0, 0.0)
    replica_balance_percentage: float = 1.10
    goal_violation_distribution_threshold_multiplier: float = 1.0
    max_replicas_per_broker: int = 10000
    leader_replica_balance_percentage: float = 1.10
    topic_replica_balance_percentage: float = 3.00
    topic_replica_balance_min_gap: int = 2
    topic_replica_balance_max_gap: int = 40
    overprovisioned_min_extra_racks: int = 2  # AnalyzerConfig.DEFAULT_OVERPROVISIONED_MIN_EXTRA_RACKS
    # BrokerSetAwareGoal: BalancingConstraint.brokerSetResolver() data (broker set id -> broker ids, the content of
    # broker.set.config.file for BrokerSetFileResolver) and replica.to.broker.set.mapping.policy.class. Brokers in no
    # set join "unmapped" (NoOpBrokerSetAssignmentPolicy, the default broker.set.assignment.policy.class).
    broker_sets: Optional[Dict[str, Sequence[int]]] = None
    broker_set_policy: str = "TopicNameHashBrokerSetMappingPolicy"
    # topics.with.min.leaders.per.broker (a regex; "" matches no topic) and min.topic.leaders.per.broker
    # (AnalyzerConfig.java:401-414). The pattern is matched against the session's topic names as
    # Utils.getTopicNamesMatchedWithPattern does (Pattern.matcher(topic).matches() = re.fullmatch; common/Utils.java:26-36).
    topics_with_min_leaders_per_broker: str = ""
    min_topic_leaders_per_broker: int = 1
    # TopicLeaderReplicaDistributionGoal: topic.leader.replica.count.balance.{threshold,min.gap,max.gap} and
    # topic.leader.replica.distribution.goal.balance.margin (AnalyzerConfig.java:112-146)
    topic_leader_replica_balance_percentage: float = 1.10
    topic_leader_replica_balance_min_gap: int = 2
    topic_leader_replica_balance_max_gap: int = 10
    topic_leader_replica_balance_margin: float = 0.9

    def set_resource_balance_percentage(self, p: float) -> None:  # BalancingConstraint.setResourceBalancePercentage
        self.resource_balance_percentage = (p, p, p, p)

    def set_capacity_threshold(self, t: float) -> None:
        self.capacity_threshold = (t, t, t, t)

    def min_leader_topics(self, topic_names: Optional[Sequence[str]]) -> List[int]:
        """Topic indices topics.with.min.leaders.per.broker matches (Utils.getTopicNamesMatchedWithPattern)."""
        if not self.topics_with_min_leaders_per_broker:
            return []
        import re
        pat = re.compile(self.topics_with_min_leaders_per_broker)
        if topic_names is None:
            raise IllegalArgumentException("topics.with.min.leaders.per.broker needs the cluster's topic names")
        return [t for t, n in enumerate(topic_names) if pat.fullmatch(n)]

    def to_struct(self, topic_names: Optional[Sequence[str]] = None,
                  broker_ids: Optional[Sequence[int]] = None) -> ConstraintStruct:
        """broker_ids: the session's Kafka broker id of every broker index (ClusterModel.broker_ids); the broker ids
        of `broker_sets` are mapped through it to the session's dense indices (ccmi_balancing_constraint
        broker_set_members), an id the model does not hold to -1. None: ids are the indices."""
        s = ConstraintStruct()
        s.resource_balance_percentage[:] = list(self.resource_balance_percentage)
        s.capacity_threshold[:] = list(self.capacity_threshold)
        s.low_utilization_threshold[:] = list(self.low_utilization_threshold)
        s.replica_balance_percentage = self.replica_balance_percentage
        s.leader_replica_balance_percentage = self.leader_replica_balance_percentage
        s.topic_replica_balance_percentage = self.topic_replica_balance_percentage
        s.topic_replica_balance_min_gap = self.topic_replica_balance_min_gap
        s.topic_replica_balance_max_gap = self.topic_replica_balance_max_gap
        s.goal_violation_distribution_threshold_multiplier = self.goal_violation_distribution_threshold_multiplier
        s.max_replicas_per_broker = self.max_replicas_per_broker
        s.overprovisioned_max_replicas_per_broker = 1500
        s.overprovisioned_min_brokers = 3
        s.overprovisioned_min_extra_racks = self.overprovisioned_min_extra_racks
        s.topic_leader_replica_balance_percentage = self.topic_leader_replica_balance_percentage
        s.topic_leader_replica_balance_min_gap = self.topic_leader_replica_balance_min_gap
        s.topic_leader_replica_balance_max_gap = self.topic_leader_replica_balance_max_gap
        s.topic_leader_replica_balance_margin = self.topic_leader_replica_balance_margin
        if self.broker_sets:
            names = list(self.broker_sets)
            index_of = None if broker_ids is None else {int(k): i for i, k in enumerate(broker_ids)}
            members = [int(b) if index_of is None else index_of.get(int(b), -1)
                       for n in names for b in self.broker_sets[n]]
            offs = [0]
            for n in names:
                offs.append(offs[-1] + len(self.broker_sets[n]))
            keep = [(C.c_char_p * len(names))(*[n.encode() for n in names]), (C.c_int32 * len(offs))(*offs),
                    (C.c_int32 * max(1, len(members)))(*members)]
            s._keep = keep  # the arrays live as long as the struct
            s.num_broker_sets = len(names)
            s.broker_set_names = C.cast(keep[0], C.POINTER(C.c_char_p))
            s.broker_set_offset = C.cast(keep[1], C.POINTER(C.c_int32))
            s.broker_set_members = C.cast(keep[2], C.POINTER(C.c_int32))
        if self.broker_set_policy not in BROKER_SET_POLICIES:
            raise IllegalArgumentException(f"unknown broker set mapping policy {self.broker_set_policy}")
        s.broker_set_policy = BROKER_SET_POLICIES[self.broker_set_policy]
        if self.min_topic_leaders_per_broker < 0:  # ConfigDef atLeast(0)
            raise IllegalArgumentException("min.topic.leaders.per.broker must be at least 0")
        s.min_topic_leaders_per_broker = self.min_topic_leaders_per_broker
        mlt = self.min_leader_topics(topic_names)
        if mlt:
            a = (C.c_int32 * len(mlt))(*mlt)
            s._keep_mlt = a
            s.min_leader_topics = C.cast(a, C.POINTER(C.c_int32))
            s.num_min_leader_topics = len(mlt)
        return s


@dataclass
class OptimizationOptions:
    excluded_topics: Sequence[int] = ()
    excluded_brokers_for_leadership: Sequence[int] = ()
    excluded_brokers_for_replica_move: Sequence[int] = ()
    is_triggered_by_goal_violation: bool = False
    requested_destination_broker_ids: Sequence[int] = ()
    only_move_immigrant_replicas: bool = False
    # The reference defaults fastMode to true (OptimizationOptions 6-arg ctor), which caps every per-broker loop by a
    # wall-clock timeout (fast.mode.per.broker.move.timeout.ms) and makes the result depend on host speed. The
    # engine never cuts a loop short — the result fast mode reaches when no timeout fires — so the binding defaults
    # to False to say so explicitly; fast_mode=True is accepted and behaves identically.
    fast_mode: bool = False

    def to_struct(self):
        keep = []

        def arr(xs):
            a = (C.c_int32 * max(1, len(xs)))(*xs)
            keep.append(a)
            return C.cast(a, C.POINTER(C.c_int32)), len(xs)

        s = OptionsStruct()
        s.excluded_topics, s.num_excluded_topics = arr(list(self.excluded_topics))
        s.excluded_brokers_for_leadership, s.num_excluded_brokers_for_leadership = arr(
            list(self.excluded_brokers_for_leadership))
        s.excluded_brokers_for_replica_move, s.num_excluded_brokers_for_replica_move = arr(
            list(self.excluded_brokers_for_replica_move))
        s.triggered_by_goal_violation = int(self.is_triggered_by_goal_violation)
        s.requested_destination_broker_ids, s.num_requested_destination_broker_ids = arr(
            list(self.requested_destination_broker_ids))
        s.only_move_immigrant_replicas = int(self.only_move_immigrant_replicas)
        s.fast_mode = int(self.fast_mode)
        return s, keep


# ----------------------------------------------------------------------------------------------- goals
class Goal:
    """A goal plugin by reference simple class name (Goal.name(), AbstractGoal.java:141-144)."""

    def __init__(self, name: Optional[str] = None, constraint: Optional[BalancingConstraint] = None):
        self._name = name or type(self).__name__
        if self._name not in GOAL_KINDS:
            raise IllegalArgumentException(f"unknown goal {self._name}")
        self.constraint = constraint

    def name(self) -> str:
        return self._name

    @property
    def kind(self) -> int:
        return GOAL_KINDS[self._name]

    # Goal.isHardGoal(): AbstractRackAwareGoal (both rack goals), BrokerSetAwareGoal, CapacityGoal, ReplicaCapacityGoal,
    # IntraBrokerDiskCapacityGoal return true (analyzer/goals/*.java)
    HARD_GOALS = ("RackAwareGoal", "RackAwareDistributionGoal", "BrokerSetAwareGoal", "ReplicaCapacityGoal",
                  "DiskCapacityGoal", "NetworkInboundCapacityGoal", "NetworkOutboundCapacityGoal", "CpuCapacityGoal",
                  "IntraBrokerDiskCapacityGoal", "KafkaAssignerEvenRackAwareGoal",
                  "KafkaAssignerDiskUsageDistributionGoal")

    def is_hard_goal(self) -> bool:
        return self._name in self.HARD_GOALS

    def optimize(self, cluster: "ClusterModel", optimized_goals: Iterable["Goal"] = (),
                 options: Optional[OptimizationOptions] = None) -> bool:
        """Goal.optimize(clusterModel, optimizedGoals, optimizationOptions) (Goal.java:60-68). Only the goals in
        `optimized_goals` constrain this goal's moves through their actionAcceptance; each must have been optimized
        on this session (else UnsupportedOperationException: the JVM would run the goal). The session
        keeps this goal, with its frozen state, for later optimized_goals sets."""
        if isinstance(optimized_goals, OptimizationOptions):
            raise IllegalArgumentException("Goal.optimize(cluster, optimized_goals, options): optimized_goals first")
        res = cluster._goal_optimize(self, optimized_goals, options)
        return bool(res.succeeded)

    def __repr__(self) -> str:
        return self._name


for _n in GOAL_KINDS:
    globals()[_n] = type(_n, (Goal,), {})


class IntraBrokerDiskCapacityGoalEmptyDisks(Goal):
    """new IntraBrokerDiskCapacityGoal(true) (IntraBrokerDiskCapacityGoal.java:61-63): also empties zero-capacity
    disks. goals_from_names([REMOVE_DISKS_GOAL]) builds it; name() is IntraBrokerDiskCapacityGoal."""

    def __init__(self, constraint: Optional[BalancingConstraint] = None):
        super().__init__("IntraBrokerDiskCapacityGoal", constraint)

    @property
    def kind(self) -> int:
        return REMOVE_DISKS_GOAL_KIND

    def __repr__(self) -> str:
        return REMOVE_DISKS_GOAL


globals()[REMOVE_DISKS_GOAL] = IntraBrokerDiskCapacityGoalEmptyDisks


# ----------------------------------------------------------------------------------------------- results
PROVISION_STATUSES = ("UNDECIDED", "RIGHT_SIZED", "UNDER_PROVISIONED", "OVER_PROVISIONED")  # ProvisionStatus.java


@dataclass
class ProvisionRecommendation:
    """analyzer/ProvisionRecommendation.java (-1 = unset; topic pattern and excluded rack ids not carried)."""
    status: str
    num_brokers: int = -1
    num_racks: int = -1
    num_disks: int = -1
    num_partitions: int = -1
    typical_broker_id: int = -1
    resource: Optional[str] = None
    typical_broker_capacity: float = -1.0
    total_capacity: float = -1.0


RESOURCE_NAMES = {"CPU": "cpu", "NW_IN": "networkInbound", "NW_OUT": "networkOutbound", "DISK": "disk"}  # Resource.java


def _recommendation_text(r: "ProvisionRecommendation") -> str:
    s = f"{'Add' if r.status == 'UNDER_PROVISIONED' else 'Remove'} at least "
    if r.num_brokers != -1:
        s += f"{r.num_brokers} broker{'s' if r.num_brokers > 1 else ''}"
    elif r.num_racks != -1:
        s += f"{r.num_racks} rack{'s' if r.num_racks > 1 else ''} with brokers"
    elif r.num_disks != -1:
        s += f"{r.num_disks} disk{'s' if r.num_disks > 1 else ''}"
    if r.typical_broker_id != -1:
        s += f" with the same {RESOURCE_NAMES[r.resource]} capacity ({r.typical_broker_capacity:.2f}) as broker-" \
             f"{r.typical_broker_id}"
    elif r.resource is not None:
        s += f" for {RESOURCE_NAMES[r.resource]}"
    if r.total_capacity != -1.0:
        s += f" with a total capacity of {r.total_capacity:.2f}"
    return s + "."


def _goal_of_message(msg: str) -> str:
    """The goal name an OptimizationFailureException message starts with ("[GoalName] ...")."""
    return msg[1:msg.index("]")] if msg.startswith("[") and "]" in msg else ""


class ProvisionResponse:
    """analyzer/ProvisionResponse.java: a status and the recommendations by recommender (goal name);
    aggregate() follows ProvisionResponse.aggregate (:97-129)."""

    def __init__(self, status: str = "UNDECIDED", recommendation: Optional[ProvisionRecommendation] = None,
                 recommender: Optional[str] = None):
        if recommendation is not None and status not in ("UNDER_PROVISIONED", "OVER_PROVISIONED"):
            raise IllegalArgumentException(f"Recommendation is irrelevant for provision status {status}.")
        self.status = status
        self.recommendation_by_recommender: Dict[str, ProvisionRecommendation] = {}
        if recommendation is not None:
            if recommender is None:
                raise IllegalArgumentException("The recommender cannot be null.")
            self.recommendation_by_recommender[recommender] = recommendation

    @staticmethod
    def from_struct(p: "ProvisionRespStruct", recommender: str) -> "ProvisionResponse":
        status = PROVISION_STATUSES[p.status]
        if not p.has_recommendation:
            return ProvisionResponse(status)
        r = p.recommendation
        rec = ProvisionRecommendation(PROVISION_STATUSES[r.status], r.num_brokers, r.num_racks, r.num_disks,
                                      r.num_partitions, r.typical_broker_id,
                                      RESOURCES[r.resource] if r.resource >= 0 else None, r.typical_broker_capacity,
                                      r.total_capacity)
        return ProvisionResponse(status, rec, recommender)

    def aggregate(self, other: "ProvisionResponse") -> "ProvisionResponse":
        if self.status == "UNDER_PROVISIONED":
            if other.status == "UNDER_PROVISIONED":
                self.recommendation_by_recommender.update(other.recommendation_by_recommender)
        elif other.status == "UNDER_PROVISIONED":
            self.status = "UNDER_PROVISIONED"
            self.recommendation_by_recommender = dict(other.recommendation_by_recommender)
        elif other.status == "RIGHT_SIZED":
            self.status = "RIGHT_SIZED"
            self.recommendation_by_recommender = {}
        elif other.status == "OVER_PROVISIONED":
            if self.status in ("OVER_PROVISIONED", "UNDECIDED"):
                self.status = "OVER_PROVISIONED"
                self.recommendation_by_recommender.update(other.recommendation_by_recommender)
        return self

    def recommendation(self) -> str:
        """ProvisionResponse.recommendation(): "[recommender] text" per recommendation (ProvisionRecommendation.toString,
        ProvisionRecommendation.java:364-398)."""
        return " ".join(f"[{k}] {_recommendation_text(v)}" for k, v in self.recommendation_by_recommender.items())

    def __eq__(self, other) -> bool:
        return isinstance(other, ProvisionResponse) and (self.status, self.recommendation_by_recommender) == \
            (other.status, other.recommendation_by_recommender)

    def __repr__(self) -> str:
        return f"ProvisionResponse({self.status}, {self.recommendation_by_recommender})"


@dataclass
class ExecutionProposal:
    partition: int
    partition_size: int
    old_leader: int
    old_replicas: List[int]
    new_replicas: List[int]
    old_disks: Optional[List[int]] = None  # logdir half of ReplicaPlacementInfo (disk indices; JBOD models)
    new_disks: Optional[List[int]] = None


@dataclass
class GoalResult:
    name: str
    succeeded: bool
    has_diff: bool
    seconds: float
    candidates: int
    device_candidates: int
    device_launches: int
    actions: int
    stats: Dict[str, object]
    provision: Optional[ProvisionResponse] = None  # Goal.provisionResponse after the goal


BROKER_STATE_NAMES = ("ALIVE", "DEAD", "NEW", "DEMOTED", "BAD_DISKS")  # ccmi_broker_state order


class BrokerStats:
    """servlet/response/stats/BrokerStats.java as ClusterModel.brokerStats fills it (ClusterModel.java:1303-1309), read
    from the device tables by ccmi_broker_stats. `brokers`, `hosts` and `disks` are numpy structured arrays with the
    fields of BasicStatsStruct / DiskStatsStruct: one row per broker in index order, one per distinct host in ascending
    host index, one per disk in desc order (empty without disks). The isEstimated flag is not carried (the desc holds
    no capacity-estimation information) and the plain-text table is left to the servlet."""

    BASIC_KEYS = (("DiskMB", "disk_mb"), ("DiskPct", "disk_pct"), ("CpuPct", "cpu_pct"),
                  ("LeaderNwInRate", "leader_nw_in_rate"), ("FollowerNwInRate", "follower_nw_in_rate"),
                  ("NwOutRate", "nw_out_rate"), ("PnwOutRate", "pnw_out_rate"), ("Replicas", "replicas"),
                  ("Leaders", "leaders"), ("DiskCapacityMB", "disk_capacity_mb"),
                  ("NetworkInCapacity", "network_in_capacity"), ("NetworkOutCapacity", "network_out_capacity"),
                  ("NumCore", "num_core"))

    def __init__(self, brokers, hosts, disks, broker_ids: Sequence[int], rack_names: Dict[int, str],
                 host_names: Dict[int, str], logdirs: Sequence[str]):
        self.brokers, self.hosts, self.disks = brokers, hosts, disks
        self.broker_ids = list(broker_ids)
        self.rack_names, self.host_names = dict(rack_names), dict(host_names)
        self.logdirs = list(logdirs)

    def rack_name(self, rack: int) -> str:
        return self.rack_names.get(int(rack), str(int(rack)))

    def host_name(self, host: int) -> str:
        return self.host_names.get(int(host), str(int(host)))

    def _basic(self, row) -> Dict[str, object]:
        return {key: (int(row[f]) if f in ("replicas", "leaders") else float(row[f])) for key, f in self.BASIC_KEYS}

    def get_json_structure(self) -> Dict[str, object]:
        """BrokerStats.getJsonStructure (BrokerStats.java:92-112): the hosts ordered by host name (the reference's
        ConcurrentSkipListMap), the brokers in id order; a broker with disks carries DiskState by logdir, a dead disk
        "DEAD" for DiskMB and DiskPct (DiskStats.java:62-65)."""
        hosts = []
        for row in self.hosts:
            e = self._basic(row)
            e["Host"], e["Rack"] = self.host_name(row["host"]), self.rack_name(row["rack"])
            hosts.append(e)
        # hosts are distinct by index (a host is keyed by name within its rack, Rack._hosts): rows that share a name in
        # different racks stay separate entries, next to each other in host index order (the sort is stable)
        hosts.sort(key=lambda e: e["Host"])
        disks_of: Dict[int, Dict[str, object]] = {}
        for d in self.disks:
            dead = not d["capacity"] > 0
            disks_of.setdefault(int(d["broker"]), {})[self.logdirs[int(d["disk"])]] = {
                "DiskMB": "DEAD" if dead else float(d["disk_mb"]), "DiskPct": "DEAD" if dead else float(d["disk_pct"]),
                "NumLeaderReplicas": int(d["num_leader_replicas"]), "NumReplicas": int(d["num_replicas"])}
        brokers = []
        for row in self.brokers:
            e = self._basic(row)
            b = int(row["broker"])
            e["Host"], e["Broker"] = self.host_name(row["host"]), self.broker_ids[b]
            e["BrokerState"] = BROKER_STATE_NAMES[int(row["state"])]
            if b in disks_of:
                e["DiskState"] = dict(sorted(disks_of[b].items()))  # Broker._diskByLogdir is a TreeMap
            e["Rack"] = self.rack_name(row["rack"])
            brokers.append(e)
        return {"hosts": hosts, "brokers": brokers}

    def __eq__(self, other) -> bool:
        return (isinstance(other, BrokerStats) and self.brokers.tobytes() == other.brokers.tobytes()
                and self.hosts.tobytes() == other.hosts.tobytes() and self.disks.tobytes() == other.disks.tobytes())

    __hash__ = None


class PartitionLoadState:
    """servlet/response/PartitionLoadState.java as PartitionLoadRunnable.getResult fills it, computed, sorted and cut by
    ccmi_partition_load. `records` is a numpy structured array with the fields of PartitionLoadRecordStruct, in the
    response's order; `num_selected` the partitions the selection kept before the entries cut. MESSAGE_IN_RATE (msg_in)
    is not a metric the model carries and is left out; the plain-text table is left to the servlet."""

    JSON_VERSION = 1
    RESOURCE_KEYS = (("cpu", 0), ("networkInbound", 1), ("networkOutbound", 2), ("disk", 3))  # Resource.resource()

    def __init__(self, records, num_selected: int, topic_names: Sequence[str], partition_topic: Sequence[int],
                 partition_number: Sequence[int], broker_ids: Sequence[int]):
        self.records = records
        self.num_selected = int(num_selected)
        self.topic_names = list(topic_names)
        self.partition_topic, self.partition_number = partition_topic, partition_number
        self.broker_ids = list(broker_ids)

    def get_json_structure(self) -> Dict[str, object]:
        """PartitionLoadState.getJsonString (PartitionLoadState.java:103-150): leader and followers as broker ids,
        `partition` the topic's partition number."""
        out = []
        for r in self.records:
            p, n = int(r["partition"]), int(r["num_replicas"])
            e: Dict[str, object] = {"topic": self.topic_names[self.partition_topic[p]],
                                    "partition": int(self.partition_number[p]),
                                    "leader": self.broker_ids[int(r["brokers"][0])],
                                    "followers": [self.broker_ids[int(b)] for b in r["brokers"][1:n]]}
            for key, res in self.RESOURCE_KEYS:
                e[key] = float(r["util"][res])
            out.append(e)
        return {"version": self.JSON_VERSION, "records": out}

    def __eq__(self, other) -> bool:
        return (isinstance(other, PartitionLoadState) and self.num_selected == other.num_selected
                and self.records.tobytes() == other.records.tobytes())

    __hash__ = None


class ProposalDiff:
    """AnalyzerUtils.getDiff of the session's current model against its initial placement, as ccmi_proposal_diff
    computed it on the device. `records` is a numpy structured array with the fields of ProposalRecordStruct in
    ascending partition order (the first `capacity` of them), `summary` a ProposalSummaryStruct over every proposal,
    returned or not."""

    def __init__(self, records, summary: ProposalSummaryStruct):
        self.records = records
        self.summary = summary

    @property
    def num_proposals(self) -> int:
        return int(self.summary.num_proposals)

    @property
    def proposals(self) -> List[ExecutionProposal]:
        """The returned records as ExecutionProposals: what ClusterModel.proposals() lists."""
        out = []
        for r in self.records:
            n = int(r["num_replicas"])
            out.append(ExecutionProposal(int(r["partition"]), int(r["size"]), int(r["old_leader"]),
                                         [int(x) for x in r["old_replicas"][:n]],
                                         [int(x) for x in r["new_replicas"][:n]],
                                         [int(x) for x in r["old_disks"][:n]], [int(x) for x in r["new_disks"][:n]]))
        return out

    def movement_stats(self) -> List[int]:
        """OptimizerResult.getMovementStats, in the order of OptimizerResult.movement_stats."""
        s = self.summary
        return [int(s.num_inter_broker_replica_movements), int(s.inter_broker_data_to_move_mb),
                int(s.num_intra_broker_replica_movements), int(s.intra_broker_data_to_move_mb),
                int(s.num_leadership_movements)]


class ExecutionPlan:
    """What ExecutionTaskPlanner.addExecutionProposals builds from the proposals of the session's current model, as
    ccmi_execution_plan computed it on the device. `tasks` is a numpy structured array with the fields of
    PlanTaskStruct, indexed by execution id; `inter[b]` the execution ids of broker b's inter-broker tasks in strategy
    order; `broker_order` the brokers with such tasks in brokerComparator's initial order; `intra[b]` the partitions of
    broker b's intra-broker tasks and `leader_tasks` the partitions of the leadership tasks, both in proposal order;
    `summary` a PlanSummaryStruct. `strategies` (CCMI_STRATEGY_* numbers) and `partition_state` are the query's."""

    def __init__(self, summary: PlanSummaryStruct, tasks, inter, broker_order, intra, leader_tasks, strategies,
                 partition_state):
        self.summary = summary
        self.tasks = tasks
        self.inter = inter
        self.broker_order = broker_order
        self.intra = intra
        self.leader_tasks = leader_tasks
        self.strategies = list(strategies)
        self.partition_state = partition_state
        # next_round's state: the tasks still filed under each broker, and the brokers of each task
        self._lists = [[int(t) for t in seg] for seg in inter]
        self._brokers = {}
        for b, seg in enumerate(self._lists):
            for t in seg:
                self._brokers.setdefault(t, []).append(b)

    def task_key(self, t: int):
        """Task t's place under the chain as a tuple: the device's order (sizes compared as int64)."""
        st = int(self.partition_state[int(self.tasks["partition"][t])]) if self.partition_state is not None else 0
        data, key = int(self.tasks["data_to_move_mb"][t]), []
        for s in self.strategies:
            if s == STRATEGY_BASE:
                break
            key.append({STRATEGY_PRIORITIZE_LARGE: -data, STRATEGY_PRIORITIZE_SMALL: data,
                        STRATEGY_POSTPONE_URP: 1 if st & PSTATE_UNDER_REPLICATED else 0,
                        STRATEGY_PRIORITIZE_MIN_ISR_WITH_OFFLINE:
                            0 if st & PSTATE_UNDER_MIN_ISR else 1 if st & PSTATE_AT_MIN_ISR else 2,
                        STRATEGY_PRIORITIZE_ONE_ABOVE_MIN_ISR_WITH_OFFLINE:
                            0 if st & PSTATE_ONE_ABOVE_MIN_ISR else 1}[s])
        return tuple(key) + (t,)

    def remaining(self) -> int:
        """Inter-broker tasks no round has taken yet."""
        return len(self._brokers)

    def next_round(self, ready_brokers: Dict[int, int], in_progress=(), max_moves: int = 1 << 30) -> List[int]:
        """ExecutionTaskPlanner.getInterBrokerReplicaMovementTasks (ExecutionTaskPlanner.java:348-439) over the
        returned lists, on the host: the execution ids of the next executable tasks, which leave the plan.
        `ready_brokers` maps a broker to its free movement slots and is decremented as the reference decrements it (a
        broker of a checked task that is missing raises KeyError, where the reference throws a NullPointerException);
        `in_progress` holds partition indices; `max_moves` caps in-progress plus returned partitions. The source of
        a task is the broker its proposal's old leader is on; the lists file a task under it and under every
        destination, and the round treats the two alike, so the brokers of a task are those whose list holds it."""
        lists, out = self._lists, []
        busy_parts = set(int(p) for p in in_progress)
        num_in_progress, involved_parts = len(busy_parts), set()

        def broker_key(b):  # brokerComparator on the lists as they are now
            return (self.task_key(lists[b][0]), -len(lists[b]), b)

        added, capped = True, False
        while added and not capped:
            added = False
            involved = set()
            for b in sorted((b for b in range(len(lists)) if lists[b]), key=broker_key):
                if capped:
                    break
                if b in involved:
                    continue
                for t in list(lists[b]):
                    if num_in_progress >= max_moves:
                        capped = True
                        break
                    brokers = self._brokers[t]
                    if any(x in involved for x in brokers):
                        continue
                    part = int(self.tasks["partition"][t])
                    if all(ready_brokers[x] > 0 for x in brokers) and part not in busy_parts \
                            and part not in involved_parts:
                        involved_parts.add(part)
                        out.append(t)
                        involved.update(brokers)
                        for x in brokers:
                            lists[x].remove(t)
                            ready_brokers[x] -= 1
                        del self._brokers[t]
                        added = True
                        num_in_progress += 1
                        break
        return out


class OptimizerResult:
    """analyzer/OptimizerResult.java: per-goal results, the ExecutionProposals and the ordered action log. The
    proposals, the action log and the broker stats after the optimization are read from the session on first access
    (the session keeps them until its next optimization), so a caller that only needs the statistics does not pay for
    them."""

    def __init__(self, goal_results: List[GoalResult], cluster: "ClusterModel", seconds: float,
                 violated_goals_after: List[str]):
        self.goal_results = goal_results
        self.seconds = seconds
        self.violated_goals_after = violated_goals_after
        self._cluster = cluster
        self._num_actions = cluster.lib.lib.ccmi_action_log_count(cluster.handle)
        self._proposals: Optional[List[ExecutionProposal]] = None
        self._actions: Optional[List[tuple]] = None
        # ClusterModel.brokerStats before the first goal (GoalOptimizer.java:442): taken only when optimizations() was
        # asked for it
        self.broker_stats_before_optimization: Optional[BrokerStats] = None
        self._stats_after: Optional[BrokerStats] = None

    @property
    def broker_stats_after_optimization(self) -> BrokerStats:
        """OptimizerResult._brokerStatsAfterOptimization (OptimizerResult.java:111), read from the session on first
        access, under the same rule as `proposals`."""
        if self._stats_after is None:
            self._stats_after = self._cluster.broker_stats()
        return self._stats_after

    def load_json(self, verbose: bool = False) -> Dict[str, object]:
        """The load blocks of a rebalance response (OptimizerResult.getJsonStructure): loadAfterOptimization, and in
        verbose mode loadBeforeOptimization when optimizations() took it."""
        out: Dict[str, object] = {}
        if verbose and self.broker_stats_before_optimization is not None:
            out["loadBeforeOptimization"] = self.broker_stats_before_optimization.get_json_structure()
        out["loadAfterOptimization"] = self.broker_stats_after_optimization.get_json_structure()
        return out

    @property
    def proposals(self) -> List[ExecutionProposal]:
        if self._proposals is None:
            self._proposals = self._cluster.proposals()
        return self._proposals

    @property
    def actions(self) -> List[tuple]:
        if self._actions is None:
            self._actions = self._cluster.actions()[:self._num_actions]
        return self._actions

    @property
    def candidates(self) -> int:
        return sum(g.candidates for g in self.goal_results)

    # GoalOptimizer.optimizations (:480-485): a goal is violated before the optimization when it moved something or
    # did not succeed, and after it when it did not succeed
    @property
    def violated_goals_before(self) -> List[str]:
        return [g.name for g in self.goal_results if g.has_diff or not g.succeeded]

    @property
    def violated_goals_after_optimization(self) -> List[str]:
        return list(self.violated_goals_after)

    def _balancedness(self, violated: Sequence[str]) -> float:
        """OptimizerResult.onDemandBalancednessScore (OptimizerResult.java:123-131)."""
        score = MAX_BALANCEDNESS_SCORE
        cost = getattr(self, "balancedness_cost_by_goal", {})
        for g in self.goal_results:
            if g.name in violated:
                score -= cost.get(g.name, 0.0)
        return score

    @property
    def on_demand_balancedness_score_before(self) -> float:
        return self._balancedness(self.violated_goals_before)

    @property
    def on_demand_balancedness_score_after(self) -> float:
        return self._balancedness(self.violated_goals_after)

    def goal_result_description(self, goal_name: str) -> str:
        """OptimizerResult.goalResultDescription (:243-246)."""
        if goal_name not in self.violated_goals_before:
            return "NO-ACTION"
        return "VIOLATED" if goal_name in self.violated_goals_after else "FIXED"

    def movement_stats(self) -> List[int]:
        """OptimizerResult.getMovementStats (:259-279): inter-broker replica moves and MB, intra-broker replica moves
        and MB, leadership moves, over the ExecutionProposals (replicasToAdd / replicasToRemove /
        replicasToMoveBetweenDisksByBroker of ExecutionProposal.java:169-245)."""
        n_inter = mb_inter = n_intra = mb_intra = n_lead = 0
        for p in self.proposals:
            # ExecutionProposal.java:74-78: additions / removals by broker id; a replica whose (broker, logdir) is new
            # on a broker that keeps the partition moves between disks
            old_b, new_b = set(p.old_replicas), set(p.new_replicas)
            to_add, to_remove = new_b - old_b, old_b - new_b
            old_pl = set(zip(p.old_replicas, p.old_disks or [-1] * len(p.old_replicas)))
            between_disks = [b for b, d in zip(p.new_replicas, p.new_disks or [-1] * len(p.new_replicas))
                             if b not in to_add and (b, d) not in old_pl]
            if to_add or to_remove:
                n_inter += 1
                mb_inter += len(to_add) * p.partition_size
            elif between_disks:
                n_intra += len(between_disks)
                mb_intra += p.partition_size * len(between_disks)
            else:
                n_lead += 1
        return [n_inter, mb_inter, n_intra, mb_intra, n_lead]

    def proposal_summary_json(self) -> Dict[str, object]:
        """OptimizerResult.getProposalSummaryForJson (OptimizerResult.java:300-320)."""
        m = self.movement_stats()
        opts = getattr(self, "options", None) or OptimizationOptions()
        names = self._cluster.topic_names()
        prov = self.provision_response
        return {
            "numReplicaMovements": m[0], "dataToMoveMB": m[1], "numIntraBrokerReplicaMovements": m[2],
            "intraBrokerDataToMoveMB": m[3], "numLeaderMovements": m[4],
            "recentWindows": self._cluster.desc.num_windows, "monitoredPartitionsPercentage": 100.0,
            "excludedTopics": sorted(names[t] for t in opts.excluded_topics),
            "excludedBrokersForLeadership": sorted(opts.excluded_brokers_for_leadership),
            "excludedBrokersForReplicaMove": sorted(opts.excluded_brokers_for_replica_move),
            "onDemandBalancednessScoreBefore": self.on_demand_balancedness_score_before,
            "onDemandBalancednessScoreAfter": self.on_demand_balancedness_score_after,
            "provisionStatus": prov.status, "provisionRecommendation": prov.recommendation(),
        }

    def proposals_json(self) -> List[Dict[str, object]]:
        """ExecutionProposal.getJsonStructure (ExecutionProposal.java:266-270) of every proposal."""
        names = self._cluster.topic_names()
        d = self._cluster.desc
        return [{"topicPartition": f"{names[d.partition_topic[p.partition]]}-{d.partition_number[p.partition]}",
                 "oldLeader": p.old_leader, "oldReplicas": list(p.old_replicas), "newReplicas": list(p.new_replicas)}
                for p in self.proposals]

    @property
    def provision_response(self) -> ProvisionResponse:
        """The aggregated provision response GoalOptimizer.optimizations reports (GoalOptimizer.java:456-496)."""
        agg = ProvisionResponse("UNDECIDED")
        for g in self.goal_results:
            if g.provision is not None:
                agg.aggregate(g.provision)
        return agg


def stats_to_dict(s: StatsStruct) -> Dict[str, object]:
    out = {}
    for name, typ in StatsStruct._fields_:
        v = getattr(s, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    return out


# ----------------------------------------------------------------------------------------------- cluster / session
class ClusterBuffers:
    """Owns a generated flattened cluster (RandomCluster fixture)."""

    def __init__(self, lib: Library, handle: int):
        self.lib = lib
        self.handle = C.c_void_p(handle)
        self.desc = lib.lib.ccmi_cluster_buffers_desc(self.handle).contents

    def __del__(self):
        try:
            self.lib.lib.ccmi_cluster_buffers_free(self.handle)
        except Exception:
            pass


class RandomCluster:
    """RandomCluster.generate + populate (RandomCluster.java:53-336) with TestConstants.BASE_PROPERTIES defaults."""

    BASE = dict(num_racks=10, num_brokers=40, num_dead_brokers=0, num_brokers_with_bad_disk=0, num_replicas=50001,
                num_topics=3000, min_replication=3, max_replication=3, mean_cpu=0.01, mean_disk=100.0,
                mean_nw_in=100.0, mean_nw_out=100.0, distribution=0, rack_aware=0, leader_in_first_position=1)

    @staticmethod
    def props(**overrides) -> RandomClusterProps:
        d = dict(RandomCluster.BASE)
        d.update(overrides)
        p = RandomClusterProps()
        for k, v in d.items():
            if k == "logdir_capacity":
                v = (C.c_double * 8)(*(list(v) + [0.0] * (8 - len(v))))
            setattr(p, k, v)
        return p

    @staticmethod
    def generate(lib: Optional[Library] = None, **overrides) -> ClusterBuffers:
        lib = lib or Library.get()
        h = C.c_void_p()
        lib.check(lib.lib.ccmi_random_cluster(C.byref(RandomCluster.props(**overrides)), C.byref(h)))
        return ClusterBuffers(lib, h.value)


METRIC_OF_RESOURCE = {"CPU": 0, "NW_IN": 2, "NW_OUT": 3, "DISK": 1}  # first metric id of each resource group
BROKER_STATES = {"ALIVE": 0, "DEAD": 1, "NEW": 2, "DEMOTED": 3, "BAD_DISKS": 4}
DISK_STATES = {"ALIVE": 0, "DEAD": 1, "DEMOTED": 2}


class ClusterModelBuilder:
    """Builds the flattened model (ccmi_cluster_desc) with the reference's ClusterModel construction API
    (model/ClusterModel.java: createRack :948, createBroker :923, createReplica :800-880, setReplicaLoad :738-760,
    setBrokerState :297-336) — the calls LoadMonitor.clusterModel and the test fixtures make. Construction order is
    kept: replicas are indexed in createReplica order, every Partition._replicas list is built by list insertion at
    the given index (Partition.addLeader/addFollower), and setReplicaLoad order becomes replica_load_order.

    Loads follow KafkaCruiseControlUnitTestUtils.getAggregatedMetricValues: the whole resource value goes to the
    first metric id of the resource group (KafkaCruiseControlUnitTestUtils.java:90-145). Broker ids must be 0..B-1.
    An optional rack-id mapper (AnalyzerConfig rack.aware.goal.rack.id.mapper.class) is applied here: racks that map
    to the same id become one rack index."""

    def __init__(self, num_windows: int = 1, rack_id_mapper=None):
        self.W = num_windows
        self.mapper = rack_id_mapper or (lambda r: r)
        self.rack_index: Dict[str, int] = {}
        self.brokers: Dict[int, tuple] = {}   # id -> (rack index, capacity[4])
        self.state: Dict[int, int] = {}
        self.topics: List[str] = []
        self.topic_index: Dict[str, int] = {}
        self.parts: Dict[tuple, int] = {}     # (topic, partition) -> partition index
        self.part_list: List[List[int]] = []  # Partition._replicas (replica indices)
        self.rep_part: List[int] = []
        self.rep_broker: List[int] = []
        self.rep_leader: List[int] = []
        self.rep_offline: List[int] = []
        self.rep_load: List[Optional[List[float]]] = []
        self.load_order: List[int] = []
        self.disks: List[tuple] = []          # (broker, logdir, capacity) in creation order
        self.disk_index: Dict[tuple, int] = {}
        self.disk_demoted: Dict[int, int] = {}
        self.rep_disk: List[int] = []
        self.host: Dict[int, str] = {}        # broker id -> host name (Rack._hosts key); absent = its own host

    def create_rack(self, rack_id: str) -> None:
        self.rack_index.setdefault(str(self.mapper(str(rack_id))), len(self.rack_index))

    def create_broker(self, rack_id: str, broker_id: int, capacity: Dict[str, float],
                      disk_capacity_by_logdir: Optional[Dict[str, float]] = None, host: Optional[str] = None) -> None:
        """createBroker with a BrokerCapacityInfo; disk_capacity_by_logdir populates the replica placement over
        disks (Broker.java:80-83; negative capacity = dead disk). `host` names the broker's host within its rack
        (Rack._hosts); brokers without one get a host of their own."""
        self.create_rack(rack_id)
        if host is not None:
            self.host[broker_id] = str(host)
        self.brokers[broker_id] = (self.rack_index[str(self.mapper(str(rack_id)))],
                                   [float(capacity[r]) for r in RESOURCES])
        for logdir, cap in (disk_capacity_by_logdir or {}).items():
            self.disk_index[(broker_id, logdir)] = len(self.disks)
            self.disks.append((broker_id, logdir, float(cap)))

    def _replica(self, broker_id: int, topic: str, partition: int) -> int:
        for r in self.part_list[self.parts[(topic, partition)]]:
            if self.rep_broker[r] == broker_id:
                return r
        raise IllegalArgumentException(f"no replica of {topic}-{partition} on broker {broker_id}")

    def create_replica(self, rack_id: str, broker_id: int, topic: str, partition: int, index: int, is_leader: bool,
                       is_offline: bool = False, logdir: Optional[str] = None) -> int:
        if topic not in self.topic_index:
            self.topic_index[topic] = len(self.topics)
            self.topics.append(topic)
        key = (topic, partition)
        if key not in self.parts:
            self.parts[key] = len(self.part_list)
            self.part_list.append([])
        r = len(self.rep_part)
        self.rep_part.append(self.parts[key])
        self.rep_broker.append(broker_id)
        self.rep_leader.append(1 if is_leader else 0)
        self.rep_offline.append(1 if is_offline else 0)
        self.rep_load.append(None)
        if logdir is not None and (broker_id, logdir) not in self.disk_index:
            raise IllegalStateException(f"Missing disk information for disk {logdir} on broker {broker_id}")
        self.rep_disk.append(self.disk_index[(broker_id, logdir)] if logdir is not None else -1)
        self.part_list[self.parts[key]].insert(index, r)
        return r

    def set_replica_load(self, rack_id: str, broker_id: int, topic: str, partition: int, cpu: float, nw_in: float,
                         nw_out: float, disk: float) -> None:
        r = self._replica(broker_id, topic, partition)
        if self.rep_load[r] is not None:
            raise IllegalStateException(f"The load for {topic}-{partition} on broker {broker_id} already has metric values.")
        load = [0.0] * 6
        for res, v in (("CPU", cpu), ("NW_IN", nw_in), ("NW_OUT", nw_out), ("DISK", disk)):
            load[METRIC_OF_RESOURCE[res]] = float(v)
        self.rep_load[r] = load
        self.load_order.append(r)

    def set_broker_state(self, broker_id: int, state: str) -> None:
        self.state[broker_id] = BROKER_STATES[state]

    def set_disk_state(self, broker_id: int, logdir: str, state: str) -> None:
        """Disk.setState: "DEMOTED" or "ALIVE" (DemoteBrokerRunnable.java:144-148)."""
        if (broker_id, logdir) not in self.disk_index:
            raise IllegalStateException(f"Broker {broker_id} does not have logdir {logdir}.")
        if state not in ("ALIVE", "DEMOTED"):
            raise IllegalArgumentException(f"unsupported disk state {state}")
        self.disk_demoted[self.disk_index[(broker_id, logdir)]] = 1 if state == "DEMOTED" else 0

    def build(self) -> "FlatCluster":
        return FlatCluster(self)


class FlatCluster:
    """Owner of the arrays behind a ClusterModelBuilder's desc (keep it alive while sessions use the desc)."""

    def __init__(self, bld: ClusterModelBuilder):
        B = len(bld.brokers)
        if sorted(bld.brokers) != list(range(B)):
            raise IllegalArgumentException("broker ids must be 0..B-1")
        R, P, T, W = len(bld.rep_part), len(bld.part_list), len(bld.topics), bld.W
        # a replica without setReplicaLoad keeps an empty Load (it is left out of replica_load_order)
        arr = lambda ct, xs: (ct * max(1, len(xs)))(*xs)  # noqa: E731
        self.keep = dict(
            broker_id=arr(C.c_int32, list(range(B))),
            broker_rack=arr(C.c_int32, [bld.brokers[b][0] for b in range(B)]),
            broker_state=arr(C.c_int32, [bld.state.get(b, 0) for b in range(B)]),
            broker_capacity=arr(C.c_double, [c for b in range(B) for c in bld.brokers[b][1]]),
            topic_names=arr(C.c_char_p, [t.encode() for t in bld.topics]),
            partition_topic=arr(C.c_int32, [0] * P), partition_number=arr(C.c_int32, [0] * P),
            partition_offset=arr(C.c_int32, [0] * (P + 1)),
            partition_replicas=arr(C.c_int32, [r for lst in bld.part_list for r in lst]),
            replica_partition=arr(C.c_int32, bld.rep_part), replica_broker=arr(C.c_int32, bld.rep_broker),
            replica_is_leader=arr(C.c_uint8, bld.rep_leader), replica_offline=arr(C.c_uint8, bld.rep_offline),
            replica_load=arr(C.c_float, [x for r in range(R) for x in (bld.rep_load[r] or [0.0] * 6) for _ in range(W)]),
            replica_load_order=arr(C.c_int32, bld.load_order))
        D = len(bld.disks)
        if D:
            self.keep.update(disk_broker=arr(C.c_int32, [x[0] for x in bld.disks]),
                             disk_logdir=arr(C.c_char_p, [x[1].encode() for x in bld.disks]),
                             disk_capacity=arr(C.c_double, [x[2] for x in bld.disks]),
                             replica_disk=arr(C.c_int32, bld.rep_disk),
                             disk_demoted=arr(C.c_uint8, [bld.disk_demoted.get(k, 0) for k in range(D)]))
        if bld.host:  # one host per (rack, name); a broker without a name is alone on its host
            index: Dict[tuple, int] = {}
            hosts = []
            for b in range(B):
                key = (bld.brokers[b][0], bld.host[b]) if b in bld.host else ("own", b)
                hosts.append(index.setdefault(key, len(index)))
            self.keep["broker_host"] = arr(C.c_int32, hosts)
        for (topic, num), p in bld.parts.items():
            self.keep["partition_topic"][p] = bld.topic_index[topic]
            self.keep["partition_number"][p] = num
        off = 0
        for p, lst in enumerate(bld.part_list):
            self.keep["partition_offset"][p] = off
            off += len(lst)
        self.keep["partition_offset"][P] = off
        d = ClusterDesc()
        d.num_windows, d.num_racks, d.num_brokers = W, len(bld.rack_index), B
        d.num_topics, d.num_partitions, d.num_replicas = T, P, R
        d.num_disks = D
        d.num_replica_loads = len(bld.load_order)
        for k, v in self.keep.items():
            setattr(d, k, C.cast(v, type(getattr(d, k))) if k not in ("topic_names", "disk_logdir") else v)
        self.desc = d
        self.topics = list(bld.topics)
        self.partitions = {p: key for key, p in bld.parts.items()}
        self._rack_names = {i: name for name, i in bld.rack_index.items()}
        self._host_names = ({self.keep["broker_host"][b]: bld.host[b] for b in range(B) if b in bld.host}
                            if bld.host else {})

    def stats_names(self):
        """Rack ids by rack index and host names by host index (a broker created without a host has none)."""
        return dict(self._rack_names), dict(self._host_names)


class LoadMonitorModel:
    """Model ingestion through the native builder (ccmi_builder_*): the calls LoadMonitor.clusterModel makes
    (monitor/LoadMonitor.java:491-543) — createRack/createBroker for every live node, handleDeadBroker for the brokers
    only partitions name, MonitorUtils.populatePartitionLoad per partition with its aggregated leader metrics, and
    setBadBrokerState — produce the flattened model directly. Replica loads are derived natively
    (getAggregatedMetricValues: CPU to percentage, replication bytes out, follower NW_OUT / CPU).

        m = LoadMonitorModel(num_windows=2)
        m.create_broker("r0", "h0", 0, {"CPU": 100, "NW_IN": 1e5, "NW_OUT": 1e5, "DISK": 1e6})
        m.populate_partition("T0", 0, replicas=[0, 1], leader=0, metrics={"CPU_USAGE": [0.115, 0.015], ...})
        cm = ClusterModel(m.desc(), keepalive=m)
    """

    METRICS = ("CPU_USAGE", "DISK_USAGE", "LEADER_BYTES_IN", "LEADER_BYTES_OUT", "REPLICATION_BYTES_IN_RATE",
               "REPLICATION_BYTES_OUT_RATE")

    def __init__(self, num_windows: int = 1, lib: Optional[Library] = None):
        self.lib = lib or Library.get()
        self.W = num_windows
        h = C.c_void_p()
        self.lib.check(self.lib.lib.ccmi_builder_create(num_windows, C.byref(h)))
        self.handle = h
        self._desc = None
        self._names: Dict[int, tuple] = {}  # broker id -> (rack, host) as createBroker received them

    def stats_names(self):
        """Rack ids by rack index and host names by host index, for the brokers create_broker named (a broker only
        partitions name has neither)."""
        d = self.desc()
        racks: Dict[int, str] = {}
        hosts: Dict[int, str] = {}
        for b, bid in enumerate(self.broker_ids()):
            if bid in self._names:
                racks[d.broker_rack[b]] = self._names[bid][0]
                hosts[d.broker_host[b] if d.broker_host else b] = self._names[bid][1]
        return racks, hosts

    def __del__(self):
        try:
            self.lib.lib.ccmi_builder_destroy(self.handle)
        except Exception:
            pass

    def create_broker(self, rack: str, host: str, broker_id: int, capacity: Dict[str, float],
                      alive: bool = True, disk_capacity_by_logdir: Optional[Dict[str, float]] = None) -> None:
        cap = (C.c_double * 4)(*[float(capacity[r]) for r in RESOURCES])
        self.lib.check(self.lib.lib.ccmi_builder_create_broker(self.handle, rack.encode(), host.encode(), broker_id,
                                                               cap, 1 if alive else 0))
        self._names[broker_id] = (rack, host)
        for logdir, c in (disk_capacity_by_logdir or {}).items():
            self.lib.check(self.lib.lib.ccmi_builder_add_disk(self.handle, broker_id, logdir.encode(), float(c)))

    def populate_partition(self, topic: str, partition: int, replicas: Sequence[int], leader: Optional[int],
                           metrics: Dict[str, Sequence[float]], offline: Sequence[int] = (),
                           logdirs: Optional[Sequence[Optional[str]]] = None) -> None:
        """metrics: aggregated leader values per metric name, newest window first (missing metrics are 0)."""
        n = len(replicas)
        vals = []
        for m in self.METRICS:
            w = list(metrics.get(m, [0.0] * self.W))
            if len(w) != self.W:
                raise IllegalArgumentException(f"{m}: {len(w)} windows, expected {self.W}")
            vals += [float(x) for x in w]
        off = (C.c_uint8 * n)(*[1 if b in set(offline) else 0 for b in replicas])
        ld = (C.c_char_p * n)(*[(x.encode() if x else None) for x in logdirs]) if logdirs else None
        self.lib.check(self.lib.lib.ccmi_builder_populate_partition(
            self.handle, topic.encode(), partition, (C.c_int32 * n)(*replicas), n,
            -1 if leader is None else leader, off, ld, (C.c_float * len(vals))(*vals)))
        self._desc = None

    def populate_from_aggregator(self, agg: "MetricSampleAggregator", from_ms: int, to_ms: int,
                                 options: "AggregationOptions", topology: "PartitionTopology", interested=None,
                                 metric_of: Optional[Sequence[int]] = None) -> "AggregatorCompleteness":
        """ccmi_builder_populate_from_aggregator: agg.aggregate(from_ms, to_ms, options, interested) and
        populate_partition for every row of it in one device call; entity e of the aggregator is partition e of
        `topology`. -> the aggregate's completeness, with `num_rows` (rows of the aggregate) and `num_populated`
        (partitions added). `metric_of`: the aggregator's metric index of each of METRICS, by default their places in
        KAFKA_COMMON_METRICS. On an error nothing is added."""
        import numpy as np

        if not self.lib.has_load_model:
            raise UnsupportedOperationException(f"{self.lib.path} does not export "
                                                "ccmi_builder_populate_from_aggregator: the bulk load runs on the "
                                                "device only")
        if metric_of is None:
            names = [n for n, _ in KAFKA_COMMON_METRICS]
            metric_of = [names.index(m) for m in self.METRICS]
        if len(metric_of) != len(self.METRICS):
            raise IllegalArgumentException("metric_of has one entry per builder metric")
        s, arrays = agg._completeness_struct(np)
        mask = agg._mask(np, interested)
        o = options.struct()
        rows, populated = C.c_int64(0), C.c_int64(0)
        t = topology.struct()
        self.lib.check(self.lib.lib.ccmi_builder_populate_from_aggregator(
            self.handle, agg.handle, from_ms, to_ms, C.byref(o), mask.ctypes.data if mask is not None else None,
            (C.c_int32 * len(metric_of))(*metric_of), C.byref(t), C.byref(s), C.byref(rows), C.byref(populated)))
        self._desc = None
        c = AggregatorCompleteness(np, s, arrays)
        c.num_rows, c.num_populated = int(rows.value), int(populated.value)
        return c

    def set_broker_state(self, broker_id: int, state: str) -> None:
        self.lib.check(self.lib.lib.ccmi_builder_set_broker_state(self.handle, broker_id, BROKER_STATES[state]))
        self._desc = None

    def set_disk_state(self, broker_id: int, logdir: str, state: str) -> None:
        """Disk.setState (DemoteBrokerRunnable.java:144-148): "ALIVE" or "DEMOTED"."""
        self.lib.check(self.lib.lib.ccmi_builder_set_disk_state(self.handle, broker_id, logdir.encode(),
                                                                DISK_STATES[state]))
        self._desc = None

    def desc(self) -> ClusterDesc:
        if self._desc is None:
            d = ClusterDesc()
            self.lib.check(self.lib.lib.ccmi_builder_desc(self.handle, C.byref(d)))
            self._desc = d
        return self._desc

    def broker_ids(self) -> List[int]:
        """Kafka broker id of every dense broker index of desc()."""
        d = self.desc()
        out = (C.c_int32 * d.num_brokers)()
        self.lib.check(self.lib.lib.ccmi_builder_broker_ids(self.handle, out))
        return list(out)

    def replica_loads(self) -> List[List[List[float]]]:
        """[replica][metric][window] of the flattened model (the values setReplicaLoad received)."""
        d = self.desc()
        W = d.num_windows
        return [[[d.replica_load[(r * 6 + m) * W + w] for w in range(W)] for m in range(6)]
                for r in range(d.num_replicas)]


@dataclass
class AggregationOptions:
    """monitor/sampling/aggregator/AggregationOptions.java without the interested entities (a mask of the calls)."""
    min_valid_entity_ratio: float = 0.0
    min_valid_entity_group_ratio: float = 0.0
    min_valid_windows: int = 1
    max_allowed_extrapolations_per_entity: int = 5
    granularity: int = GRANULARITY_ENTITY
    include_invalid_entities: bool = False

    def struct(self) -> AggregationOptionsStruct:
        return AggregationOptionsStruct(float(self.min_valid_entity_ratio), float(self.min_valid_entity_group_ratio),
                                        int(self.min_valid_windows), int(self.max_allowed_extrapolations_per_entity),
                                        int(self.granularity), 1 if self.include_invalid_entities else 0)


class AggregatorCompleteness:
    """MetricSampleCompleteness as ccmi_aggregator_completeness returns it: numpy arrays over the walked windows, newest
    first (`windows` holds their indices, `included` which of them are valid window indices), the totals, the two
    overall float ratios, and `failure` (AGG_FAILURE_*, set by aggregate only)."""

    def __init__(self, np, s: AggregatorCompletenessStruct, arrays, valid_entities=None, valid_groups=None):
        n = s.num_windows
        self.generation = s.generation
        self.failure = s.failure
        self.windows, self.included = arrays[0][:n].copy(), arrays[1][:n].copy()
        self.valid_entity_ratio_by_window = arrays[2][:n].copy()
        self.valid_entity_ratio_with_group_granularity_by_window = arrays[3][:n].copy()
        self.valid_entity_group_ratio_by_window = arrays[4][:n].copy()
        self.extrapolated_entity_ratio_by_window = arrays[5][:n].copy()
        self.valid_window_indices = self.windows[self.included != 0]
        self.num_interested_entities, self.num_interested_groups = s.num_interested_entities, s.num_interested_groups
        self.num_valid_entities, self.num_valid_groups = s.num_valid_entities, s.num_valid_groups
        self.valid_entity_ratio = np.float32(s.valid_entity_ratio)
        self.valid_entity_group_ratio = np.float32(s.valid_entity_group_ratio)
        self.valid_entities, self.valid_groups = valid_entities, valid_groups  # uint8 masks, completeness() only


class PartitionTopology:
    """ccmi_partition_topology: what Cluster.partition(tp) answers for every entity of a partition aggregator, as numpy
    arrays plus the name lists. Partition e has topic topic_names[partition_topic[e]], number partition_number[e], the
    replica brokers replica_broker_id[replica_offset[e]:replica_offset[e + 1]] in PartitionInfo.replicas() order (an
    empty range: the partition is unknown to the metadata and is skipped) and the leader leader_broker_id[e] (-1: offline).
    replica_offline (bytes) and replica_logdir (indices into logdir_names, -1 = none) are optional."""

    def __init__(self, topic_names: Sequence[str], partition_topic, partition_number, replica_offset, replica_broker_id,
                 leader_broker_id, replica_offline=None, replica_logdir=None, logdir_names: Sequence[str] = ()):
        import numpy as np

        def arr(a, dtype):
            return None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(-1)

        self.topic_names, self.logdir_names = [str(n) for n in topic_names], [str(n) for n in logdir_names]
        self.partition_topic, self.partition_number = arr(partition_topic, np.int32), arr(partition_number, np.int32)
        self.replica_offset, self.replica_broker_id = arr(replica_offset, np.int32), arr(replica_broker_id, np.int32)
        self.leader_broker_id = arr(leader_broker_id, np.int32)
        self.replica_offline, self.replica_logdir = arr(replica_offline, np.uint8), arr(replica_logdir, np.int32)
        P = int(self.partition_topic.size)
        R = int(self.replica_broker_id.size)
        if self.partition_number.size != P or self.leader_broker_id.size != P or self.replica_offset.size != P + 1:
            raise IllegalArgumentException("the per-partition arrays disagree on the number of partitions")
        if int(self.replica_offset[-1]) != R or any(a is not None and a.size != R
                                                    for a in (self.replica_offline, self.replica_logdir)):
            raise IllegalArgumentException("the per-replica arrays disagree with replica_offset")
        self.num_partitions, self.num_replicas = P, R

    def struct(self) -> PartitionTopologyStruct:
        """The C struct over this object's arrays (which it keeps alive: hold the object while the struct is in use)."""
        def ptr(a, ctype):
            return None if a is None else a.ctypes.data_as(C.POINTER(ctype))

        self._topic_c = (C.c_char_p * max(1, len(self.topic_names)))(*[n.encode() for n in self.topic_names])
        self._logdir_c = (C.c_char_p * max(1, len(self.logdir_names)))(*[n.encode() for n in self.logdir_names])
        return PartitionTopologyStruct(
            self.num_partitions, len(self.topic_names), len(self.logdir_names), 0, self._topic_c,
            ptr(self.partition_topic, C.c_int32), ptr(self.partition_number, C.c_int32),
            ptr(self.replica_offset, C.c_int32), ptr(self.replica_broker_id, C.c_int32),
            ptr(self.leader_broker_id, C.c_int32), ptr(self.replica_offline, C.c_uint8),
            ptr(self.replica_logdir, C.c_int32), self._logdir_c if self.logdir_names else None)


class AggregationResult:
    """MetricSampleAggregationResult: `entities` (ascending ids, the first `capacity` of `num_entities`), `values`
    float32 [k][M][Wv] and `extrapolations` uint8 [k][Wv] over the valid windows newest first, `invalid` uint8 [k]."""

    def __init__(self, completeness, num_entities, entities, values, extrapolations, invalid):
        self.completeness, self.num_entities = completeness, num_entities
        self.entities, self.values, self.extrapolations, self.invalid = entities, values, extrapolations, invalid

    def leader_metrics(self, row: int):
        """Row `row` of an aggregate over KAFKA_COMMON_METRICS as ccmi_builder_populate_partition's leader_metrics:
        [6 * Wv] floats in ccmi_metric order, newest window first."""
        import numpy as np

        if self.values.shape[1] != len(KAFKA_COMMON_METRICS):
            raise IllegalArgumentException("the aggregator's metrics are not KafkaMetricDef's common metrics")
        names = [n for n, _ in KAFKA_COMMON_METRICS]
        pick = [names.index(m) for m in LoadMonitorModel.METRICS]
        return np.ascontiguousarray(self.values[row][pick], dtype=np.float32).reshape(-1)

    def populate_partition(self, model: "LoadMonitorModel", row: int, topic: str, partition: int,
                           replicas: Sequence[int], leader: Optional[int], **kwargs) -> None:
        """LoadMonitorModel.populate_partition with the aggregated leader metrics of row `row`."""
        wv = self.values.shape[2]
        flat = self.leader_metrics(row)
        model.populate_partition(topic, partition, replicas, leader,
                                 {m: flat[i * wv:(i + 1) * wv] for i, m in enumerate(LoadMonitorModel.METRICS)},
                                 **kwargs)


class MetricSampleAggregator:
    """MetricSampleAggregator on the device (ccmi_aggregator_*): the step before LoadMonitorModel. Entities are dense ids
    with a group each (for partitions the topic); metric m has metric_functions[m] (AGG_AVG / AGG_MAX / AGG_LATEST).

        agg = MetricSampleAggregator(5, 300_000, 4, [f for _, f in KAFKA_COMMON_METRICS], topic_of_partition)
        agg.add_samples(partition_ids, times_ms, values)          # values: [n][M] doubles
        res = agg.aggregate(-1, now_ms, AggregationOptions(0.95, 0.0, 1, 5, GRANULARITY_ENTITY_GROUP, True))
        res.populate_partition(model, row, topic, partition, replicas, leader)
    """

    def __init__(self, num_windows: int, window_ms: int, min_samples_per_window: int,
                 metric_functions: Sequence[int], entity_group: Sequence[int], num_groups: Optional[int] = None,
                 device: int = 0, lib: Optional[Library] = None):
        import numpy as np

        self.lib = lib or Library.get()
        self.handle = None
        if not self.lib.has_aggregator:
            raise UnsupportedOperationException(f"{self.lib.path} does not export ccmi_aggregator_create: the "
                                                "aggregator runs on the device only")
        fn = np.ascontiguousarray(metric_functions, dtype=np.uint8)
        grp = np.ascontiguousarray(entity_group, dtype=np.int32)
        self.num_windows, self.window_ms, self.min_samples_per_window = num_windows, window_ms, min_samples_per_window
        self.M, self.E = int(fn.size), int(grp.size)
        self.G = int(num_groups) if num_groups is not None else (int(grp.max()) + 1 if grp.size else 0)
        cfg = AggregatorConfigStruct(window_ms, num_windows, min_samples_per_window, self.M, self.E, self.G, 0)
        h = C.c_void_p()
        self.lib.check(self.lib.lib.ccmi_aggregator_create(device, C.byref(cfg), fn.ctypes.data, grp.ctypes.data,
                                                           C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if self.handle:
                self.lib.lib.ccmi_aggregator_destroy(self.handle)
        except Exception:
            pass

    def add_samples(self, entities, times_ms, values):
        """MetricSampleAggregator.addSample for every sample in order; -> uint8 accepted flags."""
        import numpy as np

        ent = np.ascontiguousarray(entities, dtype=np.int32).reshape(-1)
        tms = np.ascontiguousarray(times_ms, dtype=np.int64).reshape(-1)
        val = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        n = int(ent.size)
        if tms.size != n or val.size != n * self.M:
            raise IllegalArgumentException("entities, times_ms and values disagree on the number of samples")
        accepted = np.zeros(n, dtype=np.uint8)
        num = C.c_int64(0)
        self.lib.check(self.lib.lib.ccmi_aggregator_add_samples(self.handle, ent.ctypes.data, tms.ctypes.data,
                                                                val.ctypes.data, n, accepted.ctypes.data, C.byref(num)))
        return accepted

    def state(self) -> AggregatorStateStruct:
        s = AggregatorStateStruct()
        self.lib.check(self.lib.lib.ccmi_aggregator_state_query(self.handle, C.byref(s)))
        return s

    generation = property(lambda self: self.state().generation)
    oldest_window_index = property(lambda self: self.state().oldest_window_index)
    current_window_index = property(lambda self: self.state().current_window_index)
    num_samples = property(lambda self: self.state().num_samples)
    num_available_windows = property(lambda self: self.state().num_available_windows)
    num_present_entities = property(lambda self: self.state().num_present_entities)

    def _completeness_struct(self, np):
        cap = self.num_windows + 1
        arrays = [np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.uint8)] + \
                 [np.zeros(cap, dtype=np.float32) for _ in range(4)]
        s = AggregatorCompletenessStruct()
        s.window_capacity = cap
        s.window_index = arrays[0].ctypes.data_as(C.POINTER(C.c_int64))
        s.window_included = arrays[1].ctypes.data_as(C.POINTER(C.c_uint8))
        s.valid_entity_ratio_by_window = arrays[2].ctypes.data_as(C.POINTER(C.c_float))
        s.valid_entity_ratio_with_group_granularity_by_window = arrays[3].ctypes.data_as(C.POINTER(C.c_float))
        s.valid_entity_group_ratio_by_window = arrays[4].ctypes.data_as(C.POINTER(C.c_float))
        s.extrapolated_entity_ratio_by_window = arrays[5].ctypes.data_as(C.POINTER(C.c_float))
        return s, arrays

    def _mask(self, np, interested):
        if interested is None:
            return None
        m = np.ascontiguousarray(interested, dtype=np.uint8).reshape(-1)
        if m.size != self.E:
            raise IllegalArgumentException("the interested mask has one byte per entity")
        return m

    def completeness(self, from_ms: int, to_ms: int, options: AggregationOptions, interested=None,
                     masks: bool = True) -> AggregatorCompleteness:
        """MetricSampleAggregator.completeness; `interested` is a byte mask over the entities (None, or nothing
        selected: every present entity). With `masks` the valid entities and groups come back as uint8 masks."""
        import numpy as np

        s, arrays = self._completeness_struct(np)
        mask = self._mask(np, interested)
        ve = np.zeros(self.E, dtype=np.uint8) if masks else None
        vg = np.zeros(self.G, dtype=np.uint8) if masks else None
        o = options.struct()
        self.lib.check(self.lib.lib.ccmi_aggregator_completeness_query(
            self.handle, from_ms, to_ms, C.byref(o), mask.ctypes.data if mask is not None else None, C.byref(s),
            ve.ctypes.data if masks else None, vg.ctypes.data if masks else None))
        return AggregatorCompleteness(np, s, arrays, ve, vg)

    def aggregate(self, from_ms: int, to_ms: int, options: AggregationOptions, interested=None,
                  capacity: Optional[int] = None) -> AggregationResult:
        """MetricSampleAggregator.aggregate. NotEnoughValidWindowsException is an expected outcome: the result then has
        completeness.failure set and no rows. `capacity` cuts the rows (num_entities is always the full count)."""
        import numpy as np

        s, arrays = self._completeness_struct(np)
        mask = self._mask(np, interested)
        cap = self.E if capacity is None else int(capacity)
        wmax = self.num_windows
        ent = np.zeros(cap, dtype=np.int32)
        val = np.zeros(cap * self.M * wmax, dtype=np.float32)
        ext = np.zeros(cap * wmax, dtype=np.uint8)
        inv = np.zeros(cap, dtype=np.uint8)
        n = C.c_int64(0)
        o = options.struct()
        self.lib.check(self.lib.lib.ccmi_aggregator_aggregate(
            self.handle, from_ms, to_ms, C.byref(o), mask.ctypes.data if mask is not None else None, C.byref(s),
            ent.ctypes.data, val.ctypes.data, ext.ctypes.data, inv.ctypes.data, cap, C.byref(n)))
        k, wv = min(cap, n.value), s.num_valid_windows
        return AggregationResult(AggregatorCompleteness(np, s, arrays), int(n.value), ent[:k],
                                 val[:k * self.M * wv].reshape(k, self.M, wv), ext[:k * wv].reshape(k, wv), inv[:k])

    def peek_current_window(self, capacity: Optional[int] = None):
        """peekCurrentWindow: -> (entities ascending, values float32 [k][M], extrapolations uint8 [k], num_entities)."""
        import numpy as np

        cap = self.E if capacity is None else int(capacity)
        ent = np.zeros(cap, dtype=np.int32)
        val = np.zeros(cap * self.M, dtype=np.float32)
        ext = np.zeros(cap, dtype=np.uint8)
        n = C.c_int64(0)
        self.lib.check(self.lib.lib.ccmi_aggregator_peek_current_window(self.handle, ent.ctypes.data, val.ctypes.data,
                                                                        ext.ctypes.data, cap, C.byref(n)))
        k = min(cap, n.value)
        return ent[:k], val[:k * self.M].reshape(k, self.M), ext[:k], int(n.value)

    def remove_entities(self, entities) -> None:
        import numpy as np

        ids = np.ascontiguousarray(entities, dtype=np.int32).reshape(-1)
        self.lib.check(self.lib.lib.ccmi_aggregator_remove_entities(self.handle, ids.ctypes.data, int(ids.size)))

    def clear(self) -> None:
        self.lib.check(self.lib.lib.ccmi_aggregator_clear(self.handle))

    def metric_anomalies(self, to_ms: int, interested_metrics, upper_percentile: float = 95.0,
                         lower_percentile: float = 2.0, upper_margin: float = 0.5, lower_margin: float = 0.2,
                         from_ms: int = -1, options: Optional[AggregationOptions] = None, interested=None,
                         capacity: Optional[int] = None) -> "MetricAnomalies":
        """PercentileMetricAnomalyFinder.metricAnomalies over this (broker) aggregator on the device
        (ccmi_aggregator_metric_anomalies): the history is aggregate(from_ms, to_ms, options, interested), by default
        KafkaBrokerMetricSampleAggregator's (ratios 0.0 / 0.0, one valid window, ENTITY, valid entities only, from -1),
        the current values are peek_current_window's. `interested_metrics` is a byte mask over the M metrics. The
        percentile and margin defaults are AnomalyDetectorConfig's."""
        import numpy as np

        if not self.lib.has_metric_anomalies:
            raise UnsupportedOperationException(f"{self.lib.path} does not export ccmi_aggregator_metric_anomalies: "
                                                "the anomaly finders run on the device only")
        s, arrays = self._completeness_struct(np)
        mask = self._mask(np, interested)
        metrics = np.ascontiguousarray(interested_metrics, dtype=np.uint8).reshape(-1)
        if metrics.size != self.M:
            raise IllegalArgumentException("the interested metrics mask has one byte per metric")
        cap = self.E * int(np.count_nonzero(metrics)) if capacity is None else int(capacity)
        rec = np.zeros(max(cap, 0), dtype=METRIC_ANOMALY_DTYPE)  # a negative capacity is the library's to refuse
        o = (options or AggregationOptions(0.0, 0.0, 1, 5, GRANULARITY_ENTITY, False)).struct()
        cfg = MetricAnomalyConfigStruct(float(upper_percentile), float(lower_percentile), float(upper_margin),
                                        float(lower_margin))
        n, window = C.c_int64(0), C.c_int64(0)
        self.lib.check(self.lib.lib.ccmi_aggregator_metric_anomalies(
            self.handle, from_ms, to_ms, C.byref(o), mask.ctypes.data if mask is not None else None, C.byref(cfg),
            metrics.ctypes.data, C.byref(s), C.byref(window), rec.ctypes.data if cap else None, cap, C.byref(n)))
        return MetricAnomalies(AggregatorCompleteness(np, s, arrays), int(window.value), int(n.value),
                               rec[:max(0, min(cap, n.value))])


def _record_dtype(struct):
    """The numpy dtype of a ctypes record struct (explicit offsets, the struct's size)."""
    import numpy as np

    kinds = {C.c_int32: np.int32, C.c_int64: np.int64, C.c_double: np.float64}
    return np.dtype({"names": [n for n, _ in struct._fields_], "formats": [kinds[t] for _, t in struct._fields_],
                     "offsets": [getattr(struct, n).offset for n, _ in struct._fields_],
                     "itemsize": C.sizeof(struct)})


try:
    METRIC_ANOMALY_DTYPE = _record_dtype(MetricAnomalyStruct)
    SLOW_BROKER_DTYPE = _record_dtype(SlowBrokerStruct)
except ImportError:  # numpy is needed only by the array-shaped calls
    METRIC_ANOMALY_DTYPE = SLOW_BROKER_DTYPE = None


class MetricAnomalies:
    """What ccmi_aggregator_metric_anomalies returns: `completeness` of the history aggregate (its failure set when
    there was none), `current_window_index`, `num_anomalies` (numAnomaliesOfType(RECENT)) and `records`, a numpy record
    array (entity, metric, current, upper_threshold, lower_threshold) in ascending (entity, metric) order, the first
    `capacity` of them."""

    def __init__(self, completeness, current_window_index, num_anomalies, records):
        self.completeness, self.current_window_index = completeness, current_window_index
        self.num_anomalies, self.records = num_anomalies, records


class SlowBrokerDetection:
    """One ccmi_slow_broker_finder_detect: `completeness`, `summary` (SlowBrokerSummaryStruct), `num_brokers`,
    `brokers` (numpy records entity, kind, score, since_ms; kind SLOW_BROKER_DEMOTE / SLOW_BROKER_REMOVE) and
    `diagnostics` (uint8 [E] of SLOW_DIAG_* bits, or None)."""

    def __init__(self, completeness, summary, num_brokers, brokers, diagnostics):
        self.completeness, self.summary, self.num_brokers = completeness, summary, num_brokers
        self.brokers, self.diagnostics = brokers, diagnostics


class SlowBrokerFinder:
    """SlowBrokerFinder with its slowness scores on the device (ccmi_slow_broker_finder_*), bound to one broker
    MetricSampleAggregator, which it keeps alive. The keyword defaults are the reference's.

        finder = SlowBrokerFinder(agg, log_flush_metric, leader_bytes_in_metric, replication_bytes_in_metric)
        d = finder.detect(now_ms)          # one metricAnomalies round at time now_ms
        d.brokers, d.summary.unfixable, finder.scores()
    """

    def __init__(self, aggregator: MetricSampleAggregator, log_flush_metric: int, leader_bytes_in_metric: int,
                 replication_bytes_in_metric: int, bytes_in_rate_detection_threshold: float = 1024.0,
                 log_flush_time_threshold_ms: float = 1000.0, metric_history_percentile: float = 90.0,
                 metric_history_margin: float = 3.0, peer_metric_percentile: float = 50.0,
                 peer_metric_margin: float = 3.0, demotion_score: int = 5, decommission_score: int = 50,
                 self_healing_unfixable_ratio: float = 0.1, removal_enabled: bool = False):
        self.aggregator, self.lib = aggregator, aggregator.lib
        self.handle = None
        if not self.lib.has_metric_anomalies:
            raise UnsupportedOperationException(f"{self.lib.path} does not export ccmi_slow_broker_finder_create: "
                                                "the anomaly finders run on the device only")
        cfg = SlowBrokerConfigStruct(float(bytes_in_rate_detection_threshold), float(log_flush_time_threshold_ms),
                                     float(metric_history_percentile), float(metric_history_margin),
                                     float(peer_metric_percentile), float(peer_metric_margin),
                                     float(self_healing_unfixable_ratio), int(demotion_score), int(decommission_score),
                                     int(log_flush_metric), int(leader_bytes_in_metric),
                                     int(replication_bytes_in_metric), 1 if removal_enabled else 0)
        h = C.c_void_p()
        self.lib.check(self.lib.lib.ccmi_slow_broker_finder_create(aggregator.handle, C.byref(cfg), C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if self.handle:
                self.lib.lib.ccmi_slow_broker_finder_destroy(self.handle)
        except Exception:
            pass

    def detect(self, time_ms: int, to_ms: Optional[int] = None, from_ms: int = -1,
               options: Optional[AggregationOptions] = None, interested=None, capacity: Optional[int] = None,
               diagnostics: bool = False) -> SlowBrokerDetection:
        """SlowBrokerFinder.metricAnomalies at _kafkaCruiseControl.timeMs() == time_ms; the history range ends at
        to_ms (by default time_ms). Every call is one round of the score update."""
        import numpy as np

        agg = self.aggregator
        s, arrays = agg._completeness_struct(np)
        mask = agg._mask(np, interested)
        cap = agg.E if capacity is None else int(capacity)
        rec = np.zeros(max(cap, 0), dtype=SLOW_BROKER_DTYPE)
        diag = np.zeros(agg.E, dtype=np.uint8) if diagnostics else None
        o = (options or AggregationOptions(0.0, 0.0, 1, 5, GRANULARITY_ENTITY, False)).struct()
        summary = SlowBrokerSummaryStruct()
        n = C.c_int64(0)
        self.lib.check(self.lib.lib.ccmi_slow_broker_finder_detect(
            self.handle, from_ms, time_ms if to_ms is None else to_ms, C.byref(o),
            mask.ctypes.data if mask is not None else None, time_ms, C.byref(s), C.byref(summary),
            rec.ctypes.data if cap else None, cap, C.byref(n), diag.ctypes.data if diagnostics else None))
        return SlowBrokerDetection(AggregatorCompleteness(np, s, arrays), summary, int(n.value),
                                   rec[:max(0, min(cap, n.value))], diag)

    def scores(self, capacity: Optional[int] = None):
        """-> numpy records (entity, kind 0, score, since_ms) of the scored entities, ascending."""
        import numpy as np

        cap = self.aggregator.E if capacity is None else int(capacity)
        rec = np.zeros(max(cap, 0), dtype=SLOW_BROKER_DTYPE)
        n = C.c_int64(0)
        self.lib.check(self.lib.lib.ccmi_slow_broker_finder_scores(self.handle, rec.ctypes.data if cap else None, cap,
                                                                   C.byref(n)))
        return rec[:max(0, min(cap, n.value))]

    def reset(self) -> None:
        self.lib.check(self.lib.lib.ccmi_slow_broker_finder_reset(self.handle))


class ProcessedSamples:
    """What MetricsProcessor.process returns: numpy arrays, see ccmi_processed_samples in include/ccmi.h."""

    def __init__(self, s: ProcessedSamplesStruct, arrays):
        (self.partition_entity, self.partition_values, self.broker_node, self.broker_values, self.broker_version,
         self.partition_skip, self.broker_skip, self.skipped_by_node) = arrays
        self.max_metric_timestamp = int(s.max_metric_timestamp)
        self.num_partition_samples, self.num_broker_samples = int(s.num_partition_samples), int(s.num_broker_samples)
        self.num_skipped_brokers = int(s.num_skipped_brokers)
        self.num_hash_fallback_brokers = int(s.num_hash_fallback_brokers)
        self.num_dropped_records = int(s.num_dropped_records)
        kp = min(self.num_partition_samples, len(self.partition_entity))
        kb = min(self.num_broker_samples, len(self.broker_node))
        self.partition_entity, self.partition_values = self.partition_entity[:kp], self.partition_values[:kp]
        self.broker_node, self.broker_values = self.broker_node[:kb], self.broker_values[:kb]
        self.broker_version = self.broker_version[:kb]


class MetricsProcessor:
    """CruiseControlMetricsProcessor on the device (ccmi_metrics_processor_*): one sampling round's raw records in,
    partition and broker samples out as the rows MetricSampleAggregator.add_samples takes.

        mp = MetricsProcessor()
        mp.add_metrics(types, broker_ids, times_ms, values, topics, partitions, topic_names)
        s = mp.process(topic_names, partition_topic, partition_number, replica_offset, leader_broker_id,
                       node_ids, num_cores)
        partition_agg.add_samples(s.partition_entity, [s.max_metric_timestamp] * len(s.partition_entity),
                                  s.partition_values)
        mp.clear()
    """

    def __init__(self, cpu_weights: Optional[Sequence[float]] = None, device: int = 0, lib: Optional[Library] = None):
        self.lib = lib or Library.get()
        self.handle = None
        if not self.lib.has_metrics_processor:
            raise UnsupportedOperationException(f"{self.lib.path} does not export ccmi_metrics_processor_create: "
                                                "the metrics processor runs on the device only")
        cfg = None
        if cpu_weights is not None:
            a, b, c = (float(x) for x in cpu_weights)
            cfg = C.byref(MetricsProcessorConfigStruct(a, b, c, 0))
        h = C.c_void_p()
        self.lib.check(self.lib.lib.ccmi_metrics_processor_create(device, cfg, C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if self.handle:
                self.lib.lib.ccmi_metrics_processor_destroy(self.handle)
        except Exception:
            pass

    def add_metrics(self, types, broker_ids, times_ms, values, topics, partitions, topic_names: Sequence[str]) -> None:
        """addMetric for every record in order. types: RawMetricType ids (RAW_METRIC_TYPE_ID); topics: index into
        topic_names or -1; partitions: -1 unless PARTITION_SIZE."""
        import numpy as np

        ty = np.ascontiguousarray(types, dtype=np.uint8).reshape(-1)
        br = np.ascontiguousarray(broker_ids, dtype=np.int32).reshape(-1)
        tm = np.ascontiguousarray(times_ms, dtype=np.int64).reshape(-1)
        va = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        to = np.ascontiguousarray(topics, dtype=np.int32).reshape(-1)
        pa = np.ascontiguousarray(partitions, dtype=np.int32).reshape(-1)
        n = int(ty.size)
        if any(int(a.size) != n for a in (br, tm, va, to, pa)):
            raise IllegalArgumentException("the record columns disagree on the number of records")
        names = (C.c_char_p * max(len(topic_names), 1))(*[t.encode() for t in topic_names])
        s = RawMetricsStruct(n, len(topic_names), 0, C.cast(names, C.POINTER(C.c_char_p)), ty.ctypes.data,
                             br.ctypes.data, tm.ctypes.data, va.ctypes.data, to.ctypes.data, pa.ctypes.data)
        self.lib.check(self.lib.lib.ccmi_metrics_processor_add_metrics(self.handle, C.byref(s)))

    def process(self, topic_names: Sequence[str], partition_topic, partition_number, replica_offset,
                leader_broker_id, node_ids, num_cores, interested=None, sampling_mode: int = SAMPLING_ALL,
                partition_capacity: Optional[int] = None, broker_capacity: Optional[int] = None,
                _into=None) -> ProcessedSamples:
        """process(cluster, partitions, samplingMode). The cluster: topic names (with their dots), per partition its
        topic index, number, replica range and leader id (-1: none); the nodes with the resolver's cores (NaN: none)."""
        import numpy as np

        pt = np.ascontiguousarray(partition_topic, dtype=np.int32).reshape(-1)
        pn = np.ascontiguousarray(partition_number, dtype=np.int32).reshape(-1)
        ro = np.ascontiguousarray(replica_offset, dtype=np.int32).reshape(-1)
        ld = np.ascontiguousarray(leader_broker_id, dtype=np.int32).reshape(-1)
        ids = np.ascontiguousarray(node_ids, dtype=np.int32).reshape(-1)
        cores = np.ascontiguousarray(num_cores, dtype=np.float64).reshape(-1)
        P, N = int(pt.size), int(ids.size)
        if pn.size != P or ld.size != P or ro.size != P + 1 or cores.size != N:
            raise IllegalArgumentException("the cluster columns disagree on the number of partitions or nodes")
        mask = None
        if interested is not None:
            mask = np.ascontiguousarray(interested, dtype=np.uint8).reshape(-1)
            if mask.size != P:
                raise IllegalArgumentException("the interested mask has one byte per partition")
        names = (C.c_char_p * max(len(topic_names), 1))(*[t.encode() for t in topic_names])
        topo = PartitionTopologyStruct()
        topo.num_partitions, topo.num_topics = P, len(topic_names)
        topo.topic_names = C.cast(names, C.POINTER(C.c_char_p))
        topo.partition_topic = pt.ctypes.data_as(C.POINTER(C.c_int32))
        topo.partition_number = pn.ctypes.data_as(C.POINTER(C.c_int32))
        topo.replica_offset = ro.ctypes.data_as(C.POINTER(C.c_int32))
        topo.leader_broker_id = ld.ctypes.data_as(C.POINTER(C.c_int32))
        nodes = ClusterNodesStruct(N, 0, ids.ctypes.data, cores.ctypes.data)
        kp = P if partition_capacity is None else int(partition_capacity)
        kb = N if broker_capacity is None else int(broker_capacity)
        arrays = [np.zeros(max(kp, 0), dtype=np.int32), np.zeros((max(kp, 0), 9), dtype=np.float64),
                  np.zeros(max(kb, 0), dtype=np.int32), np.zeros((max(kb, 0), 56), dtype=np.float64),
                  np.zeros(max(kb, 0), dtype=np.int8), np.zeros(P, dtype=np.uint8), np.zeros(N, dtype=np.uint8),
                  np.zeros(N + 1, dtype=np.int32)]
        s = ProcessedSamplesStruct()
        s.partition_capacity, s.broker_capacity = kp, kb
        (s.partition_entity, s.partition_values, s.broker_node, s.broker_values, s.broker_version, s.partition_skip,
         s.broker_skip, s.skipped_by_node) = [a.ctypes.data for a in arrays]
        if _into is not None:
            self.lib.check(self.lib.lib.ccmi_metrics_processor_process_into(
                self.handle, C.byref(topo), C.byref(nodes), mask.ctypes.data if mask is not None else None,
                int(sampling_mode), *[a.handle if a is not None else None for a in _into], C.byref(s)))
            s.partition_capacity = s.broker_capacity = 0  # no rows come back
            return ProcessedSamples(s, [a[:0] for a in arrays[:5]] + arrays[5:])
        self.lib.check(self.lib.lib.ccmi_metrics_processor_process(
            self.handle, C.byref(topo), C.byref(nodes), mask.ctypes.data if mask is not None else None,
            int(sampling_mode), C.byref(s)))
        return ProcessedSamples(s, arrays)

    def process_into(self, topic_names: Sequence[str], partition_topic, partition_number, replica_offset,
                     leader_broker_id, node_ids, num_cores, partition_aggregator: Optional[MetricSampleAggregator],
                     broker_aggregator: Optional[MetricSampleAggregator], interested=None,
                     sampling_mode: int = SAMPLING_ALL) -> ProcessedSamples:
        """process, with the rows fed to the aggregators on the device (either may be None) instead of returned: the
        result has the counts and the skip tables only."""
        return self.process(topic_names, partition_topic, partition_number, replica_offset, leader_broker_id, node_ids,
                            num_cores, interested=interested, sampling_mode=sampling_mode,
                            _into=(partition_aggregator, broker_aggregator))

    def cached_num_cores(self, broker_id: int) -> Optional[float]:
        v = C.c_double(0.0)
        self.lib.check(self.lib.lib.ccmi_metrics_processor_cached_num_cores(self.handle, int(broker_id), C.byref(v)))
        return None if v.value != v.value else v.value

    def clear(self) -> None:
        self.lib.check(self.lib.lib.ccmi_metrics_processor_clear(self.handle))


class ClusterModel:
    """A device-resident model session (ccmi_session)."""

    def __init__(self, desc: ClusterDesc, device: int = 0, lib: Optional[Library] = None, keepalive=None):
        self.lib = lib or Library.get()
        self._keep = keepalive
        self.desc = desc
        h = C.c_void_p()
        self.lib.check(self.lib.lib.ccmi_session_create(device, C.byref(desc), C.byref(h)))
        self.handle = h
        self.num_partitions = desc.num_partitions
        self.num_replicas = desc.num_replicas

    def topic_names(self) -> List[str]:
        return [self.desc.topic_names[t].decode() for t in range(self.desc.num_topics)]

    def broker_ids(self) -> List[int]:
        """Kafka broker id of every broker index: the LoadMonitorModel's id table when the desc came from one
        (ccmi_builder_broker_ids), else the desc's broker_id."""
        if hasattr(self._keep, "broker_ids"):
            return list(self._keep.broker_ids())
        return [self.desc.broker_id[b] for b in range(self.desc.num_brokers)]

    @staticmethod
    def from_buffers(buf: ClusterBuffers, device: int = 0) -> "ClusterModel":
        return ClusterModel(buf.desc, device=device, lib=buf.lib, keepalive=buf)

    def close(self) -> None:
        if self.handle:
            self.lib.lib.ccmi_session_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _goal_optimize(self, goal: Goal, optimized_goals: Iterable[Goal],
                       options: Optional[OptimizationOptions]) -> GoalResultStruct:
        res = GoalResultStruct()
        o, keep = (options or OptimizationOptions()).to_struct()
        c = (goal.constraint or BalancingConstraint()).to_struct(self.topic_names(), self.broker_ids())
        prior = [g.kind if isinstance(g, Goal) else int(g) for g in optimized_goals]
        kinds = (C.c_int32 * max(1, len(prior)))(*prior)
        self._checked(self.lib.lib.ccmi_goal_optimize(self.handle, goal.kind, kinds, len(prior), C.byref(c),
                                                      C.byref(o), C.byref(res)))
        goal.provision = ProvisionResponse.from_struct(res.provision, goal.name())
        return res

    def _checked(self, status: int) -> None:
        """lib.check, attaching the failed goal's provision response to an OptimizationFailureException."""
        try:
            self.lib.check(status)
        except OptimizationFailureException as e:
            e.provision = self.last_failure_provision(_goal_of_message(str(e)))
            raise

    def last_failure_provision(self, recommender: str = "") -> ProvisionResponse:
        out = ProvisionRespStruct()
        self.lib.check(self.lib.lib.ccmi_last_failure_provision(self.handle, C.byref(out)))
        return ProvisionResponse.from_struct(out, recommender)

    def action_acceptance(self, optimized_goal_index: int, action_type: int, partition: int, source: int,
                          destination: int, destination_partition: int = -1, source_disk: int = -1,
                          destination_disk: int = -1) -> str:
        a = ActionStruct(action_type, partition, source, destination, destination_partition, source_disk,
                         destination_disk)
        out = C.c_int32()
        self.lib.check(self.lib.lib.ccmi_action_acceptance(self.handle, optimized_goal_index, C.byref(a),
                                                           C.byref(out)))
        return ACCEPTANCE[out.value]

    def action_acceptance_by_goal(self, goal_name: str, action_type: int, partition: int, source: int,
                                  destination: int, destination_partition: int = -1, source_disk: int = -1,
                                  destination_disk: int = -1) -> str:
        """Goal.actionAcceptance of the optimized goal with this name (ccmi_action_acceptance_by_kind)."""
        a = ActionStruct(action_type, partition, source, destination, destination_partition, source_disk,
                         destination_disk)
        out = C.c_int32()
        self.lib.check(self.lib.lib.ccmi_action_acceptance_by_kind(self.handle, goal_kind(goal_name), C.byref(a),
                                                                   C.byref(out)))
        return ACCEPTANCE[out.value]

    # ---- what the batched device calls share
    def _not_exported(self, symbol: str, why: str) -> None:
        raise UnsupportedOperationException(f"{self.lib.path} does not export {symbol}: {why}")

    @staticmethod
    def _int32_rows(np, rows, width: int, complaint: str):
        """`rows` (tuples or an array) as a contiguous [k, width] int32 array: the rows are the C structs. `np` is the
        caller's numpy (this module imports it only where it is used)."""
        a = np.ascontiguousarray(rows if len(rows) else np.zeros((0, width)), dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != width:
            raise IllegalArgumentException(complaint)
        return a

    def _goals_call(self, fn, names, *args) -> None:
        """lib.check of fn(session, kinds of the goals `names`, their count, *args, first_invalid); what it raises
        carries the index the call reported as `first_invalid`."""
        kinds = (C.c_int32 * max(1, len(names)))(*map(goal_kind, names))
        bad = C.c_int64(-1)
        try:
            self.lib.check(fn(self.handle, kinds, len(names), *args, C.byref(bad)))
        except CruiseControlError as e:
            e.first_invalid = bad.value
            raise

    def actions_acceptance(self, goal_names, actions):
        """Goal.actionAcceptance of several optimized goals for a batch of actions in one device call
        (ccmi_actions_acceptance): a numpy int8 array [n, G] of ACCEPTANCE indices, cell [i, g] what
        action_acceptance_by_goal(goal_names[g], *actions[i]) returns. Actions are tuples in the action-log layout
        (type, partition, source, destination, destination partition, source disk, destination disk) or an [n, 7] int32
        array. An action the single call refuses raises IllegalArgumentException with its index in `first_invalid`."""
        import numpy as np

        if not self.lib.has_actions_acceptance:
            self._not_exported("ccmi_actions_acceptance", "the batched call runs on the device only")
        names = list(goal_names)
        acts = self._int32_rows(np, actions, 7, "actions must be [n, 7]: the action-log layout")  # ActionStruct
        n = acts.shape[0]
        out = np.zeros((n, len(names)), dtype=np.int8)
        self._goals_call(self.lib.lib.ccmi_actions_acceptance, names, C.cast(acts.ctypes.data, C.POINTER(ActionStruct)), n,
                         out.ctypes.data_as(C.POINTER(C.c_int8)))
        return out

    def moves_acceptance_mask(self, goal_names, sources, packed=False):
        """The destination brokers of a batch of move / leadership sources in one device call
        (ccmi_moves_acceptance_mask): a numpy bool array [n, B], cell [i, b] true iff b is not the source broker, the
        action (type, partition, source, b) is legit (GoalUtils.legitMove) and every goal of `goal_names` ACCEPTs it; with
        packed=True the raw uint64 words [n, W], W = (B + 63) // 64, bit b & 63 of word b >> 6. Sources are (type,
        partition, source broker) tuples or an [n, 3] int32 array. A source the call refuses raises
        IllegalArgumentException with its index in `first_invalid`."""
        import numpy as np

        if not self.lib.has_moves_acceptance_mask:
            self._not_exported("ccmi_moves_acceptance_mask", "the masks are computed on the device only")
        names = list(goal_names)
        src = self._int32_rows(np, sources, 3, "sources must be [n, 3]: type, partition, source broker")
        n, B = src.shape[0], self.desc.num_brokers
        rows = np.zeros((n, 4), dtype=np.int32)  # ccmi_move_source is four int32: three and a reserved one
        rows[:, :3] = src
        W = (B + 63) // 64
        words = np.zeros((n, W), dtype=np.uint64)
        self._goals_call(self.lib.lib.ccmi_moves_acceptance_mask, names, rows.ctypes.data, n,
                         words.ctypes.data_as(C.POINTER(C.c_uint64)))
        if packed:
            return words
        bits = np.unpackbits(words.view(np.uint8).reshape(n, W * 8), axis=1, bitorder="little")
        return bits[:, :B].astype(bool)

    def swaps_acceptance_grid(self, goal_names, sources, candidates):
        """The swap candidates of a batch of source replicas in one device call (ccmi_swaps_acceptance_grid): a numpy
        int8 array [n, m], cell [i, j] the SWAP_CODES index of swapping source replica i with candidate replica j —
        SOURCE_NOT_LEGIT / CANDIDATE_NOT_LEGIT when GoalUtils.legitMove fails for the source to the candidate's broker /
        for the candidate to the source's broker, else the first verdict of `goal_names`, in that order, that is not
        ACCEPT, else ACCEPT. Sources and candidates are (partition, broker) tuples or [k, 2] int32 arrays. A replica the
        call refuses raises IllegalArgumentException with `first_invalid` = i for a source, n + j for a candidate."""
        import numpy as np

        if not self.lib.has_swaps_acceptance_grid:
            self._not_exported("ccmi_swaps_acceptance_grid", "the grid is computed on the device only")
        names = list(goal_names)
        # ccmi_swap_replica is two int32
        src = self._int32_rows(np, sources, 2, "sources must be [k, 2]: partition, broker")
        cand = self._int32_rows(np, candidates, 2, "candidates must be [k, 2]: partition, broker")
        n, m = src.shape[0], cand.shape[0]
        codes = np.zeros((n, m), dtype=np.int8)
        self._goals_call(self.lib.lib.ccmi_swaps_acceptance_grid, names, src.ctypes.data, n, cand.ctypes.data, m,
                         codes.ctypes.data_as(C.POINTER(C.c_int8)))
        return codes

    def stats_names(self):
        """(rack names by rack index, host names by host index) from the builder the model was ingested through
        (FlatCluster / LoadMonitorModel.stats_names); an index without a name is written in decimal."""
        if hasattr(self._keep, "stats_names"):
            return self._keep.stats_names()
        return {}, {}

    def broker_stats(self) -> "BrokerStats":
        """ClusterModel.brokerStats (ClusterModel.java:1303-1309) of the session's current model in one device call
        (ccmi_broker_stats): on a fresh session the stats before optimization, after optimizations() or apply() the
        current ones. The session is not changed."""
        import numpy as np

        if not self.lib.has_broker_stats:
            self._not_exported("ccmi_broker_stats", "the stats are computed on the device only")
        B, D = self.desc.num_brokers, self.desc.num_disks
        brokers = np.zeros(B, dtype=np.dtype(BasicStatsStruct))
        hosts = np.zeros(B, dtype=np.dtype(BasicStatsStruct))
        disks = np.zeros(D, dtype=np.dtype(DiskStatsStruct))
        nh = C.c_int32(0)
        self._checked(self.lib.lib.ccmi_broker_stats(self.handle, brokers.ctypes.data, hosts.ctypes.data, C.byref(nh),
                                                     disks.ctypes.data if D else None))
        racks, host_names = self.stats_names()
        logdirs = [self.desc.disk_logdir[d].decode() for d in range(D)]
        return BrokerStats(brokers, hosts[:nh.value].copy(), disks, self.broker_ids(), racks, host_names, logdirs)

    def partition_load(self, resource: str = "DISK", max_load: bool = False, avg_load: bool = False,
                       entries: int = 2**31 - 1, topic: Optional[str] = None,
                       partition_range: Optional[Sequence[int]] = None, broker_ids: Iterable[int] = (),
                       tie_rank=None) -> "PartitionLoadState":
        """The partition load response (PartitionLoadRunnable.getResult) of the session's current model in one device
        call (ccmi_partition_load): the partitions ordered by the utilization of `resource` on their current leader,
        descending. `topic` is a regex that must match the whole topic name (Pattern.matcher().matches()),
        `partition_range` = (lower, upper) partition numbers, both inclusive, `broker_ids` the Kafka ids of which a
        kept partition has at least one among its current brokers (empty: every partition). `tie_rank[p]` orders
        partitions with exactly equal keys (the reference's HashMap iteration order, which the caller holds); None is
        the partition index. The session is not changed."""
        import re

        import numpy as np

        if not self.lib.has_partition_load:
            raise UnsupportedOperationException(
                f"{self.lib.path} does not export ccmi_partition_load: the response is computed on the device only")
        d = self.desc
        P, T, B = d.num_partitions, d.num_topics, d.num_brokers
        q = PartitionLoadQueryStruct()
        q.resource = resource if isinstance(resource, int) else RESOURCES.index(resource)
        q.want_max_load, q.want_avg_load = int(bool(max_load)), int(bool(avg_load))
        q.entries = int(entries)
        lower, upper = partition_range if partition_range is not None else (-2**31, 2**31 - 1)
        q.partition_lower, q.partition_upper = int(lower), int(upper)
        keep = []
        if topic is not None:
            pat = re.compile(topic)
            sel = np.array([1 if pat.fullmatch(n) else 0 for n in self.topic_names()], dtype=np.uint8)
            keep.append(sel)
            q.topic_selected = sel.ctypes.data_as(C.POINTER(C.c_uint8))
        wanted = set(int(b) for b in broker_ids)
        ids = self.broker_ids()
        if wanted:
            sel = np.array([1 if ids[b] in wanted else 0 for b in range(B)], dtype=np.uint8)
            keep.append(sel)
            q.broker_selected = sel.ctypes.data_as(C.POINTER(C.c_uint8))
        if tie_rank is not None:
            rank = np.ascontiguousarray(tie_rank, dtype=np.int32)
            if rank.shape != (P,):
                raise IllegalArgumentException(f"tie_rank needs one entry per partition ({P})")
            keep.append(rank)
            q.tie_rank = rank.ctypes.data_as(C.POINTER(C.c_int32))
        records = np.zeros(max(0, min(q.entries, P)), dtype=np.dtype(PartitionLoadRecordStruct))
        nrec, nsel = C.c_int64(0), C.c_int64(0)
        self._checked(self.lib.lib.ccmi_partition_load(self.handle, C.byref(q), records.ctypes.data if len(records) else None,
                                                       C.byref(nrec), C.byref(nsel)))
        return PartitionLoadState(records[:nrec.value], nsel.value, self.topic_names(),
                                  np.ctypeslib.as_array(d.partition_topic, shape=(P,)).copy() if P else [],
                                  np.ctypeslib.as_array(d.partition_number, shape=(P,)).copy() if P else [], ids)

    def proposal_diff(self, capacity: Optional[int] = None, summary_only: bool = False) -> "ProposalDiff":
        """The ExecutionProposals of the session's current model against its initial placement and their movement
        statistics, diffed on the device (ccmi_proposal_diff). `capacity` cuts the records (the summary always covers
        every proposal); None asks for the count first and then for all of them; `summary_only` returns no records.
        The session is not changed, and the list ClusterModel.proposals() reads is left alone."""
        import numpy as np

        if not self.lib.has_proposal_diff:
            self._not_exported("ccmi_proposal_diff", "the diff is computed on the device only")
        if capacity is not None and capacity < 0:
            raise IllegalArgumentException("capacity < 0")
        fn = self.lib.lib.ccmi_proposal_diff
        summary, n = ProposalSummaryStruct(), C.c_int64(0)
        sized = capacity is None and not summary_only
        if sized:  # the sizing call
            self._checked(fn(self.handle, None, 0, C.byref(n), C.byref(summary)))
        cap = 0 if summary_only else int(summary.num_proposals if sized else capacity)
        records = np.zeros(min(cap, self.desc.num_partitions), dtype=np.dtype(ProposalRecordStruct))
        if len(records) or not sized:
            self._checked(fn(self.handle, records.ctypes.data if len(records) else None, len(records), C.byref(n),
                             C.byref(summary)))
        return ProposalDiff(records[:n.value], summary)

    def sorted_replicas(self, brokers=None, *, leaders=False, followers=False, online=False, offline=False,
                        immigrants=False, immigrant_or_offline=False, priorities=(), score=None, reverse=False,
                        above=None, below=None, excluded_topics=None, included_topics=None, with_scores=False):
        """Per asked broker the list a freshly initialised SortedReplicas would iterate on the session's current model,
        selected and sorted on the device (ccmi_sorted_replicas): one numpy int32 array [k, 2] of (partition, broker)
        rows per broker of `brokers` (broker indices; None = every broker), usable as they stand as the sources or
        candidates of swaps_acceptance_grid. The keyword flags are ReplicaSortFunctionFactory's selection functions,
        `priorities` a sequence of "offline" / "immigrants" (or CCMI_PRIO_* numbers) in application order, `score` a
        resource (name or index) scored by its metric group's average, `reverse` the reversed score, `above` / `below`
        (resource, limit) pairs, `excluded_topics` / `included_topics` topic names (or a [T] uint8 mask). With
        `with_scores` the result is (lists, scores): the float64 scores exactly as compared, broker by broker. The
        buffer is sized by a first call with no room. A broker the call refuses raises IllegalArgumentException with
        its position in `first_invalid`. The session is not changed."""
        import numpy as np

        if not self.lib.has_sorted_replicas:
            raise UnsupportedOperationException(
                f"{self.lib.path} does not export ccmi_sorted_replicas: the lists are built on the device only")
        B, T = self.desc.num_brokers, self.desc.num_topics

        def res(r):
            return r if isinstance(r, int) else RESOURCES.index(r)

        q = SortedReplicasQueryStruct()
        q.select_mask = ((SEL_LEADERS if leaders else 0) | (SEL_FOLLOWERS if followers else 0) |
                         (SEL_ONLINE if online else 0) | (SEL_OFFLINE if offline else 0) |
                         (SEL_IMMIGRANTS if immigrants else 0) |
                         (SEL_IMMIGRANT_OR_OFFLINE if immigrant_or_offline else 0))
        prio = [p if isinstance(p, int) else SORT_PRIORITIES.index(p) for p in priorities]
        if len(prio) > 2:
            raise IllegalArgumentException("at most two priority functions")
        q.num_priorities = len(prio)
        q.priorities[0], q.priorities[1] = (prio + [-1, -1])[:2]
        q.score_resource = -1 if score is None else res(score)
        q.score_reverse = int(bool(reverse))
        q.above_resource, q.above_limit = (-1, 0.0) if above is None else (res(above[0]), float(above[1]))
        q.below_resource, q.below_limit = (-1, 0.0) if below is None else (res(below[0]), float(below[1]))
        keep = []

        def mask(topics):
            if isinstance(topics, np.ndarray):
                m = np.ascontiguousarray(topics, dtype=np.uint8)
                if m.shape != (T,):
                    raise IllegalArgumentException(f"a topic mask needs one entry per topic ({T})")
            else:
                wanted = set(topics)
                m = np.array([1 if n in wanted else 0 for n in self.topic_names()], dtype=np.uint8)
            if not len(m):
                m = np.zeros(1, dtype=np.uint8)
            keep.append(m)
            return m.ctypes.data_as(C.POINTER(C.c_uint8))

        if excluded_topics is not None:
            q.topic_excluded = mask(excluded_topics)
        if included_topics is not None:
            q.topic_included = mask(included_topics)
        if brokers is None:
            ask, n = None, B
        else:
            ask = np.ascontiguousarray(list(brokers), dtype=np.int32).reshape(-1)
            n = len(ask)
        fn = self.lib.lib.ccmi_sorted_replicas
        offsets = np.zeros(n + 1, dtype=np.int64)
        total, bad = C.c_int64(0), C.c_int64(-1)

        def call(records, scores, capacity):
            try:
                self._checked(fn(self.handle, C.byref(q), ask.ctypes.data if ask is not None else None, n,
                                 offsets.ctypes.data, records.ctypes.data if capacity else None,
                                 scores.ctypes.data if scores is not None and capacity else None, capacity,
                                 C.byref(total), C.byref(bad)))
            except CruiseControlError as e:
                e.first_invalid = bad.value
                raise

        if brokers is not None and n == 0:
            ask = np.zeros(1, dtype=np.int32)  # n == 0 with a list: not the NULL "every broker" form
        call(None, None, 0)  # the sizing call
        records = np.zeros((total.value, 2), dtype=np.int32)  # ccmi_swap_replica is two int32
        scores = np.zeros(total.value, dtype=np.float64) if with_scores else None
        if total.value:
            call(records, scores, total.value)
        lists = [records[offsets[i]:offsets[i + 1]] for i in range(n)]
        if with_scores:
            return lists, [scores[offsets[i]:offsets[i + 1]] for i in range(n)]
        return lists

    def execution_plan(self, strategies=(), proposal_rank=None, partition_state=None) -> "ExecutionPlan":
        """What ExecutionTaskPlanner.addExecutionProposals builds from the proposals proposal_diff() would return now,
        computed on the device (ccmi_execution_plan), under the assumption that the live cluster still has the
        session's initial placement with every replica in sync. `strategies` is the ReplicaMovementStrategy chain in
        application order, at most four of MOVEMENT_STRATEGIES (class names or CCMI_STRATEGY_* numbers; Base is
        appended when absent); `proposal_rank` ([P] int32) the position of each partition's proposal in the caller's
        collection (None: partition order); `partition_state` ([P] uint8) the PSTATE_* bits the ISR strategies read
        (None: no bit set). The buffers are sized by a first call with no room. The session is not changed."""
        import numpy as np

        if not self.lib.has_execution_plan:
            self._not_exported("ccmi_execution_plan", "the plan is built on the device only")
        B, P = self.desc.num_brokers, self.desc.num_partitions
        chain = [s if isinstance(s, int) else MOVEMENT_STRATEGIES.index(s) for s in strategies]
        if len(chain) > 4:
            raise IllegalArgumentException("at most four strategies")
        q = ExecutionPlanQueryStruct()
        q.num_strategies = len(chain)
        for i in range(4):
            q.strategies[i] = chain[i] if i < len(chain) else -1

        def per_partition(a, dtype, what):
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if len(a) != P:
                raise IllegalArgumentException(f"{what} needs one entry per partition ({P})")
            return a if P else np.zeros(1, dtype=dtype)

        rank = state = None
        if proposal_rank is not None:
            rank = per_partition(proposal_rank, np.int32, "proposal_rank")
            q.proposal_rank = rank.ctypes.data_as(C.POINTER(C.c_int32))
        if partition_state is not None:
            state = per_partition(partition_state, np.uint8, "partition_state")
            q.partition_state = state.ctypes.data_as(C.POINTER(C.c_uint8))
        fn = self.lib.lib.ccmi_execution_plan
        summary = PlanSummaryStruct()
        inter_off, intra_off = np.zeros(B + 1, dtype=np.int64), np.zeros(B + 1, dtype=np.int64)
        order = np.full(max(B, 1), -1, dtype=np.int32)
        self._checked(fn(self.handle, C.byref(q), C.byref(summary), None, 0, inter_off.ctypes.data, None, 0, None,
                         intra_off.ctypes.data, None, 0, None, 0))  # the sizing call
        dropped = summary.num_intra_tasks > 0
        none = bool(summary.mingled)
        tasks = np.zeros(0 if dropped else summary.num_inter_tasks, dtype=np.dtype(PlanTaskStruct))
        inter = np.zeros(int(inter_off[B]), dtype=np.int32)
        intra = np.zeros(int(intra_off[B]), dtype=np.int32)
        leaders = np.zeros(0 if none else summary.num_leader_tasks, dtype=np.int32)

        def ptr(a):
            return a.ctypes.data if len(a) else None

        if len(tasks) or len(inter) or len(intra) or len(leaders):
            self._checked(fn(self.handle, C.byref(q), C.byref(summary), ptr(tasks), len(tasks), inter_off.ctypes.data,
                             ptr(inter), len(inter), order.ctypes.data if len(inter) else None, intra_off.ctypes.data,
                             ptr(intra), len(intra), ptr(leaders), len(leaders)))
        return ExecutionPlan(summary, tasks, [inter[inter_off[b]:inter_off[b + 1]] for b in range(B)],
                             order[:summary.num_brokers_with_tasks].copy(),
                             [intra[intra_off[b]:intra_off[b + 1]] for b in range(B)], leaders, chain, state)

    def apply(self, actions) -> int:
        """Apply actions decided elsewhere (tuples in the action-log layout: type, partition, source,
        destination, destination partition, source disk, destination disk) to the resident model
        (ccmi_session_apply). Returns the number applied; raises on the first invalid one."""
        acts = list(actions)
        arr = (ActionStruct * max(1, len(acts)))(*[ActionStruct(*a) for a in acts])
        done = C.c_int64()
        self.lib.check(self.lib.lib.ccmi_session_apply(self.handle, arr, len(acts), C.byref(done)))
        return done.value

    # ---- queue-scan diagnostics (ccmi_queue_probe, csrc/ccmi_session.h): not part of the ABI
    @staticmethod
    def _queue_probe_args(spec, self_goal="ReplicaDistributionGoal", accept_goals=(), head=-1, skip_key=None, tail=(),
                          cands=(), mode=0):
        """(QueueProbeArgsStruct, the arrays it points into). `spec`: a dict of the struct's Spec fields (leaders,
        score_res, reverse, prio_offline, prio_immigrants, excl_topics); skip_key None: no continuation."""
        a = QueueProbeArgsStruct()
        a.sel_leaders = int(bool(spec.get("leaders", False)))
        a.score_res = int(spec.get("score_res", -1))
        a.score_reverse = int(bool(spec.get("reverse", False)))
        a.prio_offline = int(bool(spec.get("prio_offline", False)))
        a.prio_immigrants = int(bool(spec.get("prio_immigrants", False)))
        a.sel_excl_topics = int(bool(spec.get("excl_topics", False)))
        kinds = [goal_kind(g) for g in accept_goals]
        keep = [(C.c_int32 * max(1, len(kinds)))(*kinds), (C.c_int32 * max(1, len(tail)))(*tail),
                (C.c_int32 * max(1, len(cands)))(*cands)]
        a.self_kind, a.num_accept, a.accept_kinds = goal_kind(self_goal), len(kinds), keep[0]
        a.head, a.has_skip, a.skip_key = int(head), int(skip_key is not None), int(skip_key or 0)
        a.tail, a.n_tail, a.cands, a.n_cands, a.mode = keep[1], len(tail), keep[2], len(cands), int(mode)
        return a, keep

    def _queue_probe(self, spec, self_goal="ReplicaDistributionGoal", accept_goals=(), head=-1, skip_key=None, tail=(),
                     cands=(), mode=0) -> Dict[str, int]:
        """One queue scan over the entries [head] ++ tail x cands with `self_goal` as the goal being optimized and
        `accept_goals` as the optimized goals, next to a host loop's answer: the report's fields by name, with `dev` and
        `ref` the (entry, replica, column) winners or None. mode 1 leaves out the table audit, mode 2 runs the host loop only."""
        if not self.lib.has_queue_probe:
            self._not_exported("ccmi_queue_probe", "a diagnostics build has it")
        a, keep = self._queue_probe_args(spec, self_goal, accept_goals, head, skip_key, tail, cands, mode)
        out = QueueProbeReportStruct()
        self.lib.check(self.lib.lib.ccmi_queue_probe(self.handle, C.byref(a), C.byref(out)))
        rep = {f: getattr(out, f) for f, _ in QueueProbeReportStruct._fields_}
        rep["dev"] = None if out.dev_entry < 0 else (out.dev_entry, out.dev_replica, out.dev_column)
        rep["ref"] = None if out.ref_entry < 0 else (out.ref_entry, out.ref_replica, out.ref_column)
        return rep

    def _queue_probe_view(self, spec, broker: int, slots: bool = False) -> List[tuple]:
        """Broker `broker`'s rows under `spec` as the model has them: (key, replica) in key order; with `slots` also
        each replica's slot in the keyed mirror's block as the last queue sync left it (-1: none)."""
        if not self.lib.has_queue_probe:
            self._not_exported("ccmi_queue_probe_view", "a diagnostics build has it")
        a, keep = self._queue_probe_args(spec)
        n = C.c_int32()
        self.lib.check(self.lib.lib.ccmi_queue_probe_view(self.handle, C.byref(a), broker, None, None, None, 0,
                                                          C.byref(n)))
        k = max(1, n.value)
        keys, reps, slot = (C.c_uint64 * k)(), (C.c_int32 * k)(), (C.c_int32 * k)()
        self.lib.check(self.lib.lib.ccmi_queue_probe_view(self.handle, C.byref(a), broker, keys, reps, slot, n.value,
                                                          C.byref(n)))
        return [(keys[i], reps[i]) + ((slot[i],) if slots else ()) for i in range(n.value)]

    def _disks_of(self, broker_logdirs) -> List[int]:
        """Desc disk indices of {broker id: logdirs}; an unknown broker id or logdir is the reference's "Invalid log
        dirs provided for broker %d." (RemoveDisksRunnable.java:139-142)."""
        ids = self.broker_ids()
        index = {(ids[self.desc.disk_broker[d]], self.desc.disk_logdir[d].decode()): d
                 for d in range(self.desc.num_disks)}
        disks = []
        for broker_id, logdirs in broker_logdirs.items():
            for logdir in ([logdirs] if isinstance(logdirs, str) else logdirs):
                if (broker_id, logdir) not in index:
                    raise IllegalArgumentException(f"Invalid log dirs provided for broker {broker_id}.")
                disks.append(index[(broker_id, logdir)])
        return disks

    def mark_disks_for_removal(self, broker_logdirs, capacity_threshold: float) -> None:
        """RemoveDisksRunnable.checkCanRemoveDisks (:131-161) with capacityThreshold(DISK) = capacity_threshold, then
        Disk.markDiskForRemoval on every named logdir (ccmi_session_mark_disks_for_removal; all or nothing).
        broker_logdirs: {broker id: logdirs}. IllegalArgumentException with the reference's message when a check
        fails, IllegalStateException on a session that has optimized a goal or applied actions."""
        if not self.lib.has_remove_disks:
            self._not_exported("ccmi_session_mark_disks_for_removal", "remove-disks needs a newer library")
        disks = self._disks_of(broker_logdirs)
        arr = (C.c_int32 * max(1, len(disks)))(*disks)
        bad = C.c_int32(-1)
        self.lib.check(self.lib.lib.ccmi_session_mark_disks_for_removal(self.handle, arr, len(disks),
                                                                        float(capacity_threshold), C.byref(bad)))

    def remove_disks(self, broker_logdirs, constraint: Optional[BalancingConstraint] = None,
                     options: Optional[OptimizationOptions] = None) -> "OptimizerResult":
        """RemoveDisksRunnable.workWithClusterModel (:77-129): checkCanRemoveDisks, markDiskForRemoval, then one
        optimization with the single goal new IntraBrokerDiskCapacityGoal(true)."""
        bc = constraint or BalancingConstraint()
        self.mark_disks_for_removal(broker_logdirs, bc.capacity_threshold[DISK])
        return GoalOptimizer(bc).optimizations(self, goals_from_names([REMOVE_DISKS_GOAL], bc), options)

    def cluster_stats(self, constraint: Optional[BalancingConstraint] = None,
                      options: Optional[OptimizationOptions] = None) -> Dict[str, object]:
        s = StatsStruct()
        o, keep = (options or OptimizationOptions()).to_struct()
        c = (constraint or BalancingConstraint()).to_struct(self.topic_names(), self.broker_ids())
        self.lib.check(self.lib.lib.ccmi_compute_cluster_stats(self.handle, C.byref(c), C.byref(o), C.byref(s)))
        return stats_to_dict(s)

    def actions(self) -> List[tuple]:
        n = self.lib.lib.ccmi_action_log_count(self.handle)
        buf = (ActionStruct * max(1, n))()
        if n:
            self.lib.check(self.lib.lib.ccmi_action_log_copy(self.handle, 0, n, buf))
        return [(a.type, a.partition, a.source_broker, a.destination_broker, a.destination_partition,
                 a.source_disk, a.destination_disk) for a in buf[:n]]

    def replica_distribution(self) -> List[int]:
        out = (C.c_int32 * self.num_replicas)()
        self.lib.check(self.lib.lib.ccmi_replica_distribution(self.handle, out))
        return list(out)

    def replica_disks(self) -> List[int]:
        """Disk index of every replica slot in partition order (the logdir of getReplicaDistribution)."""
        out = (C.c_int32 * self.num_replicas)()
        self.lib.check(self.lib.lib.ccmi_replica_disks(self.handle, out))
        return list(out)

    def leader_distribution(self) -> List[int]:
        out = (C.c_int32 * self.num_partitions)()
        self.lib.check(self.lib.lib.ccmi_leader_distribution(self.handle, out))
        return list(out)

    def proposals(self, max_rf: int = 8) -> List[ExecutionProposal]:
        n = self.lib.lib.ccmi_proposal_count(self.handle)
        if n == 0:
            return []
        part = (C.c_int32 * n)()
        size = (C.c_int32 * n)()
        old_leader = (C.c_int32 * n)()
        old_r = (C.c_int32 * (n * max_rf))()
        new_r = (C.c_int32 * (n * max_rf))()
        self.lib.check(self.lib.lib.ccmi_proposals(self.handle, max_rf, part, size, old_leader, old_r, new_r))
        old_d = (C.c_int32 * (n * max_rf))()
        new_d = (C.c_int32 * (n * max_rf))()
        self.lib.check(self.lib.lib.ccmi_proposal_disks(self.handle, max_rf, old_d, new_d))
        out = []
        for i in range(n):
            rf = sum(1 for x in old_r[i * max_rf:(i + 1) * max_rf] if x >= 0)
            sl = slice(i * max_rf, i * max_rf + rf)
            out.append(ExecutionProposal(part[i], size[i], old_leader[i], list(old_r[sl]), list(new_r[sl]),
                                         list(old_d[sl]), list(new_d[sl])))
        return out

    def perf(self) -> PerfStruct:
        p = PerfStruct()
        self.lib.check(self.lib.lib.ccmi_perf(self.handle, C.byref(p)))
        # the host-prefix counters ride along as plain attributes (ccmi_host_prefix_perf; 0 from a library without it)
        h = HostPrefixPerfStruct()
        if self.lib.has_host_prefix_perf:
            self.lib.check(self.lib.lib.ccmi_host_prefix_perf(self.handle, C.byref(h)))
        p.host_scans, p.host_candidates = h.host_scans, h.host_candidates
        x = HostCrossPerfStruct()
        if self.lib.has_host_cross_perf:
            self.lib.check(self.lib.lib.ccmi_host_cross_perf(self.handle, C.byref(x)))
        p.host_cross_scans, p.host_cross_candidates = x.host_cross_scans, x.host_cross_candidates
        return p

    def reset_perf(self) -> None:
        self.lib.lib.ccmi_perf_reset(self.handle)

    def set_kernel_timing(self, enabled: bool) -> None:
        self.lib.lib.ccmi_set_kernel_timing(self.handle, int(enabled))

    def set_shard(self, rank: int, count: int, combine_min) -> None:
        """Destination-sharded mode with a caller-supplied combiner: combine_min(local_key:int) -> global min key
        (None / -1 for no candidate on this shard). Used with torch.distributed gloo in the CPU tests."""
        none = (1 << 63) - 1

        def _fn(_ctx, key_ptr):
            try:
                k = key_ptr[0]
                key_ptr[0] = int(combine_min(k if k != none else none))
                return 0
            except Exception:  # noqa: BLE001 - reported as a failed combine by the engine
                return 1

        self._combine_cb = AllreduceMinFn(_fn)  # keep the trampoline alive with the session
        self.lib.check(self.lib.lib.ccmi_session_set_shard(self.handle, rank, count, self._combine_cb, None))

    def attach_rccl(self, rank: int, count: int, unique_id: bytes) -> None:
        """Destination-sharded mode over the built-in RCCL combiner (one int64 MIN allreduce per scan)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self.lib.check(self.lib.lib.ccmi_session_attach_rccl(self.handle, rank, count, buf))

    def attach_shm(self, rank: int, count: int, name: str, job_nonce: int = 0, timeout_s: float = 0.0) -> None:
        """Destination-sharded mode over the built-in host shared-memory combiner (ranks on one node): one int64 MIN
        per scan in a POSIX shared-memory block; the scan server stays on. `job_nonce` (the same nonzero value on
        every rank, ccmi_session_attach_shm_job, ABI v12): the other ranks refuse a block rank 0 of this job did not
        stamp with it, however recent; `timeout_s` bounds the waits (0 = 120 s)."""
        if job_nonce or timeout_s:
            self.lib.check(self.lib.lib.ccmi_session_attach_shm_job(self.handle, rank, count, name.encode(),
                                                                    job_nonce & (2 ** 64 - 1), float(timeout_s)))
        else:
            self.lib.check(self.lib.lib.ccmi_session_attach_shm(self.handle, rank, count, name.encode()))

    def attach_group(self, group: "ShardGroup", rank: int) -> None:
        """Rank `rank` of a one-process shard group (ShardGroup): the scan server combines the ranks' keys on the
        device; this session's optimizations must run on a thread of its own, concurrently with the other ranks'."""
        self.lib.check(self.lib.lib.ccmi_session_attach_group(self.handle, group.handle, rank))
        self._group = group  # the group outlives the session


class ShardGroup:
    """The ranks of one destination-sharded proposal driven from ONE process (ccmi_shard_group_*, ABI v11): one
    session per rank (typically one per GPU), each optimized on its own host thread; a scan the session's scan server
    ran is MIN-combined with the other ranks' on the device, through pinned host memory every GPU maps. Keep the group
    alive while its sessions are."""

    def __init__(self, count: int, lib: Optional["Library"] = None):
        self.lib = lib or Library.get()
        h = C.c_void_p()
        self.lib.check(self.lib.lib.ccmi_shard_group_create(count, C.byref(h)))
        self.handle = h
        self.count = count

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.lib.ccmi_shard_group_destroy(self.handle)
            self.handle = None


def rccl_unique_id(lib: Optional["Library"] = None) -> bytes:
    """ncclGetUniqueId through libccmi (rank 0 broadcasts it to the other ranks)."""
    lib = lib or Library.get()
    buf = (C.c_uint8 * 128)()
    lib.check(lib.lib.ccmi_rccl_unique_id(buf))
    return bytes(buf)


class GoalOptimizer:
    """GoalOptimizer.optimizations (GoalOptimizer.java:435-524) on a device session. priority_weight /
    strictness_weight: goal.balancedness.priority.weight / goal.balancedness.strictness.weight (AnalyzerConfig.java:
    374-385) for the on-demand balancedness score."""

    def __init__(self, constraint: Optional[BalancingConstraint] = None, priority_weight: float = 1.1,
                 strictness_weight: float = 1.5):
        self.constraint = constraint or BalancingConstraint()
        self.priority_weight = priority_weight
        self.strictness_weight = strictness_weight

    def optimizations(self, cluster: ClusterModel, goals_by_priority: Sequence[Goal],
                      options: Optional[OptimizationOptions] = None, broker_stats: bool = False) -> OptimizerResult:
        """broker_stats=True also takes ClusterModel.brokerStats before the first goal (GoalOptimizer.java:442) into
        OptimizerResult.broker_stats_before_optimization: one more device call. The default issues none."""
        if not goals_by_priority:
            raise IllegalArgumentException("At least one goal must be provided to get an optimization result.")
        stats_before = cluster.broker_stats() if broker_stats else None
        kinds = (C.c_int32 * len(goals_by_priority))(*[g.kind for g in goals_by_priority])
        results = (GoalResultStruct * len(goals_by_priority))()
        o, keep = (options or OptimizationOptions()).to_struct()
        c = self.constraint.to_struct(cluster.topic_names(), cluster.broker_ids())
        import time
        t0 = time.perf_counter()
        cluster._checked(cluster.lib.lib.ccmi_optimizations(cluster.handle, kinds, len(goals_by_priority),
                                                            C.byref(c), C.byref(o), results))
        dt = time.perf_counter() - t0
        grs = [GoalResult(GOAL_NAMES[r.goal_kind], bool(r.succeeded), bool(r.has_diff), r.seconds, r.candidates,
                          r.device_candidates, r.device_launches, r.actions, stats_to_dict(r.stats),
                          ProvisionResponse.from_struct(r.provision, GOAL_NAMES[r.goal_kind])) for r in results]
        res = OptimizerResult(grs, cluster, dt, [g.name for g in grs if not g.succeeded])
        res.broker_stats_before_optimization = stats_before
        res.options = options or OptimizationOptions()
        res.balancedness_cost_by_goal = balancedness_cost_by_goal(goals_by_priority, self.priority_weight,
                                                                  self.strictness_weight)
        return res


MAX_BALANCEDNESS_SCORE = 100.0  # KafkaCruiseControlUtils.MAX_BALANCEDNESS_SCORE
BALANCEDNESS_SCORE_WITH_OFFLINE_REPLICAS = -1.0  # GoalViolationDetector.java:69


@dataclass
class GoalViolations:
    """detector/GoalViolations: the violated detection goals by fixability, the aggregated provision response and
    the balancedness score GoalViolationDetector.run() leaves behind."""
    fixable: List[str]
    unfixable: List[str]
    provision_response: "ProvisionResponse"
    balancedness_score: float
    skipped_due_to_offline_replicas: bool = False
    seconds: float = 0.0


class GoalViolationDetector:
    """GoalViolationDetector.run (detector/GoalViolationDetector.java:176-332) as a what-if batch.

    Each detection goal is optimized on its own, without optimized goals, with OptimizationOptions
    (excluded topics / brokers, isTriggeredByGoalViolation = true; DefaultOptimizationOptionsGenerator.java:17-25):
    an OptimizationFailureException makes it an unfixable violation, a diff a fixable one. The reference reuses the
    model only after a goal that changed nothing, so every goal sees the initial model: the goals are independent and
    run as concurrent device sessions (one host thread and HIP stream each, `max_concurrency` at a time) instead of
    one after the other. A model with dead brokers or broken disks is skipped (skipDueToOfflineReplicas :259-273)."""

    def __init__(self, detection_goals: Sequence[str], constraint: Optional[BalancingConstraint] = None,
                 priority_weight: float = 1.1, strictness_weight: float = 1.5, lib: Optional[Library] = None,
                 device: Optional[int] = None, max_concurrency: int = 8, devices: Optional[Sequence[int]] = None):
        self.goals = list(detection_goals)
        self.constraint = constraint or BalancingConstraint()
        self.cost = balancedness_cost_by_goal(goals_from_names(self.goals), priority_weight, strictness_weight)
        self.lib = lib or Library.get()
        # the sessions go round-robin over `devices` (default: every visible gfx950; `device` pins them to one)
        if devices is None:
            devices = [device] if device is not None else list(range(max(1, self.lib.device_count())))
        self.devices = list(devices)
        self.max_concurrency = max_concurrency

    def detect(self, desc: ClusterDesc, keepalive=None, excluded_topics: Sequence[int] = (),
               excluded_brokers_for_leadership: Sequence[int] = (),
               excluded_brokers_for_replica_move: Sequence[int] = ()) -> GoalViolations:
        import time
        from concurrent.futures import ThreadPoolExecutor
        t0 = time.perf_counter()
        states = [desc.broker_state[b] for b in range(desc.num_brokers)]
        if BROKER_STATES["DEAD"] in states or BROKER_STATES["BAD_DISKS"] in states:
            return GoalViolations([], [], ProvisionResponse("UNDECIDED"), BALANCEDNESS_SCORE_WITH_OFFLINE_REPLICAS, True,
                                  time.perf_counter() - t0)
        opts = OptimizationOptions(excluded_topics=list(excluded_topics),
                                   excluded_brokers_for_leadership=list(excluded_brokers_for_leadership),
                                   excluded_brokers_for_replica_move=list(excluded_brokers_for_replica_move),
                                   is_triggered_by_goal_violation=True)

        def one(i_name):  # GoalViolationDetector.optimizeForGoal (:296-331)
            i, name = i_name
            cm = ClusterModel(desc, device=self.devices[i % len(self.devices)], lib=self.lib, keepalive=keepalive)
            goal = goals_from_names([name], self.constraint)[0]
            try:
                goal.optimize(cm, set(), opts)
            except OptimizationFailureException as e:
                return name, "unfixable", e.provision
            diff = cm.proposals()
            return name, ("fixable" if diff else None), goal.provision

        with ThreadPoolExecutor(max(1, min(self.max_concurrency, len(self.goals)))) as pool:
            outcomes = list(pool.map(one, enumerate(self.goals)))
        fixable = [n for n, v, _ in outcomes if v == "fixable"]
        unfixable = [n for n, v, _ in outcomes if v == "unfixable"]
        prov = ProvisionResponse("UNDECIDED")
        for _, _, p in outcomes:
            if p is not None:
                prov.aggregate(p)
        score = MAX_BALANCEDNESS_SCORE - sum(self.cost[n] for n in fixable + unfixable)  # refreshBalancednessScore
        return GoalViolations(fixable, unfixable, prov, score, False, time.perf_counter() - t0)


def balancedness_cost_by_goal(goals: Sequence[Goal], priority_weight: float = 1.1,
                              strictness_weight: float = 1.5) -> Dict[str, float]:
    """KafkaCruiseControlUtils.balancednessCostByGoal (KafkaCruiseControlUtils.java:844-870)."""
    if not goals:
        raise IllegalArgumentException("At least one goal must be provided to get the balancedness cost.")
    if priority_weight <= 0 or strictness_weight <= 0:
        raise IllegalArgumentException(f"Balancedness weights must be positive (priority:{priority_weight:f}, "
                                       f"strictness:{strictness_weight:f}).")
    cost: Dict[str, float] = {}
    weight_sum = 0.0
    previous = 1 / priority_weight
    for g in reversed(list(goals)):
        current = priority_weight * previous
        c = current * (strictness_weight if g.is_hard_goal() else 1)
        weight_sum += c
        cost[g.name()] = c
        previous = current
    return {k: MAX_BALANCEDNESS_SCORE * v / weight_sum for k, v in cost.items()}


def goals_from_names(names: Sequence[str], constraint: Optional[BalancingConstraint] = None) -> List[Goal]:
    return [globals()[n](constraint=constraint) for n in names]
