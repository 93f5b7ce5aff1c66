/*
 * ccmi.h — C ABI of the MI355X proposal engine (libccmi.so).
 *
 * Drop-in boundary for Cruise Control's goal-optimizer hot path. Every entry point replaces a
 * reference interface (paths relative to cruise-control/src/main/java/com/linkedin/kafka/cruisecontrol/):
 *
 *   ccmi_session_create        <- the ClusterModel a caller hands to GoalOptimizer.optimizations
 *                                 (model/ClusterModel.java:135-139 createRack/createBroker/createReplica/
 *                                 setReplicaLoad, :395-446); the desc is the flattened model.
 *   ccmi_optimizations         <- GoalOptimizer.optimizations(ClusterModel, List<Goal>, OperationProgress,
 *                                 Map, OptimizationOptions)  analyzer/GoalOptimizer.java:435-524
 *   ccmi_goal_optimize         <- Goal.optimize(ClusterModel, Set<Goal>, OptimizationOptions)
 *                                 analyzer/goals/Goal.java:60-66, AbstractGoal.java:81-135
 *   ccmi_action_acceptance     <- Goal.actionAcceptance(BalancingAction, ClusterModel)
 *                                 analyzer/goals/Goal.java:68-80
 *   ccmi_actions_acceptance    <- AnalyzerUtils.isProposalAcceptableForOptimizedGoals for a candidate list
 *                                 analyzer/AnalyzerUtils.java:169-179 (every goal's verdict, one device call)
 *   ccmi_moves_acceptance_mask <- the candidate loop of AbstractGoal.maybeApplyBalancingAction
 *                                 analyzer/goals/AbstractGoal.java:243-270 (legit and accepted brokers as bit masks)
 *   ccmi_swaps_acceptance_grid <- the candidate loop of AbstractGoal.maybeApplySwapAction
 *                                 analyzer/goals/AbstractGoal.java:287-338 (one code per replica pair)
 *   ccmi_broker_stats          <- ClusterModel.brokerStats(KafkaCruiseControlConfig)  model/ClusterModel.java:1303-1309
 *                                 (the load block of a rebalance response and of the load endpoint)
 *   ccmi_partition_load        <- PartitionLoadRunnable.getResult  servlet/handler/async/runnable/PartitionLoadRunnable.java:32-60
 *                                 -> ClusterModel.replicasSortedByUtilization model/ClusterModel.java:1135-1141
 *                                 -> PartitionLoadState servlet/response/PartitionLoadState.java:56-151
 *   ccmi_compute_cluster_stats <- ClusterModel.getClusterStats(BalancingConstraint, OptimizationOptions)
 *                                 model/ClusterModel.java:137-139 -> ClusterModelStats.populate :84-102
 *   ccmi_action_log_*          <- the ordered relocateReplica/relocateLeadership calls a goal makes
 *                                 (model/ClusterModel.java:380-441); a Java shim replays them so the
 *                                 caller's ClusterModel ends in the identical state.
 *   ccmi_replica_distribution / ccmi_leader_distribution
 *                              <- ClusterModel.getReplicaDistribution / getLeaderDistribution :167-198
 *   ccmi_proposals             <- AnalyzerUtils.getDiff -> Set<ExecutionProposal>  analyzer/AnalyzerUtils.java:55-93
 *   ccmi_proposal_diff         <- AnalyzerUtils.getDiff / OptimizerResult.getMovementStats
 *   ccmi_sorted_replicas       <- SortedReplicas.sortedReplicas  model/SortedReplicas.java:75-114
 *                                 analyzer/AnalyzerUtils.java:63-93, analyzer/OptimizerResult.java:258-278 (the proposals
 *                                 and the five movement numbers of the current model, diffed on the device)
 *   ccmi_execution_plan        <- ExecutionTaskPlanner.addExecutionProposals  executor/ExecutionTaskPlanner.java:137-273,
 *                                 brokerComparator :518-539, strategy/AbstractReplicaMovementStrategy.java:28-85 (the
 *                                 tasks, their ids, the per-broker task sets in strategy order, the broker order)
 *   ccmi_aggregator_*          <- MetricSampleAggregator.addSample / completeness / aggregate / peekCurrentWindow
 *                                 cruise-control-core monitor/sampling/aggregator/MetricSampleAggregator.java:141-293,
 *                                 RawMetricValues.java, WindowState.java (the step before ccmi_builder_populate_partition)
 *   ccmi_builder_populate_from_aggregator
 *                              <- MonitorUtils.populatePartitionLoad for every partition of an aggregate
 *                                 monitor/LoadMonitor.java:491-543, monitor/MonitorUtils.java:415-479 (one device call
 *                                 from the aggregator's rows to the model builder)
 *   ccmi_aggregator_metric_anomalies
 *                              <- PercentileMetricAnomalyFinder.metricAnomalies  cruise-control-core
 *                                 detector/metricanomaly/PercentileMetricAnomalyFinder.java:64-93, :140-177
 *   ccmi_slow_broker_finder_*  <- SlowBrokerFinder.metricAnomalies  detector/SlowBrokerFinder.java:163-422 (the two
 *                                 finders MetricAnomalyDetector.run hands the broker aggregator's history and current
 *                                 window to, detector/MetricAnomalyDetector.java:69-75; the rows stay on the device)
 *   ccmi_random_cluster        <- test fixture RandomCluster.generate+populate
 *                                 (src/test/java/.../model/RandomCluster.java:53-455)
 *
 * Plain C: pointers + sizes only. All arrays are caller-owned for inputs and copied in.
 * Errors: every call returns ccmi_status; the last error text is available from ccmi_last_error().
 * Threading: a session is single-threaded; the library is thread-safe across sessions.
 */
#ifndef CCMI_H_
#define CCMI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCMI_ABI_VERSION 13

typedef enum ccmi_status {
  CCMI_OK = 0,
  CCMI_E_INVALID = 1,     /* IllegalArgumentException */
  CCMI_E_DEVICE = 2,      /* HIP runtime / device failure, or no gfx950 device */
  CCMI_E_OPT_FAILURE = 3, /* OptimizationFailureException */
  CCMI_E_STATE = 4,       /* IllegalStateException (e.g. stats regression check, AbstractGoal.java:114-117) */
  CCMI_E_UNSUPPORTED = 5  /* goal kind / option outside the implemented scope */
} ccmi_status;

/* common/Resource.java:17-25 ids */
typedef enum ccmi_resource { CCMI_CPU = 0, CCMI_NW_IN = 1, CCMI_NW_OUT = 2, CCMI_DISK = 3, CCMI_NUM_RESOURCES = 4 } ccmi_resource;

/* KafkaMetricDef COMMON metrics that carry a resource group (monitor/metricdefinition/KafkaMetricDef.java:43-53) */
typedef enum ccmi_metric {
  CCMI_M_CPU_USAGE = 0,
  CCMI_M_DISK_USAGE = 1,
  CCMI_M_LEADER_BYTES_IN = 2,
  CCMI_M_LEADER_BYTES_OUT = 3,
  CCMI_M_REPLICATION_BYTES_IN = 4,
  CCMI_M_REPLICATION_BYTES_OUT = 5,
  CCMI_NUM_METRICS = 6
} ccmi_metric;

/* model/Broker.java State */
typedef enum ccmi_broker_state {
  CCMI_BROKER_ALIVE = 0,
  CCMI_BROKER_DEAD = 1,
  CCMI_BROKER_NEW = 2,
  CCMI_BROKER_DEMOTED = 3,
  CCMI_BROKER_BAD_DISKS = 4
} ccmi_broker_state;

/* model/Disk.java State (ALIVE, DEAD, DEMOTED) */
typedef enum ccmi_disk_state { CCMI_DISK_ALIVE = 0, CCMI_DISK_DEAD = 1, CCMI_DISK_DEMOTED = 2 } ccmi_disk_state;

/* analyzer/ActionType.java */
typedef enum ccmi_action_type {
  CCMI_INTER_BROKER_REPLICA_MOVEMENT = 0,
  CCMI_LEADERSHIP_MOVEMENT = 1,
  CCMI_INTER_BROKER_REPLICA_SWAP = 2,
  CCMI_INTRA_BROKER_REPLICA_MOVEMENT = 3,
  CCMI_INTRA_BROKER_REPLICA_SWAP = 4
} ccmi_action_type;

/* analyzer/ActionAcceptance.java */
typedef enum ccmi_acceptance { CCMI_ACCEPT = 0, CCMI_REPLICA_REJECT = 1, CCMI_BROKER_REJECT = 2 } ccmi_acceptance;

/* Goal plugins by reference simple class name (Goal.name(), AbstractGoal.java:141-144); numbering follows
 * the default.goals priority order (config/constants/AnalyzerConfig.java:352-367). */
typedef enum ccmi_goal_kind {
  CCMI_GOAL_RACK_AWARE = 0,                        /* RackAwareGoal */
  CCMI_GOAL_MIN_TOPIC_LEADERS_PER_BROKER = 1,      /* MinTopicLeadersPerBrokerGoal */
  CCMI_GOAL_REPLICA_CAPACITY = 2,                  /* ReplicaCapacityGoal */
  CCMI_GOAL_DISK_CAPACITY = 3,                     /* DiskCapacityGoal */
  CCMI_GOAL_NW_IN_CAPACITY = 4,                    /* NetworkInboundCapacityGoal */
  CCMI_GOAL_NW_OUT_CAPACITY = 5,                   /* NetworkOutboundCapacityGoal */
  CCMI_GOAL_CPU_CAPACITY = 6,                      /* CpuCapacityGoal */
  CCMI_GOAL_REPLICA_DISTRIBUTION = 7,              /* ReplicaDistributionGoal */
  CCMI_GOAL_POTENTIAL_NW_OUT = 8,                  /* PotentialNwOutGoal */
  CCMI_GOAL_DISK_USAGE_DISTRIBUTION = 9,           /* DiskUsageDistributionGoal */
  CCMI_GOAL_NW_IN_USAGE_DISTRIBUTION = 10,         /* NetworkInboundUsageDistributionGoal */
  CCMI_GOAL_NW_OUT_USAGE_DISTRIBUTION = 11,        /* NetworkOutboundUsageDistributionGoal */
  CCMI_GOAL_CPU_USAGE_DISTRIBUTION = 12,           /* CpuUsageDistributionGoal */
  CCMI_GOAL_TOPIC_REPLICA_DISTRIBUTION = 13,       /* TopicReplicaDistributionGoal */
  CCMI_GOAL_LEADER_REPLICA_DISTRIBUTION = 14,      /* LeaderReplicaDistributionGoal */
  CCMI_GOAL_LEADER_BYTES_IN_DISTRIBUTION = 15,     /* LeaderBytesInDistributionGoal */
  CCMI_GOAL_INTRA_BROKER_DISK_CAPACITY = 16,       /* IntraBrokerDiskCapacityGoal */
  CCMI_GOAL_INTRA_BROKER_DISK_USAGE_DISTRIBUTION = 17, /* IntraBrokerDiskUsageDistributionGoal */
  CCMI_GOAL_PREFERRED_LEADER_ELECTION = 18,         /* PreferredLeaderElectionGoal (not in default.goals) */
  CCMI_GOAL_RACK_AWARE_DISTRIBUTION = 19,           /* RackAwareDistributionGoal (not in default.goals) */
  CCMI_GOAL_BROKER_SET_AWARE = 20,                  /* BrokerSetAwareGoal (not in default.goals) */
  CCMI_GOAL_TOPIC_LEADER_REPLICA_DISTRIBUTION = 21, /* TopicLeaderReplicaDistributionGoal (ABI v7; in goals, not in
                                                       default.goals: AnalyzerConfig.java:297-319) */
  CCMI_GOAL_KAFKA_ASSIGNER_EVEN_RACK_AWARE = 22,     /* KafkaAssignerEvenRackAwareGoal (ABI v7; in goals) */
  CCMI_GOAL_KAFKA_ASSIGNER_DISK_USAGE_DISTRIBUTION = 23, /* KafkaAssignerDiskUsageDistributionGoal (ABI v7; in goals) */
  CCMI_GOAL_INTRA_BROKER_DISK_CAPACITY_EMPTY_DISKS = 24  /* new IntraBrokerDiskCapacityGoal(true), the goal of
                                                            RemoveDisksRunnable (additive at ABI v13; present exactly
                                                            when ccmi_session_mark_disks_for_removal is). Goal.name() is
                                                            IntraBrokerDiskCapacityGoal; an intra-broker kind wherever 16
                                                            is one, with 16's actionAcceptance. It also empties
                                                            zero-capacity disks: replicas of load 0 move too, such a
                                                            disk is over its limit while it has utilization or any
                                                            replica (an alive one that stays so fails the goal with
                                                            the over-limit message and its numDisks(1)
                                                            recommendation), and a dead one that keeps a replica
                                                            fails it with "Could not move all replicas from disk
                                                            ..." (no provision recommendation) */
} ccmi_goal_kind;

/* AnalyzerConfig replica.to.broker.set.mapping.policy.class (config/ReplicaToBrokerSetMappingPolicy.java) */
typedef enum ccmi_broker_set_policy {
  CCMI_BROKER_SET_TOPIC_NAME_HASH = 0,  /* TopicNameHashBrokerSetMappingPolicy (the default) */
  CCMI_BROKER_SET_ORIGINAL_BROKER = 1   /* ReplicaToOriginalBrokerSetMappingPolicy */
} ccmi_broker_set_policy;

/*
 * Flattened ClusterModel. Semantics of construction (mirrors the reference's model building):
 *   brokers are created in index order (broker_id[b] == b in ABI v1), then for r = 0..R-1 in index order
 *   replica r is created on replica_broker[r] (ClusterModel.createReplica) and its load is set
 *   (ClusterModel.setReplicaLoad) — so broker/host/cluster/potential-leadership aggregates accumulate in
 *   replica index order exactly as the Java model does (or, with replica_load_order, all replicas are created
 *   first and the loads are set in that order); finally each partition's replica list is put in
 *   partition_offset CSR order and broker states other than ALIVE are applied in broker index order
 *   (ClusterModel.setBrokerState).
 */
typedef struct ccmi_cluster_desc {
  int32_t num_windows;               /* W, 1..5 (num.partition.metrics.windows) */
  int32_t num_racks;
  int32_t num_brokers;               /* B */
  const int32_t* broker_id;          /* [B] */
  const int32_t* broker_rack;        /* [B] rack index */
  const int32_t* broker_state;       /* [B] ccmi_broker_state */
  const double* broker_capacity;     /* [B*4] ccmi_resource order */
  int32_t num_topics;                /* T */
  const char* const* topic_names;    /* [T] ASCII topic names (Replica.compareTo tie-break) */
  int32_t num_partitions;            /* P */
  const int32_t* partition_topic;    /* [P] */
  const int32_t* partition_number;   /* [P] */
  const int32_t* partition_offset;   /* [P+1] CSR into a permutation of replicas (Partition._replicas order) */
  const int32_t* partition_replicas; /* [R] replica indices, grouped by partition via partition_offset */
  int32_t num_replicas;              /* R */
  const int32_t* replica_partition;  /* [R] */
  const int32_t* replica_broker;     /* [R] */
  const uint8_t* replica_is_leader;  /* [R] */
  const uint8_t* replica_offline;    /* [R] isOriginalOffline flag (replica on a broken disk) */
  const float* replica_load;         /* [R * 6 * W] float window values, ccmi_metric order, newest first */
  /* Optional [R] permutation (NULL = interleaved). When set, every replica is created first (index order) and
   * ClusterModel.setReplicaLoad is then called in this order — the construction order of hand-built models such as
   * DeterministicCluster.mediumClusterModel (DeterministicCluster.java:1836-1879), where it changes the float
   * rounding of the broker / potential-leadership aggregates. */
  const int32_t* replica_load_order;
  /* Replica placement over disks (JBOD; Broker._diskByLogdir, model/Broker.java:56,80-83, model/Disk.java).
   * num_disks = 0: no placement information (Replica.disk() == null everywhere). Otherwise disk d belongs to
   * broker disk_broker[d], is named disk_logdir[d] (a broker's disks iterate in logdir String order, the TreeMap)
   * and has disk_capacity[d] (negative = dead disk, Disk.java:58-66; a dead broker's disks are dead).
   * replica_disk[r] is the disk given to ClusterModel.createReplica (the replica's original disk, -1 = none); its
   * utilization accumulates when the replica's load is set (Disk.addReplicaLoad). After the model is built, the
   * disk_assign pairs replay Disk.addReplica(replica) in order — the test fixture's placement step
   * (RandomCluster.java:315-331) for replicas created without a disk (their original disk stays null). */
  int32_t num_disks;
  const int32_t* disk_broker;        /* [D] */
  const char* const* disk_logdir;    /* [D] */
  const double* disk_capacity;       /* [D] */
  const int32_t* replica_disk;       /* [R] or NULL (all -1) */
  int32_t num_disk_assignments;
  const int32_t* disk_assign_replica; /* [num_disk_assignments] */
  const int32_t* disk_assign_disk;    /* [num_disk_assignments] */
  /* ABI v5: entries of replica_load_order (0 = num_replicas). A replica the order omits never gets
   * ClusterModel.setReplicaLoad: its Load stays empty (model/Load.java isEmpty), as in hand-built fixtures such as
   * DeterministicCluster.minLeaderReplicaPerBrokerSatisfiable (DeterministicCluster.java:321-361). */
  int32_t num_replica_loads;
  /* ABI v6: the host of every broker ([B] host index in [0, B), or NULL = each broker on a host of its own). Hosts
   * belong to a rack and are keyed by name within it (Rack._hosts.computeIfAbsent, model/Rack.java:256-262;
   * LoadMonitor passes node.host(), LoadMonitor.java:602), so brokers sharing an index must share a rack. ABI v8: a
   * host keeps the reference's aggregates (model/Host.java): the load of its brokers' replicas, updated with every
   * replica and leadership move in the reference's order; its capacity, the sum of its brokers' capacities in broker
   * index order minus those of dead brokers (Host.capacityFor: -1 without an alive broker); its replica count. The
   * host resources (Resource.isHostResource: CPU, NW_IN, NW_OUT) are checked against them where the reference does:
   * CapacityGoal.java:230-239,284-366,389-408,455-475, ResourceDistributionGoal.java:880-927,982-1037,
   * ClusterModel.aliveBrokers{Under,Over}Threshold / sortedAliveBrokersUnderThreshold (:1049-1126) and
   * ClusterModelStats.java:297-303. */
  const int32_t* broker_host;
  /* ABI v6: [D] 1 = the disk is Disk.State.DEMOTED (DemoteBrokerRunnable.java:144-148), or NULL. Only
   * PreferredLeaderElectionGoal reads it (PreferredLeaderElectionGoal.java:114-124). */
  const uint8_t* disk_demoted;
} ccmi_cluster_desc;

/* analyzer/BalancingConstraint.java; defaults AnalyzerConfig.java:58-464 via ccmi_default_constraint */
typedef struct ccmi_balancing_constraint {
  double resource_balance_percentage[4];
  double capacity_threshold[4];
  double low_utilization_threshold[4];
  double replica_balance_percentage;
  double leader_replica_balance_percentage;
  double topic_replica_balance_percentage;
  int32_t topic_replica_balance_min_gap;
  int32_t topic_replica_balance_max_gap;
  double goal_violation_distribution_threshold_multiplier;
  int64_t max_replicas_per_broker;
  int64_t overprovisioned_max_replicas_per_broker;
  int32_t overprovisioned_min_brokers;
  int32_t overprovisioned_min_extra_racks;
  /* BrokerSetAwareGoal (ABI v4): BalancingConstraint.brokerSetResolver() — the broker set id -> broker ids data of
   * BrokerSetFileResolver (config/BrokerSetFileResolver.java:42-82), whose brokers missing from every set the engine
   * assigns as NoOpBrokerSetAssignmentPolicy does (to "unmapped", NoOpBrokerSetAssignmentPolicy.java:70-86) — and
   * BalancingConstraint.replicaToBrokerSetMappingPolicy(). num_broker_sets = 0: no broker set data (BrokerSetAwareGoal
   * then fails as a BrokerSetResolutionException would, CCMI_E_INVALID). Other goals ignore these fields. */
  int32_t num_broker_sets;
  int32_t broker_set_policy;              /* ccmi_broker_set_policy */
  const char* const* broker_set_names;    /* [num_broker_sets] brokerSetId */
  const int32_t* broker_set_offset;       /* [num_broker_sets + 1] CSR into broker_set_members */
  const int32_t* broker_set_members;      /* broker indices of the session, in [0, B): a Kafka id's position in
                                           * ccmi_builder_broker_ids (ascending Kafka ids); -1 (any id outside
                                           * [0, B)) = a broker the model does not hold, ignored */
  /* MinTopicLeadersPerBrokerGoal (ABI v5): the topics topics.with.min.leaders.per.broker matches — the caller's
   * Utils.getTopicNamesMatchedWithPattern(BalancingConstraint.topicsWithMinLeadersPerBrokerPattern(), topics)
   * (common/Utils.java:26-36, BalancingConstraint.java:92,275-277), as topic indices of the session's desc (0 topics =
   * the default empty pattern) — and min.topic.leaders.per.broker (BalancingConstraint.java:93,285-287; 0 = the
   * dynamic leaders / eligible brokers). BrokerSetAwareGoal reads the same topic set (BrokerSetAwareGoal.java:
   * 136-139,262). */
  const int32_t* min_leader_topics;
  int32_t num_min_leader_topics;
  int32_t min_topic_leaders_per_broker;
  /* TopicLeaderReplicaDistributionGoal (ABI v7): topic.leader.replica.count.balance.threshold (default 1.10),
   * topic.leader.replica.count.balance.min.gap (2) / .max.gap (10) and
   * topic.leader.replica.distribution.goal.balance.margin (0.9) (AnalyzerConfig.java:112-146,
   * BalancingConstraint.java:85-88,145-167). */
  double topic_leader_replica_balance_percentage;
  int32_t topic_leader_replica_balance_min_gap;
  int32_t topic_leader_replica_balance_max_gap;
  double topic_leader_replica_balance_margin;
} ccmi_balancing_constraint;

/* analyzer/OptimizationOptions.java (7-field form) */
typedef struct ccmi_opt_options {
  const int32_t* excluded_topics; /* topic indices (OptimizationOptions.excludedTopics; every goal's
                                     selectReplicasBasedOnExcludedTopics and excluded-topic checks) */
  int32_t num_excluded_topics;
  const int32_t* excluded_brokers_for_leadership;
  int32_t num_excluded_brokers_for_leadership;
  const int32_t* excluded_brokers_for_replica_move;
  int32_t num_excluded_brokers_for_replica_move;
  int32_t triggered_by_goal_violation;
  const int32_t* requested_destination_broker_ids;
  int32_t num_requested_destination_broker_ids;
  int32_t only_move_immigrant_replicas;
  int32_t fast_mode; /* accepted for API parity. The reference's fast mode (default true) cuts per-broker loops at a
                        wall-clock timeout (AnalyzerConfig fast.mode.per.broker.move.timeout.ms, 500 ms), so its
                        result depends on host speed; the engine never cuts a loop short, i.e. it always returns
                        the result fast mode reaches when no timeout fires (= fast_mode 0). */
} ccmi_opt_options;

typedef struct ccmi_action {
  int32_t type;                  /* ccmi_action_type */
  int32_t partition;             /* partition index (desc order) */
  int32_t source_broker;
  int32_t destination_broker;
  int32_t destination_partition; /* swaps only, else -1 */
  int32_t source_disk;           /* intra-broker actions: disk indices (desc order), else -1. The action log records */
  int32_t destination_disk;      /* an intra-broker swap as its two relocateReplica(tp, broker, logdir) calls. */
} ccmi_action;

/* model/ClusterModelStats.java fields */
typedef struct ccmi_cluster_stats {
  double resource_avg[4], resource_max[4], resource_min[4], resource_std[4];
  int32_t num_balanced_brokers_by_resource[4];
  double potential_nw_out_avg, potential_nw_out_max, potential_nw_out_min, potential_nw_out_std;
  int32_t num_brokers_under_potential_nw_out;
  double replica_avg, replica_std;
  int32_t replica_max, replica_min;
  double leader_avg, leader_std;
  int32_t leader_max, leader_min;
  double topic_replica_avg, topic_replica_std;
  int32_t topic_replica_max, topic_replica_min;
  int32_t num_brokers, num_replicas_in_cluster, num_partitions_with_offline_replicas, num_topics;
  int32_t num_unbalanced_disks;
  double disk_utilization_std;
} ccmi_cluster_stats;

/* analyzer/ProvisionStatus.java */
typedef enum ccmi_provision_status {
  CCMI_PROVISION_UNDECIDED = 0,
  CCMI_PROVISION_RIGHT_SIZED = 1,
  CCMI_PROVISION_UNDER_PROVISIONED = 2,
  CCMI_PROVISION_OVER_PROVISIONED = 3
} ccmi_provision_status;

/* analyzer/ProvisionRecommendation.java: -1 = unset (DEFAULT_OPTIONAL_INT / DEFAULT_OPTIONAL_DOUBLE). The
 * recommendation's topic pattern and excluded rack ids are not carried. */
typedef struct ccmi_provision_recommendation {
  int32_t status;                 /* a ccmi_provision_status: UNDER or OVER */
  int32_t num_brokers, num_racks, num_disks, num_partitions;
  int32_t typical_broker_id;      /* broker id */
  int32_t resource;               /* ccmi resource index (CPU, NW_IN, NW_OUT, DISK) */
  int32_t pad;
  double typical_broker_capacity;
  double total_capacity;
} ccmi_provision_recommendation;

/* One goal's Goal.provisionResponse() (analyzer/ProvisionResponse.java): its status and, when the goal recorded one,
 * its own recommendation (recommendationByRecommender.get(goal name)). After an OptimizationFailureException the
 * status is UNDER_PROVISIONED with the exception's recommendation (AbstractGoal.java:125-126); on success it has been
 * through GoalUtils.validateProvisionResponse (:619-650). Aggregating goals' responses (ProvisionResponse.aggregate,
 * OptimizerResult's provision status) is the caller's, over the per-goal results. */
typedef struct ccmi_provision_response {
  int32_t status;                 /* ccmi_provision_status */
  int32_t has_recommendation;
  ccmi_provision_recommendation recommendation;
} ccmi_provision_response;

typedef struct ccmi_goal_result {
  int32_t goal_kind;
  int32_t succeeded;            /* Goal.optimize return value */
  int32_t has_diff;             /* AnalyzerUtils.hasDiff after this goal */
  double seconds;               /* wall time of the goal */
  int64_t candidates;           /* reference-equivalent candidate evaluations (BASELINE.md unit) */
  int64_t device_candidates;    /* candidates evaluated on the device, speculation included */
  int64_t device_launches;      /* scan-kernel launches */
  int64_t actions;              /* relocate* calls recorded in the action log */
  ccmi_cluster_stats stats;     /* ClusterModelStats after the goal (GoalOptimizer.statsByGoalPriority) */
  ccmi_provision_response provision;
} ccmi_goal_result;

/* Test fixture generator: RandomCluster properties (common/ClusterProperty.java + populate() flags) */
typedef struct ccmi_random_cluster_props {
  int32_t num_racks, num_brokers, num_dead_brokers, num_brokers_with_bad_disk;
  int32_t num_replicas, num_topics, min_replication, max_replication;
  double mean_cpu, mean_disk, mean_nw_in, mean_nw_out;
  int32_t distribution;          /* 0 UNIFORM, 1 LINEAR, 2 EXPONENTIAL */
  int32_t rack_aware;
  int32_t leader_in_first_position;
  /* POPULATE_REPLICA_PLACEMENT_INFO: 0 none; 1 the reference's JBOD capacity file (testCapacityConfigJBOD.json:
   * brokers 0/1/2 overridden, default broker 10 logdirs); 2 every broker num_logdirs logdirs "/mnt/d<i>" with
   * capacities logdir_capacity[i] (the C4 layout; non-disk capacities from DefaultCapacityConfig.json). */
  int32_t jbod;
  int32_t num_logdirs;
  double logdir_capacity[8];
} ccmi_random_cluster_props;

typedef struct ccmi_session ccmi_session;
typedef struct ccmi_cluster_buffers ccmi_cluster_buffers; /* owns the arrays behind a generated desc */

const char* ccmi_last_error(void);
int32_t ccmi_abi_version(void);
/* Number of visible gfx950 devices (on an MI355X node: HIP ordinals 0..n-1, the `device` of ccmi_session_create);
 * 0 when none. What-if batches (GoalViolationDetector) spread their sessions over them. */
int32_t ccmi_device_count(void);
void ccmi_default_constraint(ccmi_balancing_constraint* out);
void ccmi_default_random_cluster_props(ccmi_random_cluster_props* out); /* TestConstants.BASE_PROPERTIES */

ccmi_status ccmi_random_cluster(const ccmi_random_cluster_props* props, ccmi_cluster_buffers** out);
/* TopicNameHashBrokerSetMappingPolicy.brokerSetIdForTopic (config/TopicNameHashBrokerSetMappingPolicy.java:60-70): the
 * index, in String order of the broker set ids, of the set a topic maps to among num_broker_sets sets —
 * Guava Hashing.consistentHash(|murmur3_128(topic, UTF-8).asInt()|, num_broker_sets). -1 if num_broker_sets < 1. */
int32_t ccmi_topic_broker_set(const char* topic, int32_t num_broker_sets);
const ccmi_cluster_desc* ccmi_cluster_buffers_desc(const ccmi_cluster_buffers* buf);
void ccmi_cluster_buffers_free(ccmi_cluster_buffers* buf);

/*
 * Model ingestion: LoadMonitor.clusterModel (monitor/LoadMonitor.java:491-543) builds the ClusterModel from the Kafka
 * metadata, the broker capacities and each partition's aggregated leader metrics; this builder takes the same calls
 * and produces the flattened ccmi_cluster_desc directly (no Java ClusterModel needed for the engine's side):
 *   ccmi_builder_create_broker  ClusterModel.createRack + createBroker for a live node (populateClusterCapacity
 *                               :563-600), or handleDeadBroker for a dead one (alive = 0; a no-op if it exists)
 *   ccmi_builder_add_disk       a logdir of a JBOD broker (BrokerCapacityInfo.diskCapacityByLogDir)
 *   ccmi_builder_populate_partition
 *                               MonitorUtils.populatePartitionLoad (MonitorUtils.java:415-479): one createReplica +
 *                               setReplicaLoad per replica of PartitionInfo.replicas() in order, the loads derived
 *                               from the partition's aggregated leader metrics by getAggregatedMetricValues (:215-265):
 *                               CPU unit interval -> percentage once per partition, the leader's replication bytes
 *                               out = leader bytes in x followers, a follower's NW_OUT = 0 and CPU from
 *                               ModelUtils.getFollowerCpuUtilFromLeaderLoad (0.7 / 0.15 / 0.15 weights), all in the
 *                               reference's float MetricValues arithmetic. leader_broker_id < 0 = offline partition
 *                               (no replicas created, LoadMonitor logs and skips it).
 *   ccmi_builder_set_broker_state  setBadBrokerState (MonitorUtils.java:349-356) and NEW / DEMOTED marking
 *   ccmi_builder_desc           the flattened model (valid until ccmi_builder_destroy). Brokers are indexed in
 *                               ascending id order; broker_id[b] = b in the desc, and ccmi_builder_broker_ids maps an
 *                               index back to the Kafka broker id (HashSet<Broker> iteration ties follow the dense
 *                               index, which equals the reference's order when the ids are 0..B-1).
 * leader_metrics: [6 * W] floats, ccmi_metric order, newest window first (ValuesAndExtrapolations.metricValues()).
 */
typedef struct ccmi_model_builder ccmi_model_builder;
ccmi_status ccmi_builder_create(int32_t num_windows, ccmi_model_builder** out);
void ccmi_builder_destroy(ccmi_model_builder* b);
ccmi_status ccmi_builder_create_broker(ccmi_model_builder* b, const char* rack, const char* host, int32_t broker_id,
                                       const double capacity[4], int32_t alive);
ccmi_status ccmi_builder_add_disk(ccmi_model_builder* b, int32_t broker_id, const char* logdir, double capacity);
ccmi_status ccmi_builder_populate_partition(ccmi_model_builder* b, const char* topic, int32_t partition,
                                            const int32_t* replica_broker_ids, int32_t num_replicas,
                                            int32_t leader_broker_id, const uint8_t* offline,
                                            const char* const* logdirs, const float* leader_metrics);
ccmi_status ccmi_builder_set_broker_state(ccmi_model_builder* b, int32_t broker_id, int32_t state);
/* Disk.setState for a disk added with ccmi_builder_add_disk: CCMI_DISK_ALIVE or CCMI_DISK_DEMOTED (a dead disk is
 * given by a negative capacity). */
ccmi_status ccmi_builder_set_disk_state(ccmi_model_builder* b, int32_t broker_id, const char* logdir, int32_t state);
ccmi_status ccmi_builder_desc(ccmi_model_builder* b, ccmi_cluster_desc* out);
ccmi_status ccmi_builder_broker_ids(const ccmi_model_builder* b, int32_t* out);

/* device_ordinal: the HIP device the session's tables live on (one session = one device). Destination-sharded
 * sessions are one per process and GPU, joined by ccmi_session_set_shard / ccmi_session_attach_rccl below. */
ccmi_status ccmi_session_create(int32_t device_ordinal, const ccmi_cluster_desc* desc, ccmi_session** out);
ccmi_status ccmi_session_destroy(ccmi_session* s);

/* Run a whole goal chain (GoalOptimizer.optimizations). results: caller array of n_goals entries. Every goal's
 * optimizedGoals are the goals before it in this call (GoalOptimizer.java:449,467-471), not earlier calls' goals. */
ccmi_status ccmi_optimizations(ccmi_session* s, const int32_t* goal_kinds, int32_t n_goals,
                               const ccmi_balancing_constraint* constraint, const ccmi_opt_options* options,
                               ccmi_goal_result* results);
/*
 * Goal.optimize(ClusterModel, Set<Goal> optimizedGoals, OptimizationOptions) (analyzer/goals/Goal.java:60-68,
 * AbstractGoal.java:81-135). The session keeps every goal it has optimized — one per goal kind, as GoalOptimizer keeps
 * one instance per goal class, a re-optimized kind replacing its older entry — with the frozen state its
 * actionAcceptance reads. optimized_goal_kinds[0, num_optimized_goals) is the caller's optimizedGoals set (ABI v8): only
 * those goals' actionAcceptance joins the candidate conjunction (AnalyzerUtils.isProposalAcceptableForOptimizedGoals,
 * AnalyzerUtils.java:169-179), whatever else the session has run. GoalOptimizer passes the goals optimized earlier in the
 * same optimizations() call; GoalViolationDetector passes the empty set on a model it reuses across goals
 * (GoalViolationDetector.java:193-211,314). Duplicate kinds count once; order does not matter.
 * A kind the session has not optimized — a goal whose optimize ran in the JVM, or a goal class that exists only in the
 * JVM (pass any kind outside ccmi_goal_kind, e.g. -1) — returns CCMI_E_UNSUPPORTED before anything changes: its
 * actionAcceptance is not available to the device, so the caller runs this goal in the JVM instead.
 */
ccmi_status ccmi_goal_optimize(ccmi_session* s, int32_t goal_kind, const int32_t* optimized_goal_kinds,
                               int32_t num_optimized_goals, const ccmi_balancing_constraint* constraint,
                               const ccmi_opt_options* options, ccmi_goal_result* result);
/* Acceptance of an action by the i-th goal the session holds (the goals it has optimized, one per kind, in the order
 * each was last optimized: after one ccmi_optimizations call on a fresh session, the chain position). */
ccmi_status ccmi_action_acceptance(ccmi_session* s, int32_t optimized_goal_index, const ccmi_action* action,
                                   int32_t* acceptance);
/* Goal.actionAcceptance keyed by the goal plugin (ccmi_goal_kind) instead of the chain position: the most recently
 * optimized goal of that kind (GoalOptimizer holds one instance per goal class). CCMI_E_INVALID when the session
 * has not optimized that kind. */
ccmi_status ccmi_action_acceptance_by_kind(ccmi_session* s, int32_t goal_kind, const ccmi_action* action,
                                           int32_t* acceptance);
/* ABI v13. Goal.actionAcceptance for a batch: acceptance[i * num_goals + g] is what
 * ccmi_action_acceptance_by_kind(s, goal_kinds[g], &actions[i], ..) returns on the session's current model
 * (a ccmi_acceptance value). The session is not changed. The cells run on the device in one launch per chunk of actions
 * (a JVM goal late in a mixed chain asks every optimized goal about every candidate, AnalyzerUtils.java:169-179); only
 * the cells of an intra-broker goal are answered on the host. Errors are those of the single call, decided before
 * anything runs on the device: a kind the session has not optimized is CCMI_E_INVALID, a goal whose actionAcceptance
 * throws IllegalStateException CCMI_E_STATE, an action the single call refuses CCMI_E_INVALID with *first_invalid (when
 * given) set to its index (-1 for every other error). On error the output is unspecified. n == 0 is CCMI_OK; duplicate
 * kinds give duplicate columns. A sharded session answers locally (every shard holds the whole model). */
ccmi_status ccmi_actions_acceptance(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                    const ccmi_action* actions, int64_t n, int8_t* acceptance,
                                    int64_t* first_invalid /* optional */);
/* One source of a destination-broker mask: the replica of `partition` on `source_broker` that moves
 * (CCMI_INTER_BROKER_REPLICA_MOVEMENT) or gives up leadership (CCMI_LEADERSHIP_MOVEMENT). */
typedef struct ccmi_move_source {
  int32_t type;           /* CCMI_INTER_BROKER_REPLICA_MOVEMENT or CCMI_LEADERSHIP_MOVEMENT */
  int32_t partition;      /* partition index (desc order) */
  int32_t source_broker;  /* the broker whose replica of the partition moves / gives up leadership */
  int32_t reserved;       /* 0 */
} ccmi_move_source;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). The destination brokers of a replica-move or
 * leadership-move loop (AbstractGoal.maybeApplyBalancingAction, AbstractGoal.java:243-270) for a batch of sources, one
 * bit per broker: with W = (num_brokers + 63) / 64, bit (b & 63) of mask[i * W + (b >> 6)] is set iff
 * b != sources[i].source_broker, GoalUtils.legitMove holds for (the source replica, broker b, the type) — a replica move:
 * b neither hosts the partition nor is one of its ineligible brokers; a leadership move: the source replica is the leader
 * and b hosts a replica of the partition — and every goal of goal_kinds (each the session's latest optimization of that
 * kind) returns ACCEPT for that action on the session's current model; either reject code clears the bit. Bits of
 * positions >= num_brokers are 0. num_goals == 0 gives the pure legit mask; duplicate kinds are harmless; any number of
 * goals is allowed. The session is not changed. The whole grid runs on the device (one wavefront per output word); the
 * host does no per-candidate work. The option filters of GoalUtils.eligibleBrokers (excluded brokers, NEW brokers,
 * requested destinations) stay the caller's: it ANDs the mask with its own candidate set. Swap candidates are replica
 * pairs, not brokers: ccmi_swaps_acceptance_grid below answers them.
 * Errors, all decided before anything runs on the device: CCMI_E_UNSUPPORTED for an intra-broker goal kind (such goals
 * share no chain with inter-broker goals; their host-answered cells stay with the batched verdict call),
 * CCMI_E_INVALID for a kind the session has not optimized, CCMI_E_STATE for a goal whose actionAcceptance throws
 * IllegalStateException, CCMI_E_INVALID with *first_invalid (when given) set to the source's index for a source of
 * another action type, with a partition or broker out of range, or without a replica of the partition on the source
 * broker; *first_invalid is -1 for every other error and on success. On error the output is unspecified. n == 0 is
 * CCMI_OK. A sharded session answers locally. */
ccmi_status ccmi_moves_acceptance_mask(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                       const ccmi_move_source* sources, int64_t n,
                                       uint64_t* mask /* [n * W], W = (num_brokers + 63) / 64 */,
                                       int64_t* first_invalid /* optional */);
/* One replica of a swap grid: the replica of `partition` on `broker`. */
typedef struct ccmi_swap_replica {
  int32_t partition; /* partition index (desc order) */
  int32_t broker;    /* broker index */
} ccmi_swap_replica;
/* The code of one (source replica, candidate replica) pair of a swap grid, in the order the loop body of
 * AbstractGoal.maybeApplySwapAction decides it. */
typedef enum ccmi_swap_code {
  CCMI_SWAP_ACCEPT = 0,              /* legit both ways and every goal ACCEPTs */
  CCMI_SWAP_REPLICA_REJECT = 1,      /* first non-ACCEPT verdict in goal_kinds order */
  CCMI_SWAP_BROKER_REJECT = 2,       /* first non-ACCEPT verdict in goal_kinds order */
  CCMI_SWAP_SOURCE_NOT_LEGIT = 3,    /* legitMove(source, candidate's broker) fails: AbstractGoal.java:308, return null */
  CCMI_SWAP_CANDIDATE_NOT_LEGIT = 4  /* legitMove(candidate, source's broker) fails: AbstractGoal.java:313, continue */
} ccmi_swap_code;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). The candidate loop of a swap
 * (AbstractGoal.maybeApplySwapAction, AbstractGoal.java:287-338) for n source replicas against m candidate replicas:
 * codes[i * m + j] is the ccmi_swap_code of swapping sources[i] with candidates[j], the destination broker being the
 * candidate's current broker. The checks run in the reference's order. First GoalUtils.legitMove(source, candidate's
 * broker, INTER_BROKER_REPLICA_MOVEMENT) — the broker neither hosts the source's partition nor is one of its ineligible
 * brokers — else 3 (also when both checks fail); then legitMove(candidate, source's broker), else 4; then the goals of
 * goal_kinds in that order (each the session's latest optimization of that kind) on the session's current model: the
 * code is the first verdict that is not ACCEPT (AnalyzerUtils.isProposalAcceptableForOptimizedGoals,
 * AnalyzerUtils.java:169-179), or 0 when there is none. The order of goal_kinds matters; a kind named twice is
 * harmless. num_goals == 0 gives the pure legitimacy grid (codes 0, 3, 4); any number of goals is allowed. A candidate
 * on the source's own broker, of the source's partition, or equal to the source fails the first check and is 3: no
 * special cases. Candidates may sit on any mix of brokers (several candidate brokers' replicas in one call) and may
 * repeat. m is at most 2^31 - 64. The session is not changed. The whole grid runs on the device (one wavefront per 64
 * candidates of a source); the host resolves n + m replicas and does no per-pair work. The goal's own selfSatisfied and
 * GoalUtils.eligibleReplicasForSwap (excluded topics and brokers, NEW-broker rules) stay the caller's.
 * Errors, all decided before anything runs on the device: CCMI_E_UNSUPPORTED for an intra-broker goal kind,
 * CCMI_E_INVALID for a kind the session has not optimized, CCMI_E_STATE for a goal whose actionAcceptance throws
 * IllegalStateException, CCMI_E_INVALID with *first_invalid (when given) set to i for sources[i] or n + j for
 * candidates[j] (sources are checked first) with a partition or broker out of range or without a replica of the
 * partition on the broker; *first_invalid is -1 for every other error and on success. On error the output is
 * unspecified. n == 0 or m == 0 is CCMI_OK once the kinds are checked. A sharded session answers locally. */
ccmi_status ccmi_swaps_acceptance_grid(ccmi_session* s, const int32_t* goal_kinds, int32_t num_goals,
                                       const ccmi_swap_replica* sources, int64_t n,
                                       const ccmi_swap_replica* candidates, int64_t m,
                                       int8_t* codes /* [n * m], codes[i * m + j] */,
                                       int64_t* first_invalid /* optional */);
/* Session update by deltas: apply actions decided outside this session (a JVM goal earlier in a mixed chain, an
 * executed proposal batch) to the resident model, in order, as ClusterModel.relocateReplica /
 * relocateLeadership / relocateReplica(tp, broker, logdir) do (a swap is its two relocateReplica calls,
 * AbstractGoal.maybeApplySwapAction :316-317). Only the touched rows are re-sent to the device, so a mixed-chain hop
 * costs O(actions), not an O(R) re-flatten. Actions are validated first (the replica exists on the source, the
 * destination does not host the partition / hosts a follower, disks belong to the broker); the first invalid one
 * fails the call with CCMI_E_INVALID and `*applied` (optional) = actions applied before it. Applied actions join
 * the action log and the proposals (the diff against the session's initial placement). */
ccmi_status ccmi_session_apply(ccmi_session* s, const ccmi_action* actions, int64_t n, int64_t* applied);
/* RemoveDisksRunnable.checkCanRemoveDisks (:131-161), then Disk.markDiskForRemoval (capacity := 0) on every listed
 * disk, all or nothing (additive at ABI v13; its presence is the capability flag, also of goal kind 24). `disks` are
 * desc disk indices; duplicates are harmless. The brokers named are checked in ascending broker index, each in this
 * order: every disk of the broker listed (dead disks count) -> CCMI_E_INVALID "No log dir remaining to move replicas to
 * for broker %d."; futureUsage / remainingCapacity > disk_capacity_threshold -> CCMI_E_INVALID "Not enough remaining
 * capacity to move replicas to for broker %d.", futureUsage the sum of Disk._utilization over all of the broker's disks
 * and remainingCapacity the sum of capacity() over those not listed, both in logdir order as doubles (a dead disk's -1
 * is added like any capacity; 0/0 and x/0 compare as in Java). A disk index out of range is CCMI_E_INVALID with
 * *first_invalid (optional) = its position in `disks`, the reference's "Invalid log dirs provided for broker %d.";
 * *first_invalid is -1 otherwise. CCMI_E_STATE when the session has optimized a goal or its action log is not empty
 * (the runnable starts from a fresh model); CCMI_E_INVALID for a NULL session, n < 0, NULL disks with n > 0, or a desc
 * without disks. On success the listed disks' capacity is 0.0 in the host model and in the device disk table (the
 * session's disk tables are sent again); a dead disk stays dead; broker capacities do not change. Every query then answers as a
 * fresh session created from the same desc with those disk_capacity entries 0.0. Nothing changes on failure. */
ccmi_status ccmi_session_mark_disks_for_removal(ccmi_session* s, const int32_t* disks, int32_t n,
                                                double disk_capacity_threshold, int32_t* first_invalid /* optional */);
/* Goal.provisionResponse of the goal whose OptimizationFailureException (CCMI_E_OPT_FAILURE) ended the session's last
 * optimization call: UNDER_PROVISIONED with the exception's ProvisionRecommendation (AbstractGoal.java:125-130). */
ccmi_status ccmi_last_failure_provision(const ccmi_session* s, ccmi_provision_response* out);
ccmi_status ccmi_compute_cluster_stats(ccmi_session* s, const ccmi_balancing_constraint* constraint,
                               const ccmi_opt_options* options, ccmi_cluster_stats* out);

/* servlet/response/stats/BasicStats.java of one broker (SingleBrokerStats) or one host (SingleHostStats). 128 bytes. */
typedef struct ccmi_basic_stats {
  double disk_mb, disk_pct, cpu_pct, leader_nw_in_rate, follower_nw_in_rate, nw_out_rate, pnw_out_rate;
  double disk_capacity_mb, network_in_capacity, network_out_capacity, num_core;
  int32_t replicas, leaders;
  int32_t broker;   /* broker index; -1 in a host row */
  int32_t state;    /* ccmi_broker_state; -1 in a host row */
  int32_t host;     /* host index (desc.broker_host value, or the broker index when that is NULL) */
  int32_t rack;
  int32_t reserved[4]; /* 0 */
} ccmi_basic_stats;
/* model/DiskStats.java (Disk.diskStats, Disk.java:259-264) of one disk, desc disk order. */
typedef struct ccmi_disk_stats {
  double disk_mb, disk_pct;  /* both -1 for a disk with capacity <= 0 (the reference's null / "DEAD") */
  double capacity;
  int32_t num_replicas, num_leader_replicas, disk, broker;
} ccmi_disk_stats;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). ClusterModel.brokerStats
 * (ClusterModel.java:1303-1309) of the session's current model, computed on the device from the resident tables: what
 * GoalOptimizer.java:442 takes before the first goal, OptimizerResult.java:111 after the last, and LoadMonitor.java:446
 * for the load endpoint.
 * brokers[b] is BasicStats(Broker, potentialBytesOutRate) (BasicStats.java:73-86) of broker b, every Math.max(x, 0.0)
 * as Java evaluates it (NaN stays NaN, -0.0 becomes 0.0): disk_mb = max(broker.replicas().isEmpty() ? 0 :
 * load.expectedUtilizationFor(DISK), 0); cpu_pct = max(100.0 * utilization(CPU) / capacityFor(CPU), 0) (a dead broker's
 * capacity is -1, so 0); leader_nw_in_rate = max(leadershipLoadForNwResources().expectedUtilizationFor(NW_IN), 0);
 * follower_nw_in_rate = max(utilization(NW_IN) - leader_nw_in_rate, 0); nw_out_rate = max(utilization(NW_OUT), 0);
 * pnw_out_rate = max(potentialLeadershipLoadFor(b).expectedUtilizationFor(NW_OUT), 0); disk_capacity_mb,
 * network_in_capacity, network_out_capacity = max(capacityFor(DISK | NW_IN | NW_OUT), 0); num_core = max(capacityFor(CPU)
 * / 100, 0); disk_pct = disk_capacity_mb > 0 ? 100 * disk_mb / disk_capacity_mb : -1 (diskUtilPct, :94-96); replicas and
 * leaders are broker.replicas().size() and broker.leaderReplicas().size(). The loads are the broker's own
 * (broker.load()), never its host's, also when brokers share hosts. The reference's isEstimated flag
 * (SingleBrokerStats) is not carried: the desc holds no capacity-estimation information.
 * hosts (optional, room for B rows): one row per distinct host in ascending host index, each the
 * SingleHostStats.addBasicStats sum (BasicStats.java:142-155) of the host's broker rows in ascending broker index
 * (ClusterModel.brokers() is a TreeSet and the index order is id order), every field added in double in that order,
 * disk_pct recomputed from the sums, rack the rack of the host's brokers, broker = state = -1; *num_hosts (optional)
 * receives the row count. Ordering the hosts by name (the reference's ConcurrentSkipListMap) stays with the caller,
 * which holds the names.
 * disks (read only when the desc has num_disks > 0; optional): Disk.diskStats() of every disk in desc disk order.
 * num_replicas is Disk._replicas.size() as the model keeps it — a replica an inter-broker move took away stays in its
 * old disk's set (Broker.removeReplica does not touch disks) — num_leader_replicas its members with isLeader(),
 * disk_mb Disk._utilization, disk_pct = disk_mb * 100.0 / capacity (DiskStats.java:54-56); disk_mb = disk_pct = -1 when
 * capacity <= 0 (DiskStats' null utilization, "DEAD" in its JSON).
 * The session is not changed. Valid on a fresh session (the stats before optimization), after any optimization and
 * after ccmi_session_apply with no scan in between (the pending rows are sent first). A sharded session answers locally.
 * No perf counter of the acceptance calls counts it. Errors: CCMI_E_INVALID for a NULL session or NULL brokers,
 * CCMI_E_DEVICE for a device failure; on error the outputs are unspecified. */
ccmi_status ccmi_broker_stats(ccmi_session* s, ccmi_basic_stats* brokers /* [B] */,
                              ccmi_basic_stats* hosts /* [B] capacity, or NULL */, int32_t* num_hosts /* or NULL */,
                              ccmi_disk_stats* disks /* [num_disks], or NULL */);

/* The parameters of a partition load request (PartitionLoadParameters). 64 bytes. */
typedef struct ccmi_partition_load_query {
  int32_t resource;         /* ccmi_resource: the sort key (PartitionLoadParameters.resource(), default DISK) */
  int32_t want_max_load;    /* 0 / 1 */
  int32_t want_avg_load;    /* 0 / 1 */
  int32_t entries;          /* at most this many records (Integer.MAX_VALUE = all) */
  int32_t partition_lower;  /* keep partition_number in [lower, upper], both inclusive */
  int32_t partition_upper;  /* (Integer.MIN_VALUE / MAX_VALUE = no bound) */
  int32_t reserved[4];      /* 0 (they bring the struct to 64 bytes) */
  const uint8_t* topic_selected;  /* [T] or NULL = every topic: the caller evaluates its regex on the names */
  const uint8_t* broker_selected;  /* [B] or NULL = every broker (brokerIds empty) */
  const int32_t* tie_rank;         /* [P] or NULL = the partition index */
} ccmi_partition_load_query;
/* One PartitionLoadState record (PartitionLoadState.java:56-151). 80 bytes. */
typedef struct ccmi_partition_load_record {
  double util[4];        /* ccmi_resource order, all four under the query's max / avg flags */
  int32_t partition;     /* partition index (desc order) */
  int32_t num_replicas;
  int32_t brokers[8];    /* current broker index of every replica in Partition._replicas order: [0] the leader,
                            [1, num_replicas) the followers as Partition.followers() lists them; -1 beyond */
  int32_t reserved[2];   /* 0 */
} ccmi_partition_load_record;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). The partition load response of the session's
 * current model (PartitionLoadRunnable.getResult, PartitionLoadRunnable.java:32-60): the selected partitions ordered by
 * the utilization of q->resource on their current leader, computed and sorted on the device from the resident tables.
 * Values: util[res] = partition.leader().load().expectedUtilizationFor(res, wantMaxLoad, wantAvgLoad) (Load.java:81-95):
 * 0.0 for an empty load; else Math.max(0.0 + sum over the resource's metrics of (double) f(m), 0.0) with the metrics
 * CPU: [CPU], DISK: [DISK], NW_IN: [LEADER_BYTES_IN, REPLICATION_BYTES_IN], NW_OUT: [LEADER_BYTES_OUT,
 * REPLICATION_BYTES_OUT] and the float f(m) = MetricValues.max() with want_max_load, latest() (window 0) for DISK without
 * want_avg_load, avg() = (float)(sum / W) otherwise; Math.max(x, 0.0) as Java evaluates it (-0.0 becomes 0.0). NaN loads
 * are outside the contract.
 * MetricValues.max() returns a cached _max (MetricValues.java:20, :165-171) that set() can leave stale (:39-45). For a
 * replica that is currently the leader it nevertheless equals Math.max(Float.MIN_VALUE, max_i v[i]), which is what the
 * call computes: every add / subtract recomputes _max from Float.MIN_VALUE over all windows (:86-92, :106-112, :126-131,
 * :146-152); DISK, LEADER_BYTES_IN and REPLICATION_BYTES_IN of a replica are written once, by the add of
 * Load.initializeMetricValues (Load.java:207-213), and never by set(); CPU, LEADER_BYTES_OUT and REPLICATION_BYTES_OUT of
 * a leader were last written either by that same add (a leader since ingestion) or by makeLeader's Load.addLoad
 * (Replica.java:306, Load.java:241-245), again an add — makeFollower's set() calls and clears happen only while the
 * replica stops being the leader; and since _max >= Float.MIN_VALUE > 0 always, max() never takes its updateMax() branch
 * (:166-170). So a leader whose windows are all zero (or negative) reports 2^-149 per metric in max mode, not 0, and a
 * leader with an empty load 0.0. The response reads leaders only.
 * MESSAGE_IN_RATE (the reference's msg_in column) is not one of the six metrics the model carries: it is left out.
 * Order: partitionList.sort((o1, o2) -> Double.compare(o2, o1)) on util[q->resource], descending. Among exactly equal
 * keys the reference's order is the iteration order of its HashMap<TopicPartition, Partition>, which the device does not
 * hold: the caller passes it as tie_rank. Equal keys come in ascending tie_rank[p], then ascending partition index — a
 * total order for any tie_rank contents (values may repeat and are compared as signed 32-bit integers).
 * Selection (PartitionLoadRunnable.java:45-50, PartitionLoadState.shouldSkipPartition), before the entries cut: a
 * partition is kept when topic_selected[topic] != 0 (or the array is NULL), its partition number lies in
 * [partition_lower, partition_upper], and some current broker b of it has broker_selected[b] != 0 (or the array is
 * NULL). *num_selected (optional) receives the number kept, *num_records = min(entries, kept), and records[0,
 * *num_records) the first partitions of the order; records has room for min(entries, P) rows.
 * The session is not changed. Valid on a fresh session, after any optimization and after ccmi_session_apply with nothing
 * in between (the pending rows and loads are sent first). A sharded session answers locally. The launches count into
 * stats_launches, stats_bytes and stats_kernel_ms of ccmi_perf_counters, as ccmi_broker_stats; no acceptance counter
 * counts them.
 * Errors, all before any launch: CCMI_E_INVALID for both flags set (the IllegalArgumentException of Load.java:82-84), a
 * flag other than 0 / 1, resource outside [0, 4), entries < 0, a NULL s, q or num_records, or NULL records with
 * entries > 0 and P > 0. partition_lower > partition_upper is CCMI_OK with 0 records. CCMI_E_DEVICE for a device failure;
 * on error the outputs are unspecified. */
ccmi_status ccmi_partition_load(ccmi_session* s, const ccmi_partition_load_query* q,
                                ccmi_partition_load_record* records /* [min(entries, P)] */,
                                int64_t* num_records, int64_t* num_selected /* optional */);

int64_t ccmi_action_log_count(const ccmi_session* s);
ccmi_status ccmi_action_log_copy(const ccmi_session* s, int64_t first, int64_t count, ccmi_action* out);
/* [R] current broker of each replica slot in partition CSR order / [P] leader broker per partition */
ccmi_status ccmi_replica_distribution(const ccmi_session* s, int32_t* out);
ccmi_status ccmi_leader_distribution(const ccmi_session* s, int32_t* out);
/* [R] current disk of each replica slot in partition CSR order (-1 = no disk) */
ccmi_status ccmi_replica_disks(const ccmi_session* s, int32_t* out);
/* ExecutionProposals: count, then per proposal: partition, size, old leader, RF; old and new broker lists
 * (new list leader-first) packed into old_out/new_out with stride max_rf. */
int64_t ccmi_proposal_count(const ccmi_session* s);
ccmi_status ccmi_proposals(const ccmi_session* s, int32_t max_rf, int32_t* partition, int32_t* size,
                           int32_t* old_leader, int32_t* old_out, int32_t* new_out);
/* The logdir half of the proposals' ReplicaPlacementInfo lists (disk indices, -1 = none), same packing. */
ccmi_status ccmi_proposal_disks(const ccmi_session* s, int32_t max_rf, int32_t* old_disk_out, int32_t* new_disk_out);

/* One ExecutionProposal of the current model against the session's initial placement. 160 bytes, ten 16-byte stores.
 * Brokers are broker indices, disks disk indices (the logdir half of ReplicaPlacementInfo). */
typedef struct ccmi_proposal_record {
  int32_t partition;         /* partition index (desc order) */
  int32_t size;              /* (int) leader.load().expectedUtilizationFor(DISK) of the current leader, Java narrowing:
                                toward zero, saturating, NaN -> 0 */
  int32_t old_leader;        /* the initial leader's broker */
  int32_t old_leader_disk;   /* the initial leader's disk, -1 = none */
  int32_t num_replicas;
  int32_t flags;             /* bit 0 hasReplicaAction: the old and new (broker, disk) sets differ
                                (ExecutionProposal.java:212-214); bit 1 hasLeaderAction: the old leader's placement is
                                not new_replicas[0]'s (:219-221) */
  int32_t num_to_add;        /* |replicasToAdd|: new brokers that are not old brokers (:74) */
  int32_t num_between_disks; /* |replicasToMoveBetweenDisksByBroker|: new (broker, disk) pairs on a kept broker that are
                                not old pairs (:76-78) */
  int32_t old_replicas[8];   /* the initial brokers in Partition._replicas order; unused = -1 */
  int32_t new_replicas[8];   /* the current brokers, the leader first (getDiff :84-88: position 0 and the leader's
                                position swap, nothing else moves); unused = -1 */
  int32_t old_disks[8];      /* the disks of old_replicas, same order; -1 = none */
  int32_t new_disks[8];      /* the disks of new_replicas, same order; -1 = none */
} ccmi_proposal_record;
/* OptimizerResult.getMovementStats (OptimizerResult.java:258-278) over every proposal. 64 bytes. */
typedef struct ccmi_proposal_summary {
  int64_t num_proposals;     /* all of them, whatever the capacity of the call */
  int64_t num_inter_broker_replica_movements;
  int64_t inter_broker_data_to_move_mb;
  int64_t num_intra_broker_replica_movements;
  int64_t intra_broker_data_to_move_mb;
  int64_t num_leadership_movements;
  int64_t reserved[2];       /* 0 */
} ccmi_proposal_summary;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). AnalyzerUtils.getDiff (AnalyzerUtils.java:63-93)
 * of the session's current model against the placement it was created with, and the movement statistics of the result,
 * diffed, compacted and summed on the device from the resident tables. ccmi_proposals / ccmi_proposal_disks return the
 * same proposals from the host's list, which only an optimization or ccmi_session_apply rebuilds; this call reads the
 * model as it is and leaves that list alone.
 * A partition gets a record when its current (broker, disk) list in Partition._replicas order differs from the initial
 * one or its current leader's (broker, disk) differs from the initial leader's: the `continue` test of getDiff :80.
 * Records come in ascending partition index, the order of ccmi_proposals.
 * capacity is the room in records; records[0, min(capacity, num_proposals)) are written and *num_records is that
 * minimum; nothing past it is touched. summary->num_proposals is always the whole count, so records == NULL with
 * capacity == 0 is the summary-only call and sizes the buffer of a second one. summary may be NULL.
 * The summary follows getMovementStats' own if / else-if / else over every proposal, returned or not: replicas to add or
 * to remove (old brokers that are not new brokers) -> one inter-broker movement and num_to_add * size MB; else replicas
 * between disks -> num_between_disks intra-broker movements and num_between_disks * size MB; else one leadership
 * movement. Sums are int64.
 * The reference's ExecutionProposal constructor throws for a proposal with both additions and between-disk moves
 * (ExecutionProposal.java:81-84). Here such a proposal counts as inter-broker, as the if / else does, and no error is
 * raised; the host path (ccmi_proposals and the binding's movement statistics) does the same. No goal chain of the test
 * fixtures reaches it: a chain is broker- or disk-granularity, never both.
 * The session is not changed. Valid on a fresh session (0 records, a zero summary), after any optimization and after
 * ccmi_session_apply with nothing in between (the pending rows, slot orders and leaders are sent first). On a model
 * with disks the call sends the current disk of every replica slot (4 bytes each) along; the other inputs are resident.
 * The launches count into stats_launches, stats_bytes and stats_kernel_ms of ccmi_perf_counters, as ccmi_broker_stats.
 * Errors, all before any launch: CCMI_E_INVALID for a NULL s, a NULL num_records, capacity < 0, or NULL records with
 * capacity > 0 on a model with P > 0. CCMI_E_DEVICE for a device failure; on error the outputs are unspecified. */
ccmi_status ccmi_proposal_diff(ccmi_session* s, ccmi_proposal_record* records /* [capacity] */, int64_t capacity,
                               int64_t* num_records, ccmi_proposal_summary* summary /* optional */);

/* ReplicaSortFunctionFactory's selection functions (ReplicaSortFunctionFactory.java:29-40) and the two priority
 * functions the inter-broker goals use (:21-23). */
enum { CCMI_SEL_LEADERS = 1, CCMI_SEL_FOLLOWERS = 2, CCMI_SEL_ONLINE = 4, CCMI_SEL_OFFLINE = 8,
       CCMI_SEL_IMMIGRANTS = 16, CCMI_SEL_IMMIGRANT_OR_OFFLINE = 32 };      /* ReplicaSortFunctionFactory selections */
enum { CCMI_PRIO_OFFLINE = 0, CCMI_PRIO_IMMIGRANTS = 1 };                  /* prioritizeOfflineReplicas / prioritizeImmigrants */
/* What a SortedReplicas is built from (SortedReplicas.java:57-96, SortedReplicasHelper). 64 bytes. */
typedef struct ccmi_sorted_replicas_query {
  int32_t select_mask;        /* OR of CCMI_SEL_*: every named selection must hold */
  int32_t num_priorities;     /* 0..2 */
  int32_t priorities[2];      /* CCMI_PRIO_* in application order (SortedReplicas._priorityFuncs); unused = -1 */
  int32_t score_resource;     /* ccmi_resource, or -1 = no score function */
  int32_t score_reverse;      /* 0 sortByMetricGroupValue, 1 reverseSortByMetricGroupValue */
  int32_t above_resource;     /* selectReplicasAboveLimit resource, -1 = none */
  int32_t below_resource;     /* selectReplicasBelowLimit resource, -1 = none */
  double  above_limit, below_limit;
  const uint8_t* topic_excluded;  /* [T] or NULL: selectReplicasBasedOnExcludedTopics */
  const uint8_t* topic_included;  /* [T] or NULL: selectReplicasBasedOnIncludedTopics */
} ccmi_sorted_replicas_query;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). The sorted replicas of brokers on the session's
 * current model, selected, keyed and sorted on the device from the resident tables: segment i, records[offsets[i],
 * offsets[i + 1]), is what new SortedReplicas(broker brokers[i], selections, priorities, score).sortedReplicas(false)
 * (SortedReplicas.java:57-62, :106-114) would iterate if it were initialised now (ensureInitialize, :168-177: every replica
 * of the broker that all selection functions accept). brokers == NULL asks for brokers 0..n-1 and needs n == B. Each
 * record is {partition index, broker index}: a ccmi_swap_replica, usable as it stands as a source or candidate of
 * ccmi_swaps_acceptance_grid and, with an action type, as a ccmi_move_source of ccmi_moves_acceptance_mask.
 * Order: the comparator of SortedReplicas.java:75-90. First the priority functions in list order (comparePriority,
 * :179-192), priorities[0] before priorities[1]: CCMI_PRIO_OFFLINE puts isCurrentOffline() replicas first, CCMI_PRIO_IMMIGRANTS
 * replicas with originalBroker() != broker() (ReplicaSortFunctionFactory.java:21-23); either order of the two is honoured.
 * Then, with score_resource >= 0, Double.compare of the score: (double) load().loadByWindows().valuesForGroup(the
 * resource's metric group).avg() (ReplicaSortFunctionFactory.java:51-58; CPU: [CPU], DISK: [DISK], NW_IN: [LEADER_BYTES_IN,
 * REPLICATION_BYTES_IN] added window by window in float, NW_OUT: [LEADER_BYTES_OUT, REPLICATION_BYTES_OUT]; avg() =
 * (float)(sum / W)), negated for score_reverse (:65-72). Double.compare puts -0.0 below 0.0, and a reversed zero is -0.0; an
 * empty load scores 0. Last Replica.compareTo (Replica.java:350-377): isCurrentOffline() replicas first, then the partition
 * number, then the original broker's id, then the topic name (String.compareTo). The session ranks the topic names itself;
 * the caller passes nothing for it. No two replicas compare equal, so the order is total. NaN loads are outside the
 * contract. scores (optional, [capacity]): scores[k] is the score of records[k] exactly as compared, 0.0 without a score
 * function.
 * Selections (all must hold): CCMI_SEL_LEADERS isLeader(), CCMI_SEL_FOLLOWERS !isLeader(), CCMI_SEL_ONLINE
 * !isCurrentOffline(), CCMI_SEL_OFFLINE isCurrentOffline(), CCMI_SEL_IMMIGRANTS originalBroker() != broker(),
 * CCMI_SEL_IMMIGRANT_OR_OFFLINE either (ReplicaSortFunctionFactory.java:29-40); topic_excluded keeps a replica when
 * isOriginalOffline() || !topic_excluded[topic] (:144-146: an original-offline replica passes whatever its topic);
 * topic_included keeps it when topic_included[topic] != 0 (:153-155); above_resource / below_resource keep it when
 * load().expectedUtilizationFor(resource) > above_limit / < below_limit, both strict (:163-175). Per-disk sorted replicas
 * and prioritizeDiskImmigrants (the intra-broker goals) are out of scope.
 * offsets[0..n] are always written in full and *num_records = offsets[n]. records and scores are written only when
 * offsets[n] <= capacity; otherwise neither is touched and the status is still CCMI_OK, so capacity == 0 with NULL records
 * is the sizing call (NULL records when there are records and they fit is CCMI_E_INVALID, found after the offsets are
 * written). A broker with no replica, or none selected, is a zero-length segment; n == 0 is CCMI_OK.
 * The session is not changed: tracked sorted replicas, the snapshot caches, the broker versions, the action log and the
 * proposals stay as they are. Valid on a fresh session, after any optimization and after ccmi_session_apply with nothing
 * in between (the pending rows, Java loads, slot orders and leaders are sent first). A sharded session answers locally.
 * The launches count into stats_launches, stats_bytes and stats_kernel_ms of ccmi_perf_counters, as ccmi_broker_stats; no
 * acceptance counter counts them.
 * Errors, all before any launch: CCMI_E_INVALID for a NULL s, q, offsets or num_records, capacity < 0, unknown bits in
 * select_mask, num_priorities outside 0..2, a priority value other than 0 or 1, a priority named twice, a resource
 * outside [-1, 4), score_reverse not 0 or 1, brokers == NULL with n != B, and, with *first_invalid (when given) set to
 * its position, a broker out of range or listed twice; *first_invalid is -1 for every other error and on success.
 * CCMI_E_DEVICE for a device failure. On error the outputs are unspecified. */
ccmi_status ccmi_sorted_replicas(ccmi_session* s, const ccmi_sorted_replicas_query* q,
                                 const int32_t* brokers /* [n] broker indices, or NULL = brokers 0..n-1 with n == B */,
                                 int64_t n, int64_t* offsets /* [n + 1] */,
                                 ccmi_swap_replica* records /* [capacity] */, double* scores /* [capacity] or NULL */,
                                 int64_t capacity, int64_t* num_records, int64_t* first_invalid /* optional */);

/* The ReplicaMovementStrategy classes of executor/strategy/ and the per-partition state their comparators read. */
enum { CCMI_STRATEGY_BASE = 0,                /* BaseReplicaMovementStrategy: the execution id */
       CCMI_STRATEGY_PRIORITIZE_LARGE = 1,    /* PrioritizeLargeReplicaMovementStrategy: dataToMoveInMB descending */
       CCMI_STRATEGY_PRIORITIZE_SMALL = 2,    /* PrioritizeSmallReplicaMovementStrategy: dataToMoveInMB ascending */
       CCMI_STRATEGY_POSTPONE_URP = 3,        /* PostponeUrpReplicaMovementStrategy */
       CCMI_STRATEGY_PRIORITIZE_MIN_ISR_WITH_OFFLINE = 4,           /* PrioritizeMinIsrWithOfflineReplicasStrategy */
       CCMI_STRATEGY_PRIORITIZE_ONE_ABOVE_MIN_ISR_WITH_OFFLINE = 5, /* PrioritizeOneAboveMinIsrWithOfflineReplicasStrategy */
       CCMI_NUM_STRATEGIES = 6 };
enum { CCMI_PSTATE_UNDER_REPLICATED = 1,      /* ExecutionUtils.isPartitionUnderReplicated */
       CCMI_PSTATE_UNDER_MIN_ISR = 2,         /* in populateMinIsrState's underMinIsr set (with offline replicas) */
       CCMI_PSTATE_AT_MIN_ISR = 4,            /* in its atMinIsr set */
       CCMI_PSTATE_ONE_ABOVE_MIN_ISR = 8 };   /* in its oneAboveMinIsr set */
/* What the caller of ExecutionTaskPlanner.addExecutionProposals brings besides the proposals. 64 bytes. */
typedef struct ccmi_execution_plan_query {
  int32_t num_strategies;         /* 0..4 */
  int32_t strategies[4];          /* CCMI_STRATEGY_* in application order (ReplicaMovementStrategy.chain); unused = -1 */
  int32_t reserved[7];            /* 0 */
  const int32_t* proposal_rank;   /* [P] or NULL: the position of a partition's proposal in the caller's collection */
  const uint8_t* partition_state; /* [P] or NULL: OR of CCMI_PSTATE_* per partition; NULL = no flag set */
} ccmi_execution_plan_query;
/* One inter-broker ExecutionTask; its execution id is its position in the task table. 16 bytes. */
typedef struct ccmi_plan_task {
  int32_t partition;        /* partition index (desc order) */
  int32_t num_to_add;       /* |replicasToAdd|: the task's destination brokers */
  int64_t data_to_move_mb;  /* ExecutionProposal.dataToMoveInMB (:242-244): (num_to_add + num_between_disks) * size */
} ccmi_plan_task;
/* 64 bytes. */
typedef struct ccmi_plan_summary {
  int64_t num_inter_tasks;         /* inter-broker tasks created, before maybeDropReplicaSwapTasks */
  int64_t num_inter_entries;       /* entries of inter_entries: inter_offsets[B]; 0 after the drop */
  int64_t num_intra_tasks;         /* intra-broker tasks created: entries of intra_entries, intra_offsets[B], unless mingled */
  int64_t num_leader_tasks;        /* leadership tasks created: entries of leader_tasks unless mingled */
  int64_t num_brokers_with_tasks;  /* brokers with a non-empty inter-broker list: the valid prefix of broker_order */
  int64_t size_overflow;           /* 1: some inter-broker task's data_to_move_mb exceeds INT32_MAX (see below) */
  int64_t mingled;                 /* 1: the reference throws IllegalStateException (see below); every list is empty */
  int64_t reserved;                /* 0 */
} ccmi_plan_summary;
/* Additive at ABI v13 (the capability flag is the presence of the symbol). What ExecutionTaskPlanner.addExecutionProposals
 * (executor/ExecutionTaskPlanner.java:137-273) builds from the proposals ccmi_proposal_diff would return now, computed on
 * the device from the resident tables: the tasks, their execution ids, the per-broker task sets in strategy order and the
 * first round's broker order (brokerComparator, :518-539).
 * Assumption: the live Kafka cluster still has the session's initial placement, leaders and logdirs, and every replica is
 * in sync: the state in which a freshly computed proposal set reaches the executor. The planner's three cluster reads are
 * answered from it: isInterBrokerMovementCompleted (ExecutionProposal.java:120-122) is "new_replicas equals old_replicas
 * as a broker sequence", the current logdir of a replica is its old disk, and the current leader is old_leader.
 * Inter-broker tasks: a proposal whose new_replicas differs from old_replicas as a broker sequence. So a leadership-only
 * proposal has one (data_to_move_mb 0, no destination), a disk-only proposal none.
 * Execution ids follow the iteration order of the caller's Collection<ExecutionProposal>, which the device does not hold:
 * tasks are numbered in ascending (proposal_rank[p], partition index), a total order whatever the array holds;
 * proposal_rank == NULL is the partition index. Inter-broker tasks get ids 0..num_inter_tasks-1 (they are created first,
 * :141); tasks[id] describes task id. The ids of intra-broker and leadership tasks are not reported: within a proposal
 * they follow a HashMap's order and no output order depends on them.
 * Inter-broker lists: task t is filed under old_leader (the reference files it under the old leader only, not under every
 * broker that loses a replica: AbstractReplicaMovementStrategy.java:69) and under every broker of replicasToAdd (:76).
 * Segment b, inter_entries[inter_offsets[b], inter_offsets[b + 1]), holds the execution ids of broker b's TreeSet in
 * iteration order under the chain q->strategies; BaseReplicaMovementStrategy is appended when the chain lacks it
 * (chainBaseReplicaMovementStrategyIfAbsent), so the order is total, and a strategy named after BASE never decides.
 *   BASE: the execution id. PRIORITIZE_LARGE / PRIORITIZE_SMALL: data_to_move_mb descending / ascending.
 *   POSTPONE_URP: a partition without CCMI_PSTATE_UNDER_REPLICATED first.
 *   PRIORITIZE_MIN_ISR_WITH_OFFLINE: CCMI_PSTATE_UNDER_MIN_ISR first, then CCMI_PSTATE_AT_MIN_ISR without it, then the rest.
 *   PRIORITIZE_ONE_ABOVE_MIN_ISR_WITH_OFFLINE: CCMI_PSTATE_ONE_ABOVE_MIN_ISR first.
 * The session does not hold the live ISR state; the caller evaluates it once per partition into partition_state. Naming
 * one of the three with partition_state == NULL is allowed: it never decides. A partition missing from the cluster
 * metadata is outside the contract.
 * Size overflow: the Java size comparators are (int)(d2 - d1) on longs, a consistent order exactly when every
 * data_to_move_mb fits int32. The device always orders by the int64 value and sets size_overflow when some inter-broker
 * task's value exceeds INT32_MAX; the caller decides what to do then.
 * broker_order[0, num_brokers_with_tasks) lists the brokers with a non-empty inter-broker list in brokerComparator's
 * initial order: the chain applied to each broker's first task, then the longer list, then the smaller broker index
 * (index order is id order); the rest of broker_order[B] is -1.
 * Intra-broker tasks: one per (proposal, broker) of replicasToMoveBetweenDisksByBroker. Segment b of intra_entries holds
 * the partition indices of broker b's tasks in execution order (ExecutionTask.compareTo), which is proposal order: a
 * proposal has at most one such task per broker.
 * Leadership tasks: a proposal with hasLeaderAction whose old_leader is not new_replicas[0] by broker (:262-264; a leader
 * that only changed disk gets none). leader_tasks holds their partition indices in proposal order.
 * Drop and throw: when any intra-broker task exists the inter-broker lists, tasks and broker_order are empty
 * (maybeDropReplicaSwapTasks, :168-173); num_inter_tasks keeps the count before the drop. If in that case some
 * inter-broker task has num_to_add > 0 the reference throws IllegalStateException (sanityCheckExecutionTasks, :152-160):
 * mingled = 1, every list is empty (the intra-broker and leadership ones too) and the status is CCMI_OK.
 * Round selection (getInterBrokerReplicaMovementTasks, :348-439) is serial and depends on live concurrency state: it
 * stays with the caller, over these lists.
 * Capacities: summary, inter_offsets[B + 1] and intra_offsets[B + 1] are always written. tasks, inter_entries,
 * broker_order, intra_entries and leader_tasks are written only when every one of them fits: the tasks that survive the
 * drop <= task_capacity, num_inter_entries <= inter_capacity, num_intra_tasks <= intra_capacity and num_leader_tasks <=
 * leader_capacity; otherwise none is touched and the status is still CCMI_OK. All capacities 0 with NULL arrays is the
 * sizing call.
 * The session is not changed. Valid on a fresh session (empty lists, a zero summary), after any optimization and after
 * ccmi_session_apply with nothing in between (the pending rows, slot orders and leaders are sent first; a model with disks
 * sends its current disks along, as ccmi_proposal_diff). A sharded session answers locally. The launches count into
 * stats_launches, stats_bytes and stats_kernel_ms of ccmi_perf_counters, as ccmi_broker_stats.
 * Errors, all before any launch: CCMI_E_INVALID for a NULL s, q, summary, inter_offsets or intra_offsets, a negative
 * capacity, num_strategies outside 0..4, an unknown strategy or one named twice, an array that is NULL with a capacity
 * above 0 (its data could fit), and a NULL broker_order with inter_capacity > 0. CCMI_E_DEVICE for a device failure; on
 * error the outputs are unspecified. */
ccmi_status ccmi_execution_plan(ccmi_session* s, const ccmi_execution_plan_query* q, ccmi_plan_summary* summary,
                                ccmi_plan_task* tasks /* [task_capacity] */, int64_t task_capacity,
                                int64_t* inter_offsets /* [B + 1] */, int32_t* inter_entries /* [inter_capacity] */,
                                int64_t inter_capacity, int32_t* broker_order /* [B] */,
                                int64_t* intra_offsets /* [B + 1] */, int32_t* intra_entries /* [intra_capacity] */,
                                int64_t intra_capacity, int32_t* leader_tasks /* [leader_capacity] */,
                                int64_t leader_capacity);

/*
 * ccmi_aggregator_*, additive at ABI v13: the capability flag is the presence of the symbols, ccmi_perf_counters keeps
 * its layout. MetricSampleAggregator on the device: the step of LoadMonitor.clusterModel that turns metric samples into
 * the per-window floats ccmi_builder_populate_partition takes as leader_metrics. A literal restatement of
 * cruise-control-core monitor/sampling/aggregator/{MetricSampleAggregator, RawMetricValues, WindowState,
 * MetricSampleAggregatorState.computeCompleteness, MetricSampleCompleteness, AggregationOptions, Extrapolation}.java and
 * common/WindowIndexedArrays.java. An aggregator owns its buffers and its stream on one device and needs no session;
 * it is single-threaded, several may live on one device.
 *
 * Entities are the dense ids 0..E-1 with entity_group[e] in 0..G-1 (for partitions the topic; the ids of a group need
 * not be contiguous). Metrics are 0..M-1, each with a ccmi_aggregation_function. An entity is "present" (a key of
 * _rawMetrics) from its first accepted sample until ccmi_aggregator_remove_entities or ccmi_aggregator_clear.
 *
 * ccmi_aggregator_add_samples has the effect of MetricSampleAggregator.addSample on the n samples in batch order:
 * windowIndex = time / window_ms + 1, a sample older than the oldest window is dropped (accepted[i] = 0),
 * maybeRollOutNewWindow (leaps larger than the windows kept and several roll-outs inside one batch included), the
 * updateOldestWindowIndex of a new RawMetricValues, counts and values by add / max / latest with their (float) of a
 * double expression, the _validity and _extrapolations bits by the reference's state machine, and the generation
 * (newWindowsRolledOut || windowIndex != _currentWindowIndex). Two samples of one entity take effect in batch order.
 * _counts is a Java byte: more than 127 samples in one window of one entity is outside the contract (the count then
 * differs from the reference's wrapped byte), as is min_samples_per_window outside 1..127. A negative sample time is
 * refused (CCMI_E_INVALID) before anything changes, and num_windows is at most 31 (one validity bit per kept window).
 *
 * ccmi_aggregator_completeness: MetricSampleAggregator.completeness. `interested` is a byte mask over the E entities;
 * NULL, or a mask selecting nothing, means every present entity (interpretAggregationOptions on an empty set). The
 * windows of the clamped range are walked newest to oldest through WindowState.maybeInclude; per walked window the four
 * ratios of fillInValidRatios and whether it was included, newest first, in the arrays the caller hangs into the
 * struct (window_capacity of each; num_windows + 1 always suffices; CCMI_E_INVALID when too small). A ratio over no
 * interested entity is Java's canonical NaN. The reference caches window states by generation and completeness by
 * options; this always computes from the current bits, which is the reference's answer whenever its caches are current.
 *
 * ccmi_aggregator_aggregate: completeness, validateCompleteness, then RawMetricValues.aggregate over the valid windows,
 * newest first, for include_invalid_entities ? the interested entities : the valid ones, in ascending id order, cut to
 * `capacity`; *num_entities is always the full count, so capacity = 0 is the sizing call and rows beyond the count stay
 * untouched. values is [k][M][Wv] and extrapolations [k][Wv] with Wv = out->num_valid_windows; an entity that is not
 * present gets zeros and CCMI_EXTRAPOLATION_NO_VALID in every window and is invalid, a present one is invalid iff
 * !isValid(max_allowed_extrapolations_per_entity). NotEnoughValidWindowsException is an expected outcome: CCMI_OK with
 * out->failure set, *num_entities = 0 and no row written. The two coverage IllegalStateExceptions are CCMI_E_STATE with
 * the reference's message text (its options suffix left out) in ccmi_last_error; they are restated for completeness
 * and not reachable, since a window is included only if the merged ratios meet both minima and the final ratios are
 * those of the last included window.
 *
 * ccmi_aggregator_peek_current_window: peekCurrentWindow, one window (the aggregator's current one, no range check)
 * for every present entity, ascending ids, values [k][M], the same capacity convention.
 * ccmi_aggregator_remove_entities: removeEntities (the generation advances once if any was present).
 * ccmi_aggregator_clear: clear (the window indices stay, as in the reference).
 *
 * Errors: CCMI_E_INVALID for a NULL argument that is not marked nullable, num_windows < 1 or > 31, window_ms < 1,
 * min_samples_per_window outside 1..127, M < 1, E < 1, G < 1, a group or function id out of range, n < 0, an entity id
 * out of range, a negative sample time, min_valid_windows < 1, a granularity outside the enum, capacity < 0;
 * CCMI_E_DEVICE for a device failure. On error the outputs are unspecified.
 */
typedef enum ccmi_aggregation_function { CCMI_AGG_AVG = 0, CCMI_AGG_MAX = 1, CCMI_AGG_LATEST = 2 } ccmi_aggregation_function;
typedef enum ccmi_extrapolation {
  CCMI_EXTRAPOLATION_NONE = 0,
  CCMI_EXTRAPOLATION_AVG_AVAILABLE = 1,
  CCMI_EXTRAPOLATION_AVG_ADJACENT = 2,
  CCMI_EXTRAPOLATION_FORCED_INSUFFICIENT = 3,
  CCMI_EXTRAPOLATION_NO_VALID = 4
} ccmi_extrapolation;
typedef enum ccmi_granularity { CCMI_GRANULARITY_ENTITY = 0, CCMI_GRANULARITY_ENTITY_GROUP = 1 } ccmi_granularity;
typedef enum ccmi_aggregation_failure {
  CCMI_AGG_FAILURE_NONE = 0,
  CCMI_AGG_FAILURE_NO_WINDOW_IN_RANGE = 1,         /* "There is no window available in range ..." */
  CCMI_AGG_FAILURE_NOT_ENOUGH_VALID_WINDOWS = 2    /* "There are only %d valid windows ..." */
} ccmi_aggregation_failure;

typedef struct ccmi_aggregator ccmi_aggregator;
typedef struct ccmi_aggregator_config {
  int64_t window_ms;
  int32_t num_windows, min_samples_per_window, num_metrics, num_entities, num_groups, reserved;
} ccmi_aggregator_config;
typedef struct ccmi_aggregator_state {
  int64_t generation, oldest_window_index, current_window_index, num_samples, num_present_entities;
  int32_t num_available_windows, reserved;
} ccmi_aggregator_state;
typedef struct ccmi_aggregation_options {
  double min_valid_entity_ratio, min_valid_entity_group_ratio;
  int32_t min_valid_windows, max_allowed_extrapolations_per_entity, granularity, include_invalid_entities;
} ccmi_aggregation_options;
typedef struct ccmi_aggregator_completeness {
  int64_t generation;
  int32_t num_windows, num_valid_windows, failure, window_capacity;
  int32_t num_interested_entities, num_interested_groups, num_valid_entities, num_valid_groups;
  float valid_entity_ratio, valid_entity_group_ratio;
  int64_t* window_index;                                  /* [window_capacity] the walked windows, newest first */
  uint8_t* window_included;                               /* [window_capacity] 1 = a valid window index */
  float* valid_entity_ratio_by_window;                    /* [window_capacity] */
  float* valid_entity_ratio_with_group_granularity_by_window;
  float* valid_entity_group_ratio_by_window;
  float* extrapolated_entity_ratio_by_window;
} ccmi_aggregator_completeness;

ccmi_status ccmi_aggregator_create(int32_t device_ordinal, const ccmi_aggregator_config* config,
                                   const uint8_t* metric_function /* [M] */, const int32_t* entity_group /* [E] */,
                                   ccmi_aggregator** out);
void ccmi_aggregator_destroy(ccmi_aggregator* a);
ccmi_status ccmi_aggregator_add_samples(ccmi_aggregator* a, const int32_t* entity /* [n] */,
                                        const int64_t* time_ms /* [n] */, const double* values /* [n][M] */, int64_t n,
                                        uint8_t* accepted /* nullable [n] */, int64_t* num_accepted /* nullable */);
ccmi_status ccmi_aggregator_state_query(ccmi_aggregator* a, ccmi_aggregator_state* out);
ccmi_status ccmi_aggregator_completeness_query(ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
                                               const ccmi_aggregation_options* options,
                                               const uint8_t* interested /* nullable [E] */,
                                               ccmi_aggregator_completeness* out, uint8_t* valid_entities /* nullable [E] */,
                                               uint8_t* valid_groups /* nullable [G] */);
ccmi_status ccmi_aggregator_aggregate(ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
                                      const ccmi_aggregation_options* options, const uint8_t* interested /* nullable [E] */,
                                      ccmi_aggregator_completeness* out, int32_t* entities /* [capacity] */,
                                      float* values /* [capacity][M][Wv] */, uint8_t* extrapolations /* [capacity][Wv] */,
                                      uint8_t* invalid /* [capacity] */, int64_t capacity, int64_t* num_entities);
ccmi_status ccmi_aggregator_peek_current_window(ccmi_aggregator* a, int32_t* entities /* [capacity] */,
                                                float* values /* [capacity][M] */, uint8_t* extrapolations /* [capacity] */,
                                                int64_t capacity, int64_t* num_entities);
ccmi_status ccmi_aggregator_remove_entities(ccmi_aggregator* a, const int32_t* entities /* [n] */, int64_t n);
ccmi_status ccmi_aggregator_clear(ccmi_aggregator* a);

/*
 * ccmi_builder_populate_from_aggregator, additive at ABI v13: the capability flag is the presence of the symbol. The
 * seam between the two halves of LoadMonitor.clusterModel (monitor/LoadMonitor.java:491-543) in one call: the
 * aggregate of `a` over [from_ms, to_ms] with `options` and `interested`, and MonitorUtils.populatePartitionLoad
 * (monitor/MonitorUtils.java:415-479) for every row of it. The rows never leave the device on the way: the validity
 * checks, the compaction of the partitions that are populated and the replica loads run there (K18), the finished
 * columns come back in one copy and are appended to the builder.
 *
 * Entity e of the aggregator is partition e of `topology` (Cluster.partition(tp)); metric_of[m] is the aggregator's
 * metric index of ccmi_metric m ({0, 1, 2, 3, 7, 8} for KafkaMetricDef's common metrics).
 *
 * Contract: the builder ends in exactly the state it would reach from ccmi_aggregator_aggregate (same range, options
 * and mask, with capacity for every row) followed by one ccmi_builder_populate_partition per returned row in ascending
 * entity order. Every returned row is populated, the zero rows of absent entities under include_invalid_entities
 * included. A partition with an empty replica range (partitionInfo == null, its topic was deleted) is left out. An
 * offline partition (leader_broker_id < 0) is checked for unknown and duplicate brokers and then skipped. A second
 * call appends; topics keep first-appearance order across calls. `out` is filled as ccmi_aggregator_aggregate fills
 * it; NotEnoughValidWindows, or no window in range, is CCMI_OK with out->failure set and nothing populated.
 * *num_rows is the number of rows of the aggregate, *num_populated the partitions added to the builder.
 *
 * Errors, CCMI_E_INVALID with the text in ccmi_last_error: a NULL argument that is not marked nullable; num_partitions
 * other than the aggregator's E; a metric_of entry, topic index or logdir index out of range; a replica_offset that
 * does not start at 0 or decreases; more than 8 replicas in one partition; out->num_valid_windows other than the
 * builder's W; and the three complaints of ccmi_builder_populate_partition in its words (a replica on an unknown
 * broker, a duplicate replica broker, a leader that is not one of the replica brokers). Those three are raised only
 * for partitions that are rows of the aggregate, and for the lowest such entity id. On any error the builder is
 * unchanged. That is stricter than the per-row loop, which keeps the partitions it populated before the bad one.
 * CCMI_E_DEVICE for a device failure.
 */
typedef struct ccmi_partition_topology {      /* Cluster.partition(tp) for entity e = partition e of the aggregator */
  int32_t num_partitions, num_topics, num_logdirs, reserved;
  const char* const* topic_names;             /* [num_topics] */
  const int32_t* partition_topic;             /* [P] index into topic_names */
  const int32_t* partition_number;            /* [P] */
  const int32_t* replica_offset;              /* [P + 1]; an empty range = partitionInfo == null (topic deleted): skipped */
  const int32_t* replica_broker_id;           /* [R] Kafka ids in PartitionInfo.replicas() order */
  const int32_t* leader_broker_id;            /* [P]; -1 = offline partition */
  const uint8_t* replica_offline;             /* nullable [R] */
  const int32_t* replica_logdir;              /* nullable [R] index into logdir_names, -1 = none */
  const char* const* logdir_names;            /* nullable [num_logdirs] */
} ccmi_partition_topology;

ccmi_status ccmi_builder_populate_from_aggregator(
    ccmi_model_builder* b, ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
    const ccmi_aggregation_options* options, const uint8_t* interested /* nullable [E] */,
    const int32_t metric_of[6] /* aggregator metric index of each ccmi_metric, e.g. {0,1,2,3,7,8} */,
    const ccmi_partition_topology* topology, ccmi_aggregator_completeness* out,
    int64_t* num_rows /* rows of the aggregate */, int64_t* num_populated /* partitions added to the builder */);

/*
 * ccmi_aggregator_metric_anomalies and ccmi_slow_broker_finder_*, additive at ABI v13: the capability flag is the
 * presence of the symbols. The two MetricAnomalyFinders that MetricAnomalyDetector.run
 * (detector/MetricAnomalyDetector.java:69-75) hands a broker aggregator's history and current window to, over an
 * existing ccmi_aggregator whose entities are brokers, groups hosts (BrokerEntity.group()) and metrics the caller's
 * broker metric ids. Both calls take (from_ms, to_ms, options, interested) as ccmi_aggregator_aggregate does and
 * compute two row sets on the device (K19) that never come to the host:
 *   history = the rows of that aggregate. KafkaBrokerMetricSampleAggregator.aggregate uses ratios 0.0 / 0.0,
 *             min_valid_windows 1, granularity ENTITY, include_invalid_entities false, from -1, to now.
 *             NotEnoughValidWindows, or no window in range, is the reference's empty map: out->failure is set, there
 *             are no history rows, and the finder still runs.
 *   current = the rows of peekCurrentWindow: every present entity, the aggregator's current window, no interest mask.
 * An entity "has history" iff it is a row of the aggregate. History values are newest first, latest() is value 0 of
 * the current row (a Java float: the one sum of two latest() values, the current bytes in rate of the slow broker
 * finder, is a float sum widened afterwards); every other float is widened to double before any arithmetic
 * (MetricValues.doubleArray, and the double variables latest() is assigned to). The percentile
 * is commons-math3 3.6.1's Percentile with its defaults (LEGACY estimation, NaNStrategy.REMOVED), results bit for
 * bit up to the sign of a zero; isDataSufficient is PercentileMetricAnomalyFinderUtils.java:28-35. `out` is filled
 * as ccmi_aggregator_aggregate fills it. Neither call changes the aggregator. No exception of the reference is
 * reachable on these inputs: the finders' null checks guard maps that always exist here, and a percentile of 0 or
 * 100 (where Percentile.evaluate would throw for 0) makes isDataSufficient false before evaluate is reached.
 *
 * ccmi_aggregator_metric_anomalies: PercentileMetricAnomalyFinder.metricAnomalies (:140-177) with getAnomalyForMetric
 * (:64-93). With no history row, or !isDataSufficient(Wv, upper, lower) for the aggregate's Wv valid windows, there is
 * no anomaly. Otherwise, for every current entity that has history and every metric m with interested_metrics[m]:
 * u = percentile(history, upper); u <= 1 (SIGNIFICANT_METRIC_VALUE_THRESHOLD) is no anomaly; else upper_threshold =
 * u * (1 + upper_margin), lower_threshold = percentile(history, lower) * lower_margin, current = latest, an anomaly iff
 * current > upper_threshold || current < lower_threshold. The records come in ascending (entity, metric) order.
 * *num_anomalies is always the full count (numAnomaliesOfType(RECENT)); capacity 0 with anomalies NULL is the sizing
 * call; records beyond min(capacity, count) are untouched. *current_window_index is the window of the current rows.
 * The description string and the KafkaMetricAnomaly object stay with the caller: the record carries every number the
 * string formats, `out` the history windows.
 * Errors, CCMI_E_INVALID: a NULL argument that is not marked nullable, capacity < 0, malformed options, a percentile
 * outside [0.01, 99.99], upper_margin outside [0, 10], lower_margin outside [0, 1] (the ConfigDef ranges).
 *
 * ccmi_slow_broker_finder: SlowBrokerFinder with its state, bound to one aggregator (which must outlive it); score[E]
 * and since_ms[E] (_brokerSlownessScore, _detectedSlowBrokers) live on the device. One detect is one
 * metricAnomalies (:340-353) at _kafkaCruiseControl.timeMs() == time_ms:
 *   1. per current entity: bytes = latest(leader_bytes_in) + latest(replication_bytes_in); skipped iff bytes <
 *      bytes_in_rate_detection_threshold; else flush = latest(log_flush), per_byte = flush / bytes, and with history
 *      the flush history keeps the values > 5.0, the per-byte history flush[i] / (in[i] + repl[i]) where that sum >=
 *      the threshold;
 *   2. getMetricAnomalies for each of the two metrics, the union of: from history, for an entity with history and
 *      isDataSufficient(kept, hp, hp), cur > percentile(kept, hp) * history margin; from peers, if
 *      isDataSufficient(active, pp, pp), cur > percentile(all active current values, pp) * peer margin (also with
 *      no history at all);
 *   3. suspects = both sets and flush > log_flush_time_threshold_ms;
 *   4. updateBrokerSlownessScore (:360-386) for every entity, current or not: a suspect gets since = time_ms if it had
 *      none and score = (none ? 1 : min(score + 1, decommission)); a scored non-suspect gets --score and leaves both
 *      maps at 0;
 *   5. createSlowBrokerAnomalies (:388-422): a suspect with score == decommission is "remove", else with score >=
 *      demotion "demote"; PERSISTENT = removes, RECENT = demotes, SUSPECT = |since map| - both; unfixable iff
 *      demotes + removes > cluster_size * unfixable ratio with cluster_size = the history rows.
 * The reported brokers (kind 1 demote, 2 remove, in ascending entity order) follow the capacity convention above; every
 * call is one round of the score update whatever the capacity, and E rows always suffice. When `unfixable` is set the
 * reference reports all of them in one unfixable anomaly, else the demotes as one fixable anomaly and the removes as
 * one whose fixability is removal_enabled. `diagnostics`, when given, receives one byte per entity
 * (CCMI_SLOW_DIAG_*; 0 for an entity that is not current). scores() returns the scored entities ascending (kind 0);
 * reset() forgets them.
 * Errors, CCMI_E_INVALID (the predicates of configure :434-477): a threshold < 0, a percentile outside [0, 100], a
 * margin < 1, a score < 0, a ratio outside [0, 1], a metric index outside [0, M); a NULL argument, capacity < 0,
 * malformed options. On any error the finder's scores are unchanged. CCMI_E_DEVICE for a device failure.
 */
typedef struct ccmi_metric_anomaly_config {
  double upper_percentile, lower_percentile;  /* metric.anomaly.percentile.{upper,lower}.threshold */
  double upper_margin, lower_margin;          /* metric.anomaly.{upper,lower}.margin */
} ccmi_metric_anomaly_config;
typedef struct ccmi_metric_anomaly {
  int32_t entity, metric;
  double current, upper_threshold, lower_threshold;
} ccmi_metric_anomaly;
ccmi_status ccmi_aggregator_metric_anomalies(ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
                                             const ccmi_aggregation_options* options,
                                             const uint8_t* interested /* nullable [E] */,
                                             const ccmi_metric_anomaly_config* config,
                                             const uint8_t* interested_metrics /* [M] */,
                                             ccmi_aggregator_completeness* out, int64_t* current_window_index,
                                             ccmi_metric_anomaly* anomalies /* [capacity] */, int64_t capacity,
                                             int64_t* num_anomalies);

enum { CCMI_SLOW_BROKER_DEMOTE = 1, CCMI_SLOW_BROKER_REMOVE = 2 };
enum {
  CCMI_SLOW_DIAG_SKIPPED = 1,          /* negligible traffic */
  CCMI_SLOW_DIAG_FLUSH_HISTORY = 2,    /* log flush time above its own history */
  CCMI_SLOW_DIAG_FLUSH_PEERS = 4,      /* log flush time above its peers */
  CCMI_SLOW_DIAG_PER_BYTE_HISTORY = 8, /* per-byte log flush time above its own history */
  CCMI_SLOW_DIAG_PER_BYTE_PEERS = 16,  /* per-byte log flush time above its peers */
  CCMI_SLOW_DIAG_OVER_THRESHOLD = 32,  /* log flush time above log_flush_time_threshold_ms */
  CCMI_SLOW_DIAG_SUSPECT = 64
};
typedef struct ccmi_slow_broker_finder ccmi_slow_broker_finder;
typedef struct ccmi_slow_broker_config {
  double bytes_in_rate_detection_threshold, log_flush_time_threshold_ms;
  double metric_history_percentile, metric_history_margin;
  double peer_metric_percentile, peer_metric_margin;
  double self_healing_unfixable_ratio;
  int32_t demotion_score, decommission_score;
  int32_t log_flush_metric, leader_bytes_in_metric, replication_bytes_in_metric; /* indices into the M metrics */
  int32_t removal_enabled;
} ccmi_slow_broker_config;
typedef struct ccmi_slow_broker_summary {
  int64_t current_window_index;
  double peer_base_log_flush, peer_base_per_byte; /* NaN when not evaluated */
  int32_t num_current, num_skipped, num_active;
  int32_t cluster_size;                           /* history rows */
  int32_t num_persistent, num_recent, num_suspect;
  int32_t num_to_demote, num_to_remove;
  int32_t unfixable, removal_enabled, reserved;
} ccmi_slow_broker_summary;
typedef struct ccmi_slow_broker {
  int32_t entity, kind, score, reserved;
  int64_t since_ms;
} ccmi_slow_broker;
ccmi_status ccmi_slow_broker_finder_create(ccmi_aggregator* a, const ccmi_slow_broker_config* config,
                                           ccmi_slow_broker_finder** out);
void ccmi_slow_broker_finder_destroy(ccmi_slow_broker_finder* f);
ccmi_status ccmi_slow_broker_finder_detect(ccmi_slow_broker_finder* f, int64_t from_ms, int64_t to_ms,
                                           const ccmi_aggregation_options* options,
                                           const uint8_t* interested /* nullable [E] */, int64_t time_ms,
                                           ccmi_aggregator_completeness* out, ccmi_slow_broker_summary* summary,
                                           ccmi_slow_broker* brokers /* [capacity] */, int64_t capacity,
                                           int64_t* num_brokers, uint8_t* diagnostics /* nullable [E] */);
ccmi_status ccmi_slow_broker_finder_scores(ccmi_slow_broker_finder* f, ccmi_slow_broker* scored /* [capacity] */,
                                           int64_t capacity, int64_t* num_scored);
ccmi_status ccmi_slow_broker_finder_reset(ccmi_slow_broker_finder* f);

/*
 * Destination-sharded mode (one process per GPU): every rank creates a session on its own device from the same
 * desc, runs the same goal chain, and scans only its slice [N*rank/count, N*(rank+1)/count) of every candidate
 * list. After each scan the engine calls `fn(ctx, key)`, which must replace *key by the MIN over all ranks
 * (INT64_MAX = no accepted candidate) and return 0; the result is the reference's first accepted candidate, so
 * every rank applies the same move. Swap scans and statistics run unsharded on every rank.
 * ccmi_session_attach_rccl installs the built-in RCCL combiner (one int64 MIN allreduce over xGMI per scan);
 * ccmi_rccl_unique_id produces the 128-byte id rank 0 broadcasts to the others.
 */
typedef int (*ccmi_allreduce_min_fn)(void* ctx, int64_t* key);
ccmi_status ccmi_session_set_shard(ccmi_session* s, int32_t rank, int32_t count, ccmi_allreduce_min_fn fn, void* ctx);
ccmi_status ccmi_rccl_unique_id(uint8_t out[128]);
ccmi_status ccmi_session_attach_rccl(ccmi_session* s, int32_t rank, int32_t count, const uint8_t unique_id[128]);
/* ABI v9. ccmi_session_attach_shm: the built-in combiner for ranks on one node — a MIN over one int64 per rank in a
 * POSIX shared-memory block `name` ("/name"; rank 0 creates it, the others open it, and every rank waits until all
 * `count` ranks are attached, at most 120 s). No GPU work per combine, so the session keeps its scan server. */
ccmi_status ccmi_session_attach_shm(ccmi_session* s, int32_t rank, int32_t count, const char* name);
/* ABI v12. ccmi_session_attach_shm with a job nonce: every rank passes the same nonzero `job_nonce` (e.g. rank 0's
 * start time broadcast over the job's process group); rank 0 stamps it into the block and the other ranks attach only
 * to a block carrying it, so a block a crashed run left under the same name is refused however recent (nonce 0: the
 * v9 rule, a block older than the timeout is stale). `timeout_s` bounds every wait (0 = 120 s). */
ccmi_status ccmi_session_attach_shm_job(ccmi_session* s, int32_t rank, int32_t count, const char* name,
                                        uint64_t job_nonce, double timeout_s);
/* ABI v11. Shard groups: the ranks of one sharded proposal driven from ONE process, one host thread per session
 * (typically one session per GPU of the node, each thread calling ccmi_optimizations on its own session). The ranks'
 * first-fit keys are MIN-combined in a block of pinned host memory every device maps: a scan the session's resident
 * scan server ran is combined by the server itself (its last workgroup folds the key in with system-scope atomics and
 * counts the rank in; no kernel waits for another rank), any other scan by the host thread on the same slots; whichever
 * rank arrives last (a server's workgroup or a host thread) publishes the group minimum into every rank's mailbox. A
 * destroyed session leaves its rank's slot empty and a destroyed group detaches its sessions. The queue-scan path is
 * taken only when every rank can take it (decided at each attach), so all ranks run the same scans and combines. Replaces the per-scan host MIN of GoalOptimizer's single-threaded loop with nothing on the
 * host between the ranks' scans. */
typedef struct ccmi_shard_group ccmi_shard_group;
ccmi_status ccmi_shard_group_create(int32_t count, ccmi_shard_group** out);
ccmi_status ccmi_shard_group_destroy(ccmi_shard_group* g);
ccmi_status ccmi_session_attach_group(ccmi_session* s, ccmi_shard_group* g, int32_t rank);

/* Measurement hooks used by bench.py: device time of the last optimization's scan kernels (HIP events
 * on the engine stream) and their algorithmic bytes. */
typedef struct ccmi_perf_counters {
  int64_t scan_launches;
  double scan_kernel_ms;       /* sum of HIP-event durations of the scan kernel */
  int64_t scan_bytes;          /* algorithmic bytes (DESIGN.md per-candidate figure x candidates) */
  int64_t stats_launches;
  double stats_kernel_ms;
  int64_t stats_bytes;
  int64_t host_syncs;
  int64_t scan_required;       /* candidates the scans had to evaluate: every device list up to its winner (the
                                  algorithmic work; smaller than `candidates` where the engine never sends rows that
                                  cannot be accepted, e.g. non-legit leadership rows) */
  int64_t chain_launches;      /* K7 chain launches (several decisions applied on the device per launch) */
  int64_t intra_launches;      /* K6 intra-broker launches (one per intra-broker goal, plus overflow re-runs) */
  double intra_kernel_ms;      /* HIP-event duration of the K6 intra_brokers launches */
  int64_t intra_bytes;         /* algorithmic bytes of K6 */
  int64_t cross_launches;      /* the scan_cross share of scan_launches / scan_required / scan_kernel_ms (the kernel */
  int64_t cross_required;      /* tools/pmc_summary.py prices against its own FETCH_SIZE / WRITE_SIZE counters) */
  double cross_kernel_ms;
  int64_t combines;            /* shard-combiner calls (RCCL / host MIN-allreduce of a scan's first-fit key) */
  /* ABI v6: the persistent scan server (K8): its launches (each also counts in scan_launches), the cross / pair scans
   * it served (no launch each), their candidates up to the winner, and its busy time (first workgroup seeing a
   * command to the result published, summed over commands) */
  int64_t server_launches;
  int64_t server_scans;
  int64_t server_required;
  double server_busy_ms;
  int64_t server_payload_bytes; /* command payload the host wrote into device memory for the server */
  /* ABI v8: K7 chains the running server took as commands (SOP_CHAIN: no launch, no server stop and relaunch; the
   * chain_launches above count only chains that ran as their own launch), and commands the server's idle watchdog
   * ended before it saw them (each then ran as a launch) */
  int64_t server_chains;
  int64_t server_idle_exits;
  /* ABI v9: HIP-event time from each scan-server launch to its exit, summed (with ccmi_set_kernel_timing on): the
   * residency a rocprofv3 kernel trace reports for scan_server, idle polling included */
  double server_resident_ms;
  /* ABI v10: K6's per-call sort (intra_sort, one launch per intra-broker call) timed apart from intra_brokers, whose
   * HIP-event time intra_kernel_ms now holds alone */
  int64_t intra_sort_launches;
  double intra_sort_ms;
  /* ABI v13: ccmi_actions_acceptance launches, the cells they answered on the device, and their HIP-event time (with
   * ccmi_set_kernel_timing on) */
  int64_t accept_launches;
  int64_t accept_cells;
  double accept_kernel_ms;
} ccmi_perf_counters;
ccmi_status ccmi_perf(const ccmi_session* s, ccmi_perf_counters* out);
void ccmi_perf_reset(ccmi_session* s);
/* Record HIP events around every scan/stats kernel (adds a little host overhead; off by default). */
void ccmi_set_kernel_timing(ccmi_session* s, int32_t enabled);
/* Host-prefix counters (additive at ABI v13: the capability flag is the presence of the symbol, ccmi_perf_counters
 * keeps its layout). A pair scan's first CCMI_HOST_PREFIX pairs are evaluated on the host where that is expected to
 * decide the scan; such a scan posts nothing to the device, so scan_required, server_required,
 * server_scans and host_syncs of ccmi_perf_counters keep counting device work only. ccmi_perf_reset clears these too. */
typedef struct ccmi_host_prefix_counters {
  int64_t host_scans;      /* pair scans decided on the host: a winner within the prefix, or a list no longer than it */
  int64_t host_candidates; /* candidates evaluated on the host, those of prefixes that missed included */
} ccmi_host_prefix_counters;
ccmi_status ccmi_host_prefix_perf(const ccmi_session* s, ccmi_host_prefix_counters* out);
/* The same for cross scans (additive at ABI v13 too; host_scans / host_candidates above stay pair-only). A cross scan's
 * first CCMI_HOST_PREFIX_CROSS candidates in key order (row-major: row k, column j, key k * N + j) are evaluated on
 * the host; a scan they decide posts nothing, a miss posts the whole scan. ccmi_perf_reset clears these too. */
typedef struct ccmi_host_cross_counters {
  int64_t host_cross_scans;      /* cross scans decided on the host: a winner within the prefix, or K * N within it */
  int64_t host_cross_candidates; /* candidates evaluated on the host, those of prefixes that missed included */
} ccmi_host_cross_counters;
ccmi_status ccmi_host_cross_perf(const ccmi_session* s, ccmi_host_cross_counters* out);

/*
 * ccmi_metrics_processor_*, additive at ABI v13: the capability flag is the presence of the symbols.
 * CruiseControlMetricsProcessor (monitor/sampling/CruiseControlMetricsProcessor.java with BrokerLoad, RawMetricsHolder
 * and SamplingUtils) on the device (K20): one sampling round's raw CruiseControlMetric records in, the partition and
 * broker metric samples out, as the rows ccmi_aggregator_add_samples takes. The consumer, the serde and the sample
 * stores stay with the caller.
 *
 * add_metrics appends a batch in arrival order (addMetric for each record). `type` is the RawMetricType id (0..62);
 * topic is an index into the batch's topic_names (the names as the reporter wrote them, dots already replaced), -1 for
 * a broker-scope type; partition is -1 unless the type is PARTITION_SIZE. The records stay on the device.
 *
 * process(cluster, nodes, interested, sampling_mode, out) is process(Cluster, partitions, SamplingMode):
 *   cluster : the partitions (leader_broker_id, replica ranges, topic names with their dots); entity e = partition e.
 *   nodes   : Cluster.nodes() and, per node, what the BrokerCapacityConfigResolver gives for its CPU cores (NaN:
 *             nothing). The cache of cores follows updateCachedNumCoresByBroker: filled only for a broker that sent a
 *             metric and is a node, a NaN is not cached, a cached value survives clear and a later NaN.
 *   out     : partition samples compacted in ascending partition index (partition_entity[k], partition_values[k][9] in
 *             KafkaMetricDef.commonMetricDef() id order) and broker samples in node order (broker_node[k] = index into
 *             nodes, broker_values[k][56] in brokerMetricDef() id order, broker_version[k]); both kinds close at
 *             max_metric_timestamp. num_* are the full counts, the first *_capacity rows are written.
 *             partition_skip[P] (nullable): 0 built or not interested, 1 no leader, 2 no broker load or no
 *             BROKER_CPU_UTIL, 3 no cached cores, 4 the topic has no partition size on the leader, 5 no partition size,
 *             6 a broker holder of the CPU estimate is missing (the reference throws), 7 the estimate is null, 8 the
 *             leader is not a node. broker_skip[num_nodes] (nullable): 0 built, 1 no broker load, 2 the minimum
 *             required metrics are not available, 3 a type of either version is not available.
 *             skipped_by_node[num_nodes + 1] (nullable): skipped partitions by leader, the last slot is
 *             UNRECOGNIZED_BROKER_ID (codes 1, 6 and 8). Records of a broker that is not a node take no part and are
 *             counted in num_dropped_records, so a partition led by such a broker is code 8.
 *             num_hash_fallback_brokers: nodes whose topic set or partition map would resize early or build a tree bin
 *             in the JVM; their iteration order came from the host's HashMap emulation (engine/broker_load.h).
 * The double sums of the reference (an AVG holder in arrival order, the seven ALL_TOPIC_* sums in the iteration order
 * of a HashSet<String>, diskUsage() in that of a HashMap<TopicPartition, ...>) are added in those orders.
 * After a process or a process_into, add_metrics and both process calls return CCMI_E_STATE until clear: the reference's second process would see
 * the holders the first one overwrote. clear forgets the records and max_metric_timestamp, not the cached cores.
 *
 * Errors, CCMI_E_INVALID with the text in ccmi_last_error: a NULL argument that is not marked nullable; a type above
 * 62; a topic or partition index that does not fit the type's scope (or a partition number above 262142); a negative
 * time; duplicate names in a batch's topic table; duplicate node ids; more than 262143 nodes or 4194302 topics; a
 * capacity < 0 or a NULL output array with a capacity > 0; an unknown sampling mode. CCMI_E_DEVICE for a device failure.
 * On an error of add_metrics nothing was added.
 */
typedef struct ccmi_metrics_processor ccmi_metrics_processor;
typedef struct ccmi_metrics_processor_config { /* the static CPU model's weights (ModelParameters) */
  double cpu_weight_of_leader_bytes_in_rate;   /* 0.7 */
  double cpu_weight_of_leader_bytes_out_rate;  /* 0.15 */
  double cpu_weight_of_follower_bytes_in_rate; /* 0.15 */
  int64_t reserved;
} ccmi_metrics_processor_config;
typedef struct ccmi_raw_metrics {
  int64_t n;
  int32_t num_topics, reserved;
  const char* const* topic_names; /* [num_topics] */
  const uint8_t* type;            /* [n] */
  const int32_t* broker_id;       /* [n] */
  const int64_t* time_ms;         /* [n] */
  const double* value;            /* [n] */
  const int32_t* topic;           /* [n] */
  const int32_t* partition;       /* [n] */
} ccmi_raw_metrics;
typedef struct ccmi_cluster_nodes {
  int32_t num_nodes, reserved;
  const int32_t* broker_id; /* [num_nodes] */
  const double* num_cores;  /* [num_nodes]; NaN = the resolver gave nothing */
} ccmi_cluster_nodes;
typedef enum ccmi_sampling_mode {
  CCMI_SAMPLING_ALL = 0,
  CCMI_SAMPLING_BROKER_METRICS_ONLY = 1,
  CCMI_SAMPLING_PARTITION_METRICS_ONLY = 2,
  CCMI_SAMPLING_ONGOING_EXECUTION = 3
} ccmi_sampling_mode;
typedef struct ccmi_processed_samples {
  int64_t max_metric_timestamp;
  int64_t partition_capacity, num_partition_samples;
  int32_t* partition_entity; /* [partition_capacity] */
  double* partition_values;  /* [partition_capacity][9] */
  int64_t broker_capacity, num_broker_samples;
  int32_t* broker_node;      /* [broker_capacity] */
  double* broker_values;     /* [broker_capacity][56] */
  int8_t* broker_version;    /* [broker_capacity] */
  uint8_t* partition_skip;   /* nullable [P] */
  uint8_t* broker_skip;      /* nullable [num_nodes] */
  int32_t* skipped_by_node;  /* nullable [num_nodes + 1] */
  int32_t num_skipped_brokers, num_hash_fallback_brokers;
  int64_t num_dropped_records;
} ccmi_processed_samples;
ccmi_status ccmi_metrics_processor_create(int32_t device_ordinal,
                                          const ccmi_metrics_processor_config* config /* nullable: the defaults */,
                                          ccmi_metrics_processor** out);
void ccmi_metrics_processor_destroy(ccmi_metrics_processor* p);
ccmi_status ccmi_metrics_processor_add_metrics(ccmi_metrics_processor* p, const ccmi_raw_metrics* batch);
ccmi_status ccmi_metrics_processor_process(ccmi_metrics_processor* p, const ccmi_partition_topology* cluster,
                                           const ccmi_cluster_nodes* nodes, const uint8_t* interested /* nullable [P] */,
                                           int32_t sampling_mode, ccmi_processed_samples* out);
/* process, with the rows fed to the aggregators instead of returned: both end in exactly the state that process
 * followed by ccmi_aggregator_add_samples(entity, max_metric_timestamp, values) gives them, and no row crosses to the
 * host. The partition aggregator needs E = num_partitions and M = 9, the broker aggregator E = num_nodes (entity = node
 * index) and M = 56, both on the processor's device (CCMI_E_INVALID otherwise, before anything changes). `out` gets the
 * counts and the skip tables; its row arrays and capacities are not read. KafkaPartitionMetricSampleAggregator's own
 * isValid filtering is the caller's. */
ccmi_status ccmi_metrics_processor_process_into(ccmi_metrics_processor* p, const ccmi_partition_topology* cluster,
                                                const ccmi_cluster_nodes* nodes,
                                                const uint8_t* interested /* nullable [P] */, int32_t sampling_mode,
                                                ccmi_aggregator* partition_aggregator /* nullable */,
                                                ccmi_aggregator* broker_aggregator /* nullable */,
                                                ccmi_processed_samples* out);
ccmi_status ccmi_metrics_processor_cached_num_cores(ccmi_metrics_processor* p, int32_t broker_id,
                                                    double* out /* NaN = not cached */);
ccmi_status ccmi_metrics_processor_clear(ccmi_metrics_processor* p);

#ifdef __cplusplus
}
#endif
#endif /* CCMI_H_ */
