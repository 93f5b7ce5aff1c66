// The arithmetic of CruiseControlMetricsProcessor (K20), written once for the host and the device: the value holders
// (ValueAndCount, ValueAndTime), HolderUtils.convertUnit and allowMissingBrokerMetric, the version logic of
// BrokerLoad.maybeSetBrokerRawMetrics / setNullableBrokerMetrics, the enough-metrics ratios, the static CPU model of
// ModelUtils.estimateLeaderCpuUtilPerCore, the two key hashes and the list-bin order rule of a JDK 11 HashMap. No HIP
// runtime call: tests/cpp/test_broker_load.cpp builds it with a plain host compiler. Built with -ffp-contract=off:
// every expression is the reference's IEEE double expression.
//
// HashMap order. A broker's keys are iterated bucket by bucket at the final capacity, and inside a list bin in
// insertion order, as long as no bin ever reaches 9 nodes: then every resize happened at the load-factor threshold and
// splits kept insertion order. Key number r (0-based, by first arrival) is inserted into a table of
// tableCapacity(r) buckets; it finds 8 or more earlier keys in its bucket there iff the JDK would resize early or
// build a tree bin at that insertion (binFlagged). A broker with such a key takes the host's JHashSet order instead.
// Equal-hash TopicPartitions inside a tree bin are ordered by identity hash in the JVM, which nobody can reproduce:
// such ties are broken by insertion rank.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCMI_BL_HD __host__ __device__ __forceinline__
#else
#define CCMI_BL_HD inline
#endif

namespace ccmi {
namespace bl {

constexpr int kNumRawTypes = 63;       // RawMetricType ids 0..62
constexpr int kPartitionMetrics = 9;   // KafkaMetricDef.commonMetricDef()
constexpr int kBrokerMetrics = 56;     // KafkaMetricDef.brokerMetricDef()
constexpr int kPartitionSize = 4, kBrokerCpuUtil = 5, kFollowerFetchRate = 18;
constexpr int kScopeBroker = 0, kScopeTopic = 1, kScopePartition = 2;
constexpr int kNumTopicTypes = 7;

// RawMetricType.topicMetricTypes() in enum order
CCMI_BL_HD int topicType(int i) {
  const int t[kNumTopicTypes] = {2, 3, 11, 12, 13, 14, 15};
  return t[i];
}
CCMI_BL_HD int scopeOf(int type) {
  if (type == kPartitionSize) return kScopePartition;
  if (type == 2 || type == 3 || (type >= 11 && type <= 15)) return kScopeTopic;
  return kScopeBroker;
}
CCMI_BL_HD int versionSince(int type) { return type >= 43 ? 5 : 4; }  // broker-scope types only
// HolderUtils.METRIC_TYPES_TO_SUM: topic type -> the ALL_TOPIC_* broker type its sum overwrites
CCMI_BL_HD int sumTarget(int topicTypeId) {
  switch (topicTypeId) {
    case 2: return 0;
    case 3: return 1;
    case 11: return 6;
    case 12: return 7;
    case 13: return 8;
    case 14: return 9;
    default: return 10;  // 15
  }
}
// KafkaMetricDef id (brokerMetricDef(); the first nine are commonMetricDef()) of a raw type; -1: none
CCMI_BL_HD int metricDefOf(int type) {
  switch (type) {
    case 0: case 2: return 2;    // LEADER_BYTES_IN
    case 1: case 3: return 3;    // LEADER_BYTES_OUT
    case 4: return 1;            // DISK_USAGE
    case 5: return 0;            // CPU_USAGE
    case 6: case 11: return 7;   // REPLICATION_BYTES_IN_RATE
    case 7: case 12: return 8;   // REPLICATION_BYTES_OUT_RATE
    case 8: case 13: return 4;   // PRODUCE_RATE
    case 9: case 14: return 5;   // FETCH_RATE
    case 10: case 15: return 6;  // MESSAGE_IN_RATE
    default: return type >= 16 && type < kNumRawTypes ? type - 7 : -1;
  }
}
CCMI_BL_HD double convertUnit(double v, int type) {
  switch (type) {
    case 0: case 1: case 6: case 7: case 2: case 3: case 11: case 12: return v / 1024;
    case kPartitionSize: return v / (1024 * 1024);
    default: return v;
  }
}
// HolderUtils.allowMissingBrokerMetric; followerFetchRequired: the broker leads a partition with more than one replica
CCMI_BL_HD bool allowMissing(int type, bool followerFetchRequired) {
  switch (type) {
    case kFollowerFetchRate: return !followerFetchRequired;
    case 40: case 41: case 42: case 61: case 62: case 16: case 17: return true;
    default: return false;
  }
}

// ValueAndCount (AVG, every type but PARTITION_SIZE) and ValueAndTime (LATEST, PARTITION_SIZE)
struct Holder {
  double value;
  long long time;
  int count;
};
CCMI_BL_HD void holderReset(Holder& h) {
  h.value = 0.0;
  h.time = -1;
  h.count = 0;
}
CCMI_BL_HD void holderRecord(Holder& h, bool latest, double v, long long t) {
  if (latest) {
    if (t > h.time) {
      h.value = v;
      h.time = t;
    }
  } else {
    h.value += v;
    h.count++;
  }
}
CCMI_BL_HD double holderValue(const Holder& h, bool latest) {
  return latest ? h.value : (h.count == 0 ? 0.0 : h.value / h.count);
}

// The broker holders of one BrokerLoad after prepareBrokerMetrics, unconverted.
struct Prepared {
  double value[kNumRawTypes];
  unsigned long long avail;  // bit t: _brokerMetrics.metricValue(t) != null
  double diskUsage;
  int32_t version;      // _brokerSampleDeserializationVersion
  int32_t minRequired;  // _minRequiredBrokerMetricsAvailable
  int32_t hasLoad;      // the broker sent a record
  int32_t enough;       // enoughTopicPartitionMetrics
};
CCMI_BL_HD bool available(const Prepared& p, int type) { return (p.avail >> type) & 1ull; }
CCMI_BL_HD void setValue(Prepared& p, int type, double v) {
  p.value[type] = v;
  p.avail |= 1ull << type;
}

// BrokerLoad.enoughTopicPartitionMetrics from its four counts
CCMI_BL_HD bool enoughMetrics(int missingTopics, int topics, int missingPartitions, int ledPartitions) {
  if (ledPartitions == 0) return true;
  return ((double)missingTopics / topics) <= 0.01 && (double)missingPartitions / ledPartitions <= 0.01;
}

// maybeSetBrokerRawMetrics + setNullableBrokerMetrics + _minRequiredBrokerMetricsAvailable, on a fresh BrokerLoad
CCMI_BL_HD void versionLogic(Prepared& p, bool followerFetchRequired) {
  p.version = -1;
  for (int v = 4; v <= 5; ++v) {
    bool missing = false;
    for (int t = 0; t < kNumRawTypes; ++t) {
      if (scopeOf(t) != kScopeBroker || versionSince(t) != v || available(p, t)) continue;
      if (allowMissing(t, followerFetchRequired)) setValue(p, t, 0.0);  // MISSING_BROKER_METRIC_VALUE
      else missing = true;
    }
    if (missing) break;  // the missing set is recorded while the version is -1: it is non-empty iff version stays -1
    p.version = v;
  }
  if (p.version != -1)
    for (int t = 0; t < kNumRawTypes; ++t)
      if (scopeOf(t) == kScopeBroker && versionSince(t) > p.version) setValue(p, t, 0.0);
  p.minRequired = p.enough && p.version != -1;
}

struct CpuWeights {
  double leaderBytesIn, leaderBytesOut, followerBytesIn;  // 0.7 / 0.15 / 0.15
};
// ModelUtils.estimateLeaderCpuUtilPerCore, static model; false: null
CCMI_BL_HD bool cpuUtilPerCore(const CpuWeights& w, double brokerCpuUtil, double brokerLeaderBytesIn,
                               double brokerLeaderBytesOut, double brokerFollowerBytesIn, double partitionBytesIn,
                               double partitionBytesOut, double* out) {
  if (brokerLeaderBytesIn == 0 && brokerLeaderBytesOut == 0) {
    *out = 0.0;
    return true;
  }
  if (brokerLeaderBytesIn * 1.05 < partitionBytesIn && brokerLeaderBytesIn > 10) return false;
  if (brokerLeaderBytesOut * 1.05 < partitionBytesOut && brokerLeaderBytesOut > 10) return false;
  const double inC = w.leaderBytesIn * brokerLeaderBytesIn;
  const double outC = w.leaderBytesOut * brokerLeaderBytesOut;
  const double folC = w.followerBytesIn * brokerFollowerBytesIn;
  const double total = inC + outC + folC;
  const double inR = brokerLeaderBytesIn == 0 ? 0 : partitionBytesIn / brokerLeaderBytesIn;
  const double outR = brokerLeaderBytesOut == 0 ? 0 : partitionBytesOut / brokerLeaderBytesOut;
  // Math.min(1, x): NaN if x is NaN
  const double inF = inR != inR ? inR : (1.0 <= inR ? 1.0 : inR);
  const double outF = outR != outR ? outR : (1.0 <= outR ? 1.0 : outR);
  const double leader = (inC * inF) + (outC * outF);
  *out = (leader / total) * brokerCpuUtil;
  return true;
}

// The values of one partition sample from the prepared broker holders of its leader; out[kPartitionMetrics].
// topicRaw[i]: the unconverted holder value of topicType(i), topicHas[i]: the holder exists. -> 0 built, 6 a broker
// holder of the estimate is missing (the reference throws), 7 the estimate is null.
CCMI_BL_HD int partitionSample(const Prepared& b, const CpuWeights& w, const double* topicRaw, const bool* topicHas,
                               int numLeaders, double partitionSizeRaw, double numCores, double* out) {
  for (int i = 0; i < kNumTopicTypes; ++i) {
    const int t = topicType(i);
    const double v = topicHas[i] ? convertUnit(topicRaw[i], t) : 0.0;
    out[metricDefOf(t)] = numLeaders == 0 ? 0 : v / numLeaders;
  }
  out[1] = convertUnit(partitionSizeRaw, kPartitionSize);
  if (!available(b, 1) || !available(b, 7) || !available(b, kBrokerCpuUtil) || !available(b, 0) || !available(b, 6))
    return 6;
  const double totalOut = convertUnit(b.value[1], 1) + convertUnit(b.value[7], 7);
  double perCore;
  if (!cpuUtilPerCore(w, b.value[kBrokerCpuUtil], convertUnit(b.value[0], 0), totalOut, convertUnit(b.value[6], 6),
                      out[2], out[3] + out[8], &perCore))
    return 7;
  out[0] = numCores * perCore;
  return 0;
}

// String.hashCode is jStringHash (jsem.h); TopicPartition.hashCode: 31 * (31 + partition) + topic.hashCode()
CCMI_BL_HD int32_t topicPartitionHash(int32_t topicHash, int32_t partition) {
  return (int32_t)(31u * (31u + (uint32_t)partition) + (uint32_t)topicHash);
}
CCMI_BL_HD uint32_t spread(int32_t h) { return (uint32_t)h ^ ((uint32_t)h >> 16); }
// the table a default HashMap has when it holds n keys and never resized early: 16 buckets, load factor 0.75
CCMI_BL_HD uint32_t tableCapacity(uint32_t n) {
  uint32_t cap = 16;
  while (n > cap / 4 * 3) cap <<= 1;
  return cap;
}
// the key of insertion rank `rank` meets `earlierInBucket` earlier keys in its bucket of tableCapacity(rank)
CCMI_BL_HD bool binFlagged(uint32_t earlierInBucket) { return earlierInBucket >= 8; }
CCMI_BL_HD bool sameBucket(uint32_t spreadA, uint32_t spreadB, uint32_t capacity) {
  return ((spreadA ^ spreadB) & (capacity - 1)) == 0;
}
// list-bin iteration order: (bucket at the final capacity, insertion rank)
CCMI_BL_HD bool iteratesBefore(uint32_t spreadA, uint32_t rankA, uint32_t spreadB, uint32_t rankB, uint32_t capacity) {
  const uint32_t a = spreadA & (capacity - 1), b = spreadB & (capacity - 1);
  return a != b ? a < b : rankA < rankB;
}

// The sort key of a record: node slot (18 bits) | topic + 1 (22) | partition + 1 (18) | type (6). Broker scope has
// topic + 1 == 0, topic scope partition + 1 == 0, so a node's records sort as broker types, then per topic the topic
// types followed by the partitions.
constexpr int kSlotShift = 46, kTopicShift = 24, kPartitionShift = 6;
constexpr int kMaxSlots = (1 << 18) - 1, kMaxTopics = (1 << 22) - 1, kMaxPartition = (1 << 18) - 2;
CCMI_BL_HD unsigned long long recordKey(uint32_t slot, int32_t topic, int32_t partition, int type) {
  return ((unsigned long long)slot << kSlotShift) | ((unsigned long long)(uint32_t)(topic + 1) << kTopicShift) |
         ((unsigned long long)(uint32_t)(partition + 1) << kPartitionShift) | (unsigned long long)type;
}
CCMI_BL_HD uint32_t keySlot(unsigned long long k) { return (uint32_t)(k >> kSlotShift); }
CCMI_BL_HD int32_t keyTopic(unsigned long long k) { return (int32_t)((k >> kTopicShift) & 0x3fffffu) - 1; }
CCMI_BL_HD int32_t keyPartition(unsigned long long k) { return (int32_t)((k >> kPartitionShift) & 0x3ffffu) - 1; }
CCMI_BL_HD int keyType(unsigned long long k) { return (int)(k & 63u); }

}  // namespace bl
}  // namespace ccmi
