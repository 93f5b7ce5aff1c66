// What ccmi_metrics_processor.cpp hands the K20 kernels (kernels/metrics_processor.hip): plain pointers into the
// processor's DevBuf pieces, and one launcher per step. Every list below is sorted by node slot, so a node's segment
// of a list is found by binary search and no offsets table is kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "broker_load.h"

namespace ccmi {

constexpr int kMpBlock = 256;       // the workgroup of the one-lane-per-item kernels
constexpr int kMpSortTile = 2048;   // entries per workgroup of a radix pass
constexpr int kMpScanTile = 2048;   // flags per workgroup of the flag scan

struct MpEntry {  // a sort entry: 16 bytes, moved with one 16-byte access
  unsigned long long key;
  uint32_t idx, pad;
};

struct MpRecords {  // the buffered records, in arrival order
  const uint8_t* type;
  const int32_t* broker;
  const long long* time;
  const double* value;
  const int32_t* topic;  // interned
  const int32_t* partition;
  long long n;
};

struct MpKeyList {  // a broker-major list of HashMap keys: the partition map (PE) or the topic set (TE)
  uint32_t* slot;   // node slot
  int32_t* hash;    // hashCode of the key
  uint32_t* arr;    // first arrival: the insertion order
  uint32_t* ref;    // PE: position of the holder in the sorted records; TE: the interned topic
  uint32_t* order;  // [count] list indices in iteration order, segment by segment
  uint32_t count;
};

struct MpCluster {  // per partition, computed by the host from the topology
  const int32_t* leaderSlot;   // node slot, -1 no leader, -2 the leader is not a node
  const int32_t* metricTopic;  // interned id of the dot-handled topic, -1 not reported by anyone
  const int32_t* hid;          // dense id of the dot-handled topic name
  const int32_t* topic;        // the topology's topic index (the original name)
  const int32_t* number;       // partition number
  const uint8_t* multi;        // more than one replica
  const uint8_t* interested;   // nullable
  int32_t P;
};

struct MpSorted {
  const MpEntry* S;  // records by key, arrival order inside a key
  long long n;
  const double* hval;  // [n] the holder's value() at the first position of its run
};

constexpr int kLedSlotShift = 44, kLedHidShift = 22;  // led key: slot | hid (22) | topology topic (22)

size_t mpSortCountWords(long long n);
size_t mpScanBlocks(long long n);
void mpLaunchKeys(const MpRecords& R, const int32_t* nodeIdSorted, const int32_t* nodeSlotSorted, int32_t N,
                  MpEntry* out, uint32_t* dropped, hipStream_t st);
// stable LSD radix sort on the low keyBits bits; -> the buffer that holds the result (a or b)
MpEntry* mpLaunchSort(MpEntry* a, MpEntry* b, long long n, int keyBits, uint32_t* counts, hipStream_t st);
void mpLaunchReduce(const MpEntry* S, long long n, const MpRecords& R, int32_t N, double* hval, hipStream_t st);
// exclusive scan of flags[0, n) in place, flags[n] = the total
void mpLaunchScan(uint32_t* flags, long long n, uint32_t* blockSums, hipStream_t st);
void mpLaunchFlagPe(const MpEntry* S, long long n, int32_t N, uint32_t* flags, hipStream_t st);
void mpLaunchGatherPe(const MpEntry* S, long long n, const uint32_t* scanned, const int32_t* topicHash, MpKeyList pe,
                      hipStream_t st);
void mpLaunchFlagTe(const MpEntry* S, MpKeyList pe, uint32_t* flags, hipStream_t st);
void mpLaunchGatherTe(const MpEntry* S, MpKeyList pe, const uint32_t* scanned, const int32_t* topicHash, MpKeyList te,
                      unsigned long long* teKey, hipStream_t st);
void mpLaunchHashOrder(MpKeyList list, uint8_t* flagged, hipStream_t st);
void mpLaunchLedKeys(const MpCluster& C, int32_t N, MpEntry* out, hipStream_t st);
void mpLaunchPrepare(const MpSorted& R, MpKeyList pe, MpKeyList te, const unsigned long long* teKey,
                     const MpEntry* led, const MpCluster& C, int32_t N, bl::Prepared* prepared, hipStream_t st);
void mpLaunchPartitions(const MpSorted& R, const unsigned long long* teKey, uint32_t teCount, const MpEntry* led,
                        const MpCluster& C, int32_t N, const bl::Prepared* prepared, const double* cores,
                        bl::CpuWeights w, uint8_t* skip, uint32_t* flags, double* staged, uint32_t* skippedByNode,
                        hipStream_t st);
void mpLaunchBrokerRows(const bl::Prepared* prepared, int32_t N, uint8_t* skip, uint32_t* flags, double* staged,
                        hipStream_t st);
// rows i of src[n][M] with a set flag (scanned[i + 1] > scanned[i]) to dst[scanned[i]], below capacity
void mpLaunchGatherRows(const uint32_t* scanned, long long n, int M, const double* src, long long capacity,
                        int32_t* entity, double* dst, const bl::Prepared* prepared, int8_t* version, hipStream_t st);

}  // namespace ccmi
