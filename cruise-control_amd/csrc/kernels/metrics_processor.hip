// gfx950 kernels of ccmi_metrics_processor (K20): CruiseControlMetricsProcessor.process over one sampling round's raw
// records. The arithmetic is engine/broker_load.h; this file moves the data.
//
//     mp_keys         : one lane per record: broker id -> node slot (binary search in the sorted node ids; a broker that
//                       is not a node gets slot N and is counted), the 64-bit key of broker_load.h, entry {key, arrival}.
//     mp_hist / mp_scan_counts / mp_scatter : a stable LSD radix sort of the entries, 8 bits per pass, in the shape of
//                       K13's passes (tile histogram in LDS, one-workgroup scan in digit-major order, ballot-ranked
//                       scatter), over the key bits the call can set. Equal keys keep arrival order.
//     mp_reduce       : one lane per run head: the holder of that key, records added serially in arrival order (the
//                       double sum of an AVG holder depends on it). A long run is slow but exact.
//     mp_flag_* / mp_scan_* / mp_gather_* : ballot-free flag, scan, gather compactions: the partition-map keys (run
//                       heads of PARTITION_SIZE) and the topic-set keys (first partition key of a topic) of every node.
//     mp_hash_order   : one lane per key: its insertion rank, the early-resize / tree-bin check and its place in the
//                       HashMap's iteration order, all by counting over its node's keys (quadratic in a node's keys; a
//                       node has a few hundred).
//     mp_led_keys     : one lane per partition: (leader slot, dot-handled topic, topic) -> the same radix sort gives
//                       every node its led partitions grouped by topic.
//     mp_prepare      : one lane per node: BrokerLoad.prepareBrokerMetrics -> one bl::Prepared.
//     mp_partitions   : one lane per partition: buildPartitionMetricSample, holders found by binary search.
//     mp_broker_rows  : one lane per (node, broker metric): buildBrokerMetricSample.
//     mp_gather_rows  : the built rows, compacted in index order.
// Every launch is a kernel boundary on the processor's stream; no workgroup reads another's writes inside a launch.
// Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../engine/metrics_processor.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kSortBlock = 256;
constexpr int kSortWaveItems = kMpSortTile / 4;
constexpr int kSortRounds = kSortWaveItems / 64;
constexpr int kScanBlock = 1024;
constexpr int kScanPerThread = kMpScanTile / kMpBlock;
static_assert(sizeof(MpEntry) == 16 && kSortRounds == 8 && kScanPerThread == 8, "shapes");

__device__ __forceinline__ long long lowerBoundKey(const MpEntry* __restrict__ S, long long n, unsigned long long key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (S[mid].key < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ long long findKey(const MpEntry* __restrict__ S, long long n, unsigned long long key) {
  const long long i = lowerBoundKey(S, n, key);
  return i < n && S[i].key == key ? i : -1;
}
__device__ __forceinline__ uint32_t lowerBoundU32(const uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t lowerBoundU64(const unsigned long long* __restrict__ a, uint32_t n,
                                                  unsigned long long v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kMpBlock) void mp_keys(MpRecords R, const int32_t* __restrict__ nodeId,
                                                    const int32_t* __restrict__ nodeSlot, int32_t N,
                                                    MpEntry* __restrict__ out, uint32_t* __restrict__ dropped) {
  const long long i = (long long)blockIdx.x * kMpBlock + threadIdx.x;
  if (i >= R.n) return;
  const int32_t b = R.broker[i];
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nodeId[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  uint32_t slot = (uint32_t)N;
  if (lo < N && nodeId[lo] == b) slot = (uint32_t)nodeSlot[lo];
  else atomicAdd(dropped, 1u);
  MpEntry e;
  e.key = bl::recordKey(slot, R.topic[i], R.partition[i], R.type[i]);
  e.idx = (uint32_t)i;
  e.pad = 0;
  *reinterpret_cast<uint4*>(out + i) = *reinterpret_cast<const uint4*>(&e);
}

__global__ __launch_bounds__(kSortBlock) void mp_hist(const MpEntry* __restrict__ src, uint32_t n, uint32_t off,
                                                      int tiles, uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)kMpSortTile;
#pragma unroll
  for (int k = 0; k < kMpSortTile / kSortBlock; ++k) {
    const uint32_t i = base + k * kSortBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[(uint32_t)(src[i].key >> off) & 0xffu], 1u);
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kScanBlock) void mp_scan_counts(int words, uint32_t* __restrict__ counts) {
  (void)scanCountsInPlace<uint32_t, kScanBlock>(counts, words);
}

__global__ __launch_bounds__(kSortBlock) void mp_scatter(const MpEntry* __restrict__ src, MpEntry* __restrict__ dst,
                                                         uint32_t n, uint32_t off, int tiles,
                                                         const uint32_t* __restrict__ offsets) {
  const uint32_t base = blockIdx.x * (uint32_t)kMpSortTile;
  if (base >= n) return;
  __shared__ uint32_t cnt[4][256];
  __shared__ uint32_t wbase[4][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
  __syncthreads();
  MpEntry e[kSortRounds];
  uint32_t dg[kSortRounds], loc[kSortRounds];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kSortRounds; ++k) {
    const uint32_t i = base + wave * kSortWaveItems + k * 64 + lane;
    const bool valid = i < n;
    if (valid) *reinterpret_cast<uint4*>(&e[k]) = *reinterpret_cast<const uint4*>(src + i);
    const uint32_t d = valid ? (uint32_t)(e[k].key >> off) & 0xffu : 0u;
    unsigned long long match = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(valid && bit);
      match &= bit ? bal : ~bal;
    }
    const uint32_t before = (uint32_t)__popcll(match & below);
    uint32_t old = 0;
    if (valid) old = cnt[wave][d];
    __builtin_amdgcn_wave_barrier();
    if (valid && before == 0) cnt[wave][d] = old + (uint32_t)__popcll(match);
    __builtin_amdgcn_wave_barrier();
    dg[k] = d;
    loc[k] = old + before;
  }
  __syncthreads();
  {
    uint32_t b = offsets[(size_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      wbase[w][threadIdx.x] = b;
      b += cnt[w][threadIdx.x];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSortRounds; ++k) {
    const uint32_t i = base + wave * kSortWaveItems + k * 64 + lane;
    if (i < n) {
      const uint32_t to = wbase[wave][dg[k]] + loc[k];
      if (to < n) *reinterpret_cast<uint4*>(dst + to) = *reinterpret_cast<const uint4*>(&e[k]);
    }
  }
}

__global__ __launch_bounds__(kMpBlock) void mp_reduce(const MpEntry* __restrict__ S, long long n, MpRecords R, int32_t N,
                                                      double* __restrict__ hval) {
  const long long i = (long long)blockIdx.x * kMpBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = S[i].key;
  if (bl::keySlot(key) >= (uint32_t)N || (i > 0 && S[i - 1].key == key)) return;
  const bool latest = bl::keyType(key) == bl::kPartitionSize;
  bl::Holder h;
  bl::holderReset(h);
  for (long long j = i; j < n && S[j].key == key; ++j) {
    const uint32_t r = S[j].idx;
    bl::holderRecord(h, latest, R.value[r], R.time[r]);
  }
  hval[i] = bl::holderValue(h, latest);
}

// ---- flag scan: per-tile sums, one-workgroup scan of the sums, per-tile prefixes
__global__ __launch_bounds__(kMpBlock) void mp_scan_sums(const uint32_t* __restrict__ flags, long long n,
                                                         uint32_t* __restrict__ blockSums) {
  const long long base = (long long)blockIdx.x * kMpScanTile + (long long)threadIdx.x * kScanPerThread;
  unsigned long long s = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k)
    if (base + k < n) s += flags[base + k];
  s = waveSum(s);
  __shared__ uint32_t w[kMpBlock / 64];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = (uint32_t)s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int k = 0; k < kMpBlock / 64; ++k) t += w[k];
    blockSums[blockIdx.x] = t;
  }
}
__global__ __launch_bounds__(kScanBlock) void mp_scan_blocks(uint32_t* __restrict__ blockSums, int blocks,
                                                             uint32_t* __restrict__ total) {
  const uint32_t t = scanCountsInPlace<uint32_t, kScanBlock>(blockSums, blocks);
  if (threadIdx.x == 0) *total = t;
}
__global__ __launch_bounds__(kMpBlock) void mp_scan_apply(uint32_t* __restrict__ flags, long long n,
                                                          const uint32_t* __restrict__ blockSums) {
  const long long base = (long long)blockIdx.x * kMpScanTile + (long long)threadIdx.x * kScanPerThread;
  uint32_t v[kScanPerThread], s = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    v[k] = base + k < n ? flags[base + k] : 0u;
    s += v[k];
  }
  uint32_t total;
  uint32_t run = blockExclusiveScan<uint32_t, kMpBlock>(s, &total) + blockSums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    if (base + k < n) flags[base + k] = run;
    run += v[k];
  }
}

__device__ __forceinline__ bool isPe(const MpEntry* __restrict__ S, long long i, int32_t N) {
  const unsigned long long key = S[i].key;
  return bl::keySlot(key) < (uint32_t)N && bl::keyType(key) == bl::kPartitionSize && (i == 0 || S[i - 1].key != key);
}
__global__ __launch_bounds__(kMpBlock) void mp_flag_pe(const MpEntry* __restrict__ S, long long n, int32_t N,
                                                       uint32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * kMpBlock + threadIdx.x;
  if (i < n) flags[i] = isPe(S, i, N) ? 1u : 0u;
}
__global__ __launch_bounds__(kMpBlock) void mp_gather_pe(const MpEntry* __restrict__ S, long long n,
                                                         const uint32_t* __restrict__ scanned,
                                                         const int32_t* __restrict__ topicHash, MpKeyList pe) {
  const long long i = (long long)blockIdx.x * kMpBlock + threadIdx.x;
  if (i >= n || scanned[i + 1] == scanned[i]) return;
  const uint32_t k = scanned[i];
  if (k >= pe.count) return;
  const unsigned long long key = S[i].key;
  pe.slot[k] = bl::keySlot(key);
  pe.hash[k] = bl::topicPartitionHash(topicHash[bl::keyTopic(key)], bl::keyPartition(key));
  pe.arr[k] = S[i].idx;
  pe.ref[k] = (uint32_t)i;
}
// the first partition key of a (slot, topic): the key's bits above the partition field change
__global__ __launch_bounds__(kMpBlock) void mp_flag_te(const MpEntry* __restrict__ S, MpKeyList pe,
                                                       uint32_t* __restrict__ flags) {
  const uint32_t k = blockIdx.x * (uint32_t)kMpBlock + threadIdx.x;
  if (k >= pe.count) return;
  flags[k] = k == 0 || (S[pe.ref[k]].key >> bl::kTopicShift) != (S[pe.ref[k - 1]].key >> bl::kTopicShift) ? 1u : 0u;
}
__global__ __launch_bounds__(kMpBlock) void mp_gather_te(const MpEntry* __restrict__ S, MpKeyList pe,
                                                         const uint32_t* __restrict__ scanned,
                                                         const int32_t* __restrict__ topicHash, MpKeyList te,
                                                         unsigned long long* __restrict__ teKey) {
  const uint32_t k = blockIdx.x * (uint32_t)kMpBlock + threadIdx.x;
  if (k >= pe.count || scanned[k + 1] == scanned[k]) return;
  const uint32_t m = scanned[k];
  if (m >= te.count) return;
  const unsigned long long tk = S[pe.ref[k]].key >> bl::kTopicShift;
  uint32_t first = pe.arr[k];
  for (uint32_t j = k + 1; j < pe.count && (S[pe.ref[j]].key >> bl::kTopicShift) == tk; ++j)
    first = pe.arr[j] < first ? pe.arr[j] : first;
  const int32_t topic = bl::keyTopic(S[pe.ref[k]].key);
  te.slot[m] = pe.slot[k];
  te.hash[m] = topicHash[topic];
  te.arr[m] = first;
  te.ref[m] = (uint32_t)topic;
  teKey[m] = tk;
}

__global__ __launch_bounds__(kMpBlock) void mp_hash_order(MpKeyList L, uint8_t* __restrict__ flagged) {
  const uint32_t i = blockIdx.x * (uint32_t)kMpBlock + threadIdx.x;
  if (i >= L.count) return;
  const uint32_t s = L.slot[i];
  const uint32_t lo = lowerBoundU32(L.slot, L.count, s), hi = lowerBoundU32(L.slot, L.count, s + 1);
  const uint32_t a = L.arr[i], h = bl::spread(L.hash[i]);
  uint32_t rank = 0;
  for (uint32_t j = lo; j < hi; ++j) rank += L.arr[j] < a ? 1u : 0u;
  const uint32_t capAt = bl::tableCapacity(rank), capFinal = bl::tableCapacity(hi - lo);
  uint32_t earlier = 0, pos = 0;
  for (uint32_t j = lo; j < hi; ++j) {
    const uint32_t aj = L.arr[j], hj = bl::spread(L.hash[j]);
    if (aj < a && bl::sameBucket(hj, h, capAt)) earlier++;
    if (j != i && bl::iteratesBefore(hj, aj, h, a, capFinal)) pos++;
  }
  if (lo + pos < hi) L.order[lo + pos] = i;
  if (bl::binFlagged(earlier)) flagged[s] = 1;
}

__global__ __launch_bounds__(kMpBlock) void mp_led_keys(MpCluster C, int32_t N, MpEntry* __restrict__ out) {
  const int p = blockIdx.x * kMpBlock + threadIdx.x;
  if (p >= C.P) return;
  const int32_t ls = C.leaderSlot[p];
  MpEntry e;
  e.key = ((unsigned long long)(ls >= 0 ? (uint32_t)ls : (uint32_t)N) << kLedSlotShift) |
          ((unsigned long long)(uint32_t)C.hid[p] << kLedHidShift) | (unsigned long long)(uint32_t)C.topic[p];
  e.idx = (uint32_t)p;
  e.pad = 0;
  *reinterpret_cast<uint4*>(out + p) = *reinterpret_cast<const uint4*>(&e);
}

__device__ __forceinline__ bool topicReported(const unsigned long long* __restrict__ teKey, uint32_t teCount,
                                              uint32_t slot, int32_t metricTopic) {
  if (metricTopic < 0) return false;
  const unsigned long long k = ((unsigned long long)slot << (bl::kSlotShift - bl::kTopicShift)) |
                               (unsigned long long)(uint32_t)(metricTopic + 1);
  const uint32_t m = lowerBoundU64(teKey, teCount, k);
  return m < teCount && teKey[m] == k;
}

__global__ __launch_bounds__(kMpBlock) void mp_prepare(MpSorted R, MpKeyList pe, MpKeyList te,
                                                       const unsigned long long* __restrict__ teKey,
                                                       const MpEntry* __restrict__ led, MpCluster C, int32_t N,
                                                       bl::Prepared* __restrict__ prepared) {
  const int s = blockIdx.x * kMpBlock + threadIdx.x;
  if (s >= N) return;
  bl::Prepared P;
  for (int t = 0; t < bl::kNumRawTypes; ++t) P.value[t] = 0.0;
  P.avail = 0;
  P.diskUsage = 0.0;
  P.version = -1;
  P.minRequired = 0;
  P.enough = 0;
  const long long recLo = lowerBoundKey(R.S, R.n, (unsigned long long)s << bl::kSlotShift);
  const long long recHi = lowerBoundKey(R.S, R.n, (unsigned long long)(s + 1) << bl::kSlotShift);
  P.hasLoad = recHi > recLo;
  if (P.hasLoad) {
    for (long long i = recLo; i < recHi && bl::keyTopic(R.S[i].key) < 0; ++i)
      if (i == recLo || R.S[i - 1].key != R.S[i].key) bl::setValue(P, bl::keyType(R.S[i].key), R.hval[i]);
    // enoughTopicPartitionMetrics and the follower-fetch rule over the led partitions, grouped by dot-handled topic
    const long long ledLo = lowerBoundKey(led, C.P, (unsigned long long)s << kLedSlotShift);
    const long long ledHi = lowerBoundKey(led, C.P, (unsigned long long)(s + 1) << kLedSlotShift);
    int topics = 0, missingTopics = 0, missingPartitions = 0;
    bool followerFetch = false, curMissing = false;
    long long prevHid = -1;
    for (long long i = ledLo; i < ledHi; ++i) {
      const uint32_t p = led[i].idx;
      const long long hid = (long long)((led[i].key >> kLedHidShift) & 0x3fffffu);
      if (hid != prevHid) {
        prevHid = hid;
        topics++;
        curMissing = !topicReported(teKey, te.count, (uint32_t)s, C.metricTopic[p]);
        if (curMissing) missingTopics++;
      }
      if (curMissing) missingPartitions++;
      if (C.multi[p]) followerFetch = true;
    }
    P.enough = bl::enoughMetrics(missingTopics, topics, missingPartitions, (int)(ledHi - ledLo));
    const uint32_t tLo = lowerBoundU32(te.slot, te.count, (uint32_t)s), tHi = lowerBoundU32(te.slot, te.count, (uint32_t)s + 1);
    if (P.enough && tHi > tLo) {
      double sums[bl::kNumTopicTypes];
      for (int k = 0; k < bl::kNumTopicTypes; ++k) sums[k] = 0.0;
      for (uint32_t x = tLo; x < tHi; ++x) {
        uint32_t m = te.order[x];
        if (m >= te.count) m = x;  // never: every place of a segment is written
        const int32_t topic = (int32_t)te.ref[m];
        for (int k = 0; k < bl::kNumTopicTypes; ++k) {
          const long long pos = findKey(R.S, R.n, bl::recordKey((uint32_t)s, topic, -1, bl::topicType(k)));
          sums[k] += pos >= 0 ? R.hval[pos] : 0.0;
        }
      }
      for (int k = 0; k < bl::kNumTopicTypes; ++k) bl::setValue(P, bl::sumTarget(bl::topicType(k)), sums[k]);
    }
    const uint32_t pLo = lowerBoundU32(pe.slot, pe.count, (uint32_t)s), pHi = lowerBoundU32(pe.slot, pe.count, (uint32_t)s + 1);
    double disk = 0.0;
    for (uint32_t x = pLo; x < pHi; ++x) {
      uint32_t k = pe.order[x];
      if (k >= pe.count) k = x;
      disk += R.hval[pe.ref[k]];
    }
    P.diskUsage = bl::convertUnit(disk, bl::kPartitionSize);
    bl::versionLogic(P, followerFetch);
  }
  prepared[s] = P;
}

__global__ __launch_bounds__(kMpBlock) void mp_partitions(MpSorted R, const unsigned long long* __restrict__ teKey,
                                                          uint32_t teCount, const MpEntry* __restrict__ led,
                                                          MpCluster C, int32_t N,
                                                          const bl::Prepared* __restrict__ prepared,
                                                          const double* __restrict__ cores, bl::CpuWeights w,
                                                          uint8_t* __restrict__ skip, uint32_t* __restrict__ flags,
                                                          double* __restrict__ staged,
                                                          uint32_t* __restrict__ skippedByNode) {
  const int p = blockIdx.x * kMpBlock + threadIdx.x;
  if (p >= C.P) return;
  int code = 0, under = N;
  bool built = false;
  if (!C.interested || C.interested[p]) {
    const int32_t ls = C.leaderSlot[p];
    if (ls == -1) code = 1;
    else if (ls < 0 || ls >= N) code = 8;
    else {
      under = ls;
      const bl::Prepared& B = prepared[ls];
      const int32_t mt = C.metricTopic[p];
      const int32_t number = C.number[p];
      if (!B.hasLoad || !bl::available(B, bl::kBrokerCpuUtil)) code = 2;
      else if (cores[ls] != cores[ls]) code = 3;
      else if (!topicReported(teKey, teCount, (uint32_t)ls, mt)) code = 4;
      else {
        double raw[bl::kNumTopicTypes];
        bool has[bl::kNumTopicTypes];
        for (int k = 0; k < bl::kNumTopicTypes; ++k) {
          const long long pos = findKey(R.S, R.n, bl::recordKey((uint32_t)ls, mt, -1, bl::topicType(k)));
          has[k] = pos >= 0;
          raw[k] = pos >= 0 ? R.hval[pos] : 0.0;
        }
        const unsigned long long lk = ((unsigned long long)(uint32_t)ls << kLedSlotShift) |
                                      ((unsigned long long)(uint32_t)C.hid[p] << kLedHidShift) |
                                      (unsigned long long)(uint32_t)C.topic[p];
        const int numLeaders = (int)(lowerBoundKey(led, C.P, lk + 1) - lowerBoundKey(led, C.P, lk));
        const long long sizePos = number >= 0 && number <= bl::kMaxPartition
                                      ? findKey(R.S, R.n, bl::recordKey((uint32_t)ls, mt, number, bl::kPartitionSize))
                                      : -1;
        if (sizePos < 0) code = 5;
        else {
          double out[bl::kPartitionMetrics];
          code = bl::partitionSample(B, w, raw, has, numLeaders, R.hval[sizePos], cores[ls], out);
          if (code == 6) under = N;  // the exception is counted under UNRECOGNIZED_BROKER_ID
          if (code == 0) {
            built = true;
            for (int m = 0; m < bl::kPartitionMetrics; ++m) staged[(size_t)p * bl::kPartitionMetrics + m] = out[m];
          }
        }
      }
    }
    if (code) atomicAdd(&skippedByNode[under], 1u);
  }
  skip[p] = (uint8_t)code;
  flags[p] = built ? 1u : 0u;
}

__device__ __forceinline__ int brokerTypeOfDef(int m) {
  switch (m) {
    case 0: return 5;
    case 2: return 0;
    case 3: return 1;
    case 4: return 8;
    case 5: return 9;
    case 6: return 10;
    case 7: return 6;
    case 8: return 7;
    default: return m + 7;  // 9..55 -> 16..62; 1 (DISK_USAGE) is diskUsage()
  }
}

__global__ __launch_bounds__(kMpBlock) void mp_broker_rows(const bl::Prepared* __restrict__ prepared, int32_t N,
                                                           uint8_t* __restrict__ skip, uint32_t* __restrict__ flags,
                                                           double* __restrict__ staged) {
  const long long g = (long long)blockIdx.x * kMpBlock + threadIdx.x;
  if (g >= (long long)N * bl::kBrokerMetrics) return;
  const int s = (int)(g / bl::kBrokerMetrics), m = (int)(g % bl::kBrokerMetrics);
  const bl::Prepared& B = prepared[s];
  unsigned long long all = 0;
  for (int t = 0; t < bl::kNumRawTypes; ++t)
    if (bl::scopeOf(t) == bl::kScopeBroker) all |= 1ull << t;
  const int code = !B.hasLoad ? 1 : !B.minRequired ? 2 : (B.avail & all) != all ? 3 : 0;
  if (m == 0) {
    skip[s] = (uint8_t)code;
    flags[s] = code ? 0u : 1u;
  }
  if (code) return;
  const int t = brokerTypeOfDef(m);
  staged[g] = m == 1 ? B.diskUsage : bl::convertUnit(B.value[t], t);
}

__global__ __launch_bounds__(kMpBlock) void mp_gather_rows(const uint32_t* __restrict__ scanned, long long n, int M,
                                                           const double* __restrict__ src, long long capacity,
                                                           int32_t* __restrict__ entity, double* __restrict__ dst,
                                                           const bl::Prepared* __restrict__ prepared,
                                                           int8_t* __restrict__ version) {
  const long long g = (long long)blockIdx.x * kMpBlock + threadIdx.x;
  if (g >= n * M) return;
  const long long i = g / M;
  const int m = (int)(g % M);
  if (scanned[i + 1] == scanned[i]) return;
  const long long k = scanned[i];
  if (k >= capacity) return;
  dst[k * M + m] = src[g];
  if (m == 0) {
    entity[k] = (int32_t)i;
    if (version) version[k] = (int8_t)prepared[i].version;
  }
}

inline int blocksFor(long long n, int per) { return (int)std::max<long long>(1, (n + per - 1) / per); }

}  // namespace

size_t mpSortCountWords(long long n) { return (size_t)256 * (size_t)blocksFor(n, kMpSortTile); }
size_t mpScanBlocks(long long n) { return (size_t)blocksFor(n, kMpScanTile); }

void mpLaunchKeys(const MpRecords& R, const int32_t* nodeIdSorted, const int32_t* nodeSlotSorted, int32_t N,
                  MpEntry* out, uint32_t* dropped, hipStream_t st) {
  if (R.n <= 0) return;
  hipLaunchKernelGGL(mp_keys, dim3(blocksFor(R.n, kMpBlock)), dim3(kMpBlock), 0, st, R, nodeIdSorted, nodeSlotSorted, N,
                     out, dropped);
}

MpEntry* mpLaunchSort(MpEntry* a, MpEntry* b, long long n, int keyBits, uint32_t* counts, hipStream_t st) {
  if (n <= 1) return a;
  const int tiles = blocksFor(n, kMpSortTile);
  MpEntry *src = a, *dst = b;
  for (int off = 0; off < keyBits; off += 8) {
    hipLaunchKernelGGL(mp_hist, dim3(tiles), dim3(kSortBlock), 0, st, src, (uint32_t)n, (uint32_t)off, tiles, counts);
    hipLaunchKernelGGL(mp_scan_counts, dim3(1), dim3(kScanBlock), 0, st, 256 * tiles, counts);
    hipLaunchKernelGGL(mp_scatter, dim3(tiles), dim3(kSortBlock), 0, st, src, dst, (uint32_t)n, (uint32_t)off, tiles,
                       counts);
    std::swap(src, dst);
  }
  return src;
}

void mpLaunchReduce(const MpEntry* S, long long n, const MpRecords& R, int32_t N, double* hval, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(mp_reduce, dim3(blocksFor(n, kMpBlock)), dim3(kMpBlock), 0, st, S, n, R, N, hval);
}

void mpLaunchScan(uint32_t* flags, long long n, uint32_t* blockSums, hipStream_t st) {
  const int blocks = blocksFor(n, kMpScanTile);
  hipLaunchKernelGGL(mp_scan_sums, dim3(blocks), dim3(kMpBlock), 0, st, flags, n, blockSums);
  hipLaunchKernelGGL(mp_scan_blocks, dim3(1), dim3(kScanBlock), 0, st, blockSums, blocks, flags + n);
  hipLaunchKernelGGL(mp_scan_apply, dim3(blocks), dim3(kMpBlock), 0, st, flags, n, blockSums);
}

void mpLaunchFlagPe(const MpEntry* S, long long n, int32_t N, uint32_t* flags, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(mp_flag_pe, dim3(blocksFor(n, kMpBlock)), dim3(kMpBlock), 0, st, S, n, N, flags);
}
void mpLaunchGatherPe(const MpEntry* S, long long n, const uint32_t* scanned, const int32_t* topicHash, MpKeyList pe,
                      hipStream_t st) {
  if (n <= 0 || !pe.count) return;
  hipLaunchKernelGGL(mp_gather_pe, dim3(blocksFor(n, kMpBlock)), dim3(kMpBlock), 0, st, S, n, scanned, topicHash, pe);
}
void mpLaunchFlagTe(const MpEntry* S, MpKeyList pe, uint32_t* flags, hipStream_t st) {
  if (!pe.count) return;
  hipLaunchKernelGGL(mp_flag_te, dim3(blocksFor(pe.count, kMpBlock)), dim3(kMpBlock), 0, st, S, pe, flags);
}
void mpLaunchGatherTe(const MpEntry* S, MpKeyList pe, const uint32_t* scanned, const int32_t* topicHash, MpKeyList te,
                      unsigned long long* teKey, hipStream_t st) {
  if (!pe.count || !te.count) return;
  hipLaunchKernelGGL(mp_gather_te, dim3(blocksFor(pe.count, kMpBlock)), dim3(kMpBlock), 0, st, S, pe, scanned,
                     topicHash, te, teKey);
}
void mpLaunchHashOrder(MpKeyList list, uint8_t* flagged, hipStream_t st) {
  if (!list.count) return;
  hipLaunchKernelGGL(mp_hash_order, dim3(blocksFor(list.count, kMpBlock)), dim3(kMpBlock), 0, st, list, flagged);
}
void mpLaunchLedKeys(const MpCluster& C, int32_t N, MpEntry* out, hipStream_t st) {
  if (C.P <= 0) return;
  hipLaunchKernelGGL(mp_led_keys, dim3(blocksFor(C.P, kMpBlock)), dim3(kMpBlock), 0, st, C, N, out);
}
void mpLaunchPrepare(const MpSorted& R, MpKeyList pe, MpKeyList te, const unsigned long long* teKey,
                     const MpEntry* led, const MpCluster& C, int32_t N, bl::Prepared* prepared, hipStream_t st) {
  if (N <= 0) return;
  hipLaunchKernelGGL(mp_prepare, dim3(blocksFor(N, kMpBlock)), dim3(kMpBlock), 0, st, R, pe, te, teKey, led, C, N,
                     prepared);
}
void mpLaunchPartitions(const MpSorted& R, const unsigned long long* teKey, uint32_t teCount, const MpEntry* led,
                        const MpCluster& C, int32_t N, const bl::Prepared* prepared, const double* cores,
                        bl::CpuWeights w, uint8_t* skip, uint32_t* flags, double* staged, uint32_t* skippedByNode,
                        hipStream_t st) {
  if (C.P <= 0) return;
  hipLaunchKernelGGL(mp_partitions, dim3(blocksFor(C.P, kMpBlock)), dim3(kMpBlock), 0, st, R, teKey, teCount, led, C, N,
                     prepared, cores, w, skip, flags, staged, skippedByNode);
}
void mpLaunchBrokerRows(const bl::Prepared* prepared, int32_t N, uint8_t* skip, uint32_t* flags, double* staged,
                        hipStream_t st) {
  if (N <= 0) return;
  hipLaunchKernelGGL(mp_broker_rows, dim3(blocksFor((long long)N * bl::kBrokerMetrics, kMpBlock)), dim3(kMpBlock), 0,
                     st, prepared, N, skip, flags, staged);
}
void mpLaunchGatherRows(const uint32_t* scanned, long long n, int M, const double* src, long long capacity,
                        int32_t* entity, double* dst, const bl::Prepared* prepared, int8_t* version, hipStream_t st) {
  if (n <= 0 || capacity <= 0) return;
  hipLaunchKernelGGL(mp_gather_rows, dim3(blocksFor(n * M, kMpBlock)), dim3(kMpBlock), 0, st, scanned, n, M, src,
                     capacity, entity, dst, prepared, version);
}

}  // namespace ccmi
