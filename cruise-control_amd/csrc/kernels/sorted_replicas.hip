// gfx950 kernels for ccmi_sorted_replicas: per asked broker the list a freshly initialised SortedReplicas would iterate
// (SortedReplicas.java:75-90, ReplicaSortFunctionFactory, Replica.compareTo), built from the resident tables: the
// replica, broker and partition records, the Java loads (rLoad) and the static rank of Replica.compareTo's tail.
//
// K15 sorted_replicas_keys    : one lane per replica (grid-stride): the replica's current broker -> its segment
//                               (seg[B], -1 = not asked for), the selections of Model::selects, the score recomputed
//                               from rLoad the way LoadOps::groupAvg does (ldZero / ldAdd / ldAvg; an empty load
//                               scores 0) and the 64-bit key; writes key[r] (all ones = not selected) and segOf[r],
//                               and counts per segment: the lanes of a wave that share a segment add once.
//     sorted_replicas_offsets : one workgroup: segmentOffsets (segments.h) turns the n counts into the int64 offsets,
//                               the total and the longest segment, and clears the scatter cursors.
//     sorted_replicas_scatter : one lane per replica: a selected replica's {key, replica id} goes to
//                               offsets[seg] + its rank among the segment's arrivals (wave-aggregated cursor). The slot
//                               order inside a segment is whatever the atomics give; the keys are unique (rStatic is a
//                               dense rank of a tuple no two replicas share), so the sort alone fixes the result.
//     launchSegSort           : the shared segmented sort (segments.h) under SrLess: an LDS bitonic sort per segment,
//                               and merge passes into the second buffer only when the longest segment exceeds
//                               kSegSortTile; a segment of length len ends in buffer (segSortPasses(len) & 1).
//     sorted_replicas_gather  : two records per lane: entry -> {partition, broker} (one 16-byte store) and, when asked,
//                               the score decoded from the key's own bits, so it is the score exactly as compared (one
//                               16-byte store).
// The host reads the offsets, the total and the longest segment back after sorted_replicas_offsets (the caller gets the
// offsets whatever happens) and launches scatter, sort, merge and gather only when the total fits the capacity.
// Every launch is a kernel boundary on the session stream; no workgroup reads another's writes inside a launch; nothing
// spins or waits on another workgroup. Built with -ffp-contract=off: every expression is the reference's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ccmi.h"
#include "../engine/devtypes.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kSrBlock = 256;
constexpr int kSrMaxBlocks = 1024;
constexpr int kSrScanBlock = 1024;
constexpr int kSrSmallTile = 256;  // the 4 KB image of segments.h, under the name the tests read it by
static_assert(kSrSmallTile == kSegSmallTile, "the small LDS image is the shared sort's");

static_assert(sizeof(ccmi_swap_replica) == 8, "record sizes");

// valuesForGroup(resource group).avg() of a replica's load as LoadOps::groupAvg computes it; an empty load scores 0
__device__ __forceinline__ float srScore(const LoadVec& L, int res, int W) {
  if (!L.mask) return 0.f;
  if (res == R_CPU) return ldAvg(L.m[M_CPU], W);
  if (res == R_DISK) return ldAvg(L.m[M_DISK], W);
  Window acc;
  ldZero(acc, W);
  ldAdd(acc, L.m[res == R_NW_IN ? M_LBI : M_LBO], W);
  ldAdd(acc, L.m[res == R_NW_IN ? M_RBI : M_RBO], W);
  return ldAvg(acc, W);
}

__device__ __forceinline__ uint64_t srKeyOf(const uint4& e) { return ((uint64_t)e.y << 32) | (uint64_t)e.x; }

}  // namespace

// the order of the lists: the key, then the replica id (never reached between two replicas: their keys differ). The
// fourth word is not read, so the sort's compare-exchange loads 12 bytes per entry.
struct SrLess {
  static __device__ __forceinline__ bool less(const uint4& a, const uint4& b) {
    const uint64_t ka = srKeyOf(a), kb = srKeyOf(b);
    return ka != kb ? ka < kb : a.z < b.z;
  }
};

__global__ __launch_bounds__(kSrBlock) void sorted_replicas_keys(SrTables T, SrQuery q, uint64_t* __restrict__ keys,
                                                                 int32_t* __restrict__ segOf,
                                                                 uint32_t* __restrict__ counts) {
  const int stride = gridDim.x * kSrBlock;
  for (int base = blockIdx.x * kSrBlock; base < T.R; base += stride) {  // wave-uniform trip count
    const int r = base + (int)threadIdx.x;
    int seg = -1;
    uint64_t key = kSrNotSelected;
    if (r < T.R) {
      const ReplicaRec rec = T.replicas[r];
      const int b = rec.broker;
      if ((unsigned)b < (unsigned)T.B) seg = T.seg[b];
      if (seg >= 0 && (unsigned)rec.part < (unsigned)T.P) {
        const bool leader = (rec.flags & RF_LEADER) != 0;
        const bool origOff = (rec.flags & (RF_ORIG_OFFLINE | RF_ORIG_DEAD)) != 0;  // Replica.isOriginalOffline
        const bool off = (origOff && b == rec.orig) || !T.brokers[b].alive;        // Replica.isCurrentOffline
        const bool imm = rec.orig != b;
        bool keep = true;  // Model::selects
        if ((q.selectMask & CCMI_SEL_LEADERS) && !leader) keep = false;
        if ((q.selectMask & CCMI_SEL_FOLLOWERS) && leader) keep = false;
        if ((q.selectMask & CCMI_SEL_ONLINE) && off) keep = false;
        if ((q.selectMask & CCMI_SEL_OFFLINE) && !off) keep = false;
        if ((q.selectMask & CCMI_SEL_IMMIGRANTS) && !imm) keep = false;
        if ((q.selectMask & CCMI_SEL_IMMIGRANT_OR_OFFLINE) && !(imm || off)) keep = false;
        if (T.topicExcluded || T.topicIncluded) {
          const int topic = T.parts[rec.part].topic;
          const bool inT = (unsigned)topic < (unsigned)T.T;
          // ReplicaSortFunctionFactory.java:144-146: an original-offline replica passes whatever its topic
          if (T.topicExcluded && !origOff && inT && T.topicExcluded[topic]) keep = false;
          if (T.topicIncluded && !(inT && T.topicIncluded[topic])) keep = false;
        }
        if (q.aboveRes >= 0 && !(rec.util[q.aboveRes] > q.aboveLimit)) keep = false;
        if (q.belowRes >= 0 && !(rec.util[q.belowRes] < q.belowLimit)) keep = false;
        if (keep) {
          uint64_t k = 0;
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            if (q.prio[i] == CCMI_PRIO_OFFLINE && !off) k |= 1ull << (63 - i);
            if (q.prio[i] == CCMI_PRIO_IMMIGRANTS && !imm) k |= 1ull << (63 - i);
          }
          if (q.scoreRes >= 0) {
            const uint32_t bits = (uint32_t)__float_as_int(srScore(T.rLoad[r], q.scoreRes, T.W));
            uint32_t u = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);  // Double.compare order: -0.0 < 0.0
            if (q.scoreReverse) u = ~u;  // Double.compare(-a, -b)
            k |= (uint64_t)u << 30;
          }
          if (!off) k |= 1ull << 29;
          key = k | (uint64_t)((uint32_t)T.rStatic[r] & 0x1fffffffu);
        } else {
          seg = -1;
        }
      } else {
        seg = -1;
      }
      keys[r] = key;
      segOf[r] = seg;
    }
    (void)waveSegAdd(counts, seg, seg >= 0);
  }
}

// state[0] = total, state[1] = the longest segment, state[2 + i] = offsets[i], i <= n
__global__ __launch_bounds__(kSrScanBlock) void sorted_replicas_offsets(const uint32_t* __restrict__ counts, int n,
                                                                        unsigned long long* __restrict__ state,
                                                                        uint32_t* __restrict__ cursor) {
  if (blockIdx.x != 0) return;
  segmentOffsets<kSrScanBlock>(counts, n, false, state, cursor);
}

__global__ __launch_bounds__(kSrBlock) void sorted_replicas_scatter(int R, int n, const uint64_t* __restrict__ keys,
                                                                    const int32_t* __restrict__ segOf,
                                                                    const unsigned long long* __restrict__ offsets,
                                                                    uint32_t* __restrict__ cursor,
                                                                    SortEntry* __restrict__ entries) {
  const int stride = gridDim.x * kSrBlock;
  for (int base = blockIdx.x * kSrBlock; base < R; base += stride) {  // wave-uniform trip count
    const int r = base + (int)threadIdx.x;
    int seg = -1;
    uint64_t key = kSrNotSelected;
    if (r < R) {
      seg = segOf[r];
      key = keys[r];
    }
    const bool active = seg >= 0 && seg < n;
    const uint32_t slot = waveSegAdd(cursor, seg, active);
    if (active) {
      const unsigned long long at = offsets[seg] + slot;
      if (at < offsets[seg + 1]) {  // always: the counts came from the same keys
        uint4 e;  // {lo = key, hi = replica id}
        e.x = (uint32_t)key;
        e.y = (uint32_t)(key >> 32);
        e.z = (uint32_t)r;
        e.w = 0;
        *reinterpret_cast<uint4*>(entries + at) = e;
      }
    }
  }
}

__global__ __launch_bounds__(kSrBlock) void sorted_replicas_gather(const ReplicaRec* __restrict__ replicas, int R,
                                                                   const unsigned long long* __restrict__ offsets, int n,
                                                                   long long total, int anyLong, int scoreOn,
                                                                   int scoreReverse, const SortEntry* __restrict__ bufA,
                                                                   const SortEntry* __restrict__ bufB,
                                                                   ccmi_swap_replica* __restrict__ records,
                                                                   double* __restrict__ scores) {
  const long long stride = (long long)gridDim.x * kSrBlock;
  for (long long pair = (long long)blockIdx.x * kSrBlock + threadIdx.x; 2 * pair < total; pair += stride) {
    int32_t rec[4] = {-1, -1, -1, -1};
    double sc[2] = {0.0, 0.0};
    const int cnt = 2 * pair + 1 < total ? 2 : 1;
    for (int h = 0; h < cnt; ++h) {
      const long long k = 2 * pair + h;
      const SortEntry* buf = bufA;
      if (anyLong) {
        const int sg = segmentOf(offsets, n, k);
        if (segSortPasses((long long)(offsets[sg + 1] - offsets[sg])) & 1) buf = bufB;
      }
      const uint4 e = *reinterpret_cast<const uint4*>(buf + k);
      const int r = (int)e.z;
      if ((unsigned)r < (unsigned)R) {
        const int4 w = *reinterpret_cast<const int4*>(&replicas[r].broker);  // broker, part, orig, flags
        rec[2 * h] = w.y;
        rec[2 * h + 1] = w.x;
      }
      if (scoreOn) {
        uint32_t u = (uint32_t)(srKeyOf(e) >> 30);
        if (scoreReverse) u = ~u;
        const uint32_t bits = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
        const double v = (double)__int_as_float((int)bits);
        sc[h] = scoreReverse ? -v : v;  // -(double) avg: a reversed zero is -0.0
      }
    }
    if (cnt == 2) {
      *reinterpret_cast<int4*>(records + 2 * pair) = make_int4(rec[0], rec[1], rec[2], rec[3]);
      if (scores) *reinterpret_cast<double2*>(scores + 2 * pair) = make_double2(sc[0], sc[1]);
    } else {
      *reinterpret_cast<int2*>(records + 2 * pair) = make_int2(rec[0], rec[1]);
      if (scores) scores[2 * pair] = sc[0];
    }
  }
}

// First half of a call on stream st: the counts cleared, keys, offsets. The host then reads `state` back.
hipError_t launchSortedReplicasCount(const SrTables& T, const SrQuery& q, int n, uint64_t* keys, int32_t* segOf,
                                     uint32_t* counts, uint32_t* cursor, unsigned long long* state, int* launches,
                                     hipStream_t stream) {
  if (T.R < 1 || T.B < 1 || T.W < 1 || T.W > kMaxW || n < 1 || n > T.B || !T.brokers || !T.replicas || !T.parts ||
      !T.rLoad || !T.rStatic || !T.seg || !keys || !segOf || !counts || !cursor || !state || q.scoreRes < -1 ||
      q.scoreRes > 3 || q.aboveRes < -1 || q.aboveRes > 3 || q.belowRes < -1 || q.belowRes > 3)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const int blocks = std::min(kSrMaxBlocks, (T.R + kSrBlock - 1) / kSrBlock);
  hipLaunchKernelGGL(sorted_replicas_keys, dim3((unsigned)blocks), dim3(kSrBlock), 0, stream, T, q, keys, segOf, counts);
  hipLaunchKernelGGL(sorted_replicas_offsets, dim3(1), dim3(kSrScanBlock), 0, stream, counts, n, state, cursor);
  if (launches) *launches += 2;
  return hipGetLastError();
}

// Second half, when the total fits: scatter, sort, the merge passes a segment longer than a tile needs, gather.
hipError_t launchSortedReplicasFill(const SrTables& T, const SrQuery& q, int n, const uint64_t* keys,
                                    const int32_t* segOf, uint32_t* cursor, const unsigned long long* state,
                                    long long total, long long maxLen, SortEntry* bufA, SortEntry* bufB,
                                    ccmi_swap_replica* records, double* scores, int* launches, hipStream_t stream) {
  if (total < 1 || total > T.R || maxLen < 1 || maxLen > total || n < 1 || !keys || !segOf || !cursor || !state ||
      !bufA || !records || (maxLen > kSegSortTile && !bufB))
    return hipErrorInvalidValue;
  const unsigned long long* offsets = state + 2;
  const int blocks = std::min(kSrMaxBlocks, (T.R + kSrBlock - 1) / kSrBlock);
  hipLaunchKernelGGL(sorted_replicas_scatter, dim3((unsigned)blocks), dim3(kSrBlock), 0, stream, T.R, n, keys, segOf,
                     offsets, cursor, bufA);
  int nl = 1 + launchSegSort<SrLess>(offsets, n, total, maxLen, bufA, bufB, stream);
  const int anyLong = maxLen > kSegSortTile ? 1 : 0;  // a merge pass ran: some segment ended in bufB
  const long long pairs = (total + 1) / 2;
  const int gblocks = (int)std::min<long long>(kSrMaxBlocks, (pairs + kSrBlock - 1) / kSrBlock);
  hipLaunchKernelGGL(sorted_replicas_gather, dim3((unsigned)gblocks), dim3(kSrBlock), 0, stream, T.replicas, T.R,
                     offsets, n, total, anyLong, q.scoreRes >= 0 ? 1 : 0, q.scoreReverse, bufA, anyLong ? bufB : bufA,
                     records, scores);
  nl++;
  if (launches) *launches += nl;
  return hipGetLastError();
}

}  // namespace ccmi
