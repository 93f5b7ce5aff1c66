// gfx950 kernels for ccmi_sorted_replicas: per asked broker the list a freshly initialised SortedReplicas would iterate
// (SortedReplicas.java:75-90, ReplicaSortFunctionFactory, Replica.compareTo), built from the resident tables: the
// replica, broker and partition records, the Java loads (rLoad) and the static rank of Replica.compareTo's tail.
//
// K15 sorted_replicas_keys    : one lane per replica (grid-stride): the replica's current broker -> its segment
//                               (seg[B], -1 = not asked for), the selections of Model::selects, the score recomputed
//                               from rLoad the way LoadOps::groupAvg does (ldZero / ldAdd / ldAvg; an empty load
//                               scores 0) and the 64-bit key; writes key[r] (all ones = not selected) and segOf[r],
//                               and counts per segment: the lanes of a wave that share a segment add once.
//     sorted_replicas_offsets : one workgroup: the exclusive scan of the n counts into the int64 offsets (a thread sums
//                               a contiguous chunk, so n may exceed the block), the total, the longest segment, and the
//                               scatter cursors cleared.
//     sorted_replicas_scatter : one lane per replica: a selected replica's {key, replica id} goes to
//                               offsets[seg] + its rank among the segment's arrivals (wave-aggregated cursor). The slot
//                               order inside a segment is whatever the atomics give; the keys are unique (rStatic is a
//                               dense rank of a tuple no two replicas share), so the sort alone fixes the result.
//     sorted_replicas_sort    : one workgroup per segment. A segment of up to kSrSortTile entries is loaded into LDS
//                               with 16-byte accesses, padded to its next power of two with all-ones keys, sorted by a
//                               bitonic network of that width (a 100-entry segment runs the 128-wide network, not the
//                               tile's) and written back. When the call's longest segment (read back with the offsets)
//                               is at most 256 entries the launcher takes the instance with a 4 KB image and 128
//                               lanes, so the common case does not reserve the tile's 64 KB per workgroup either. A
//                               longer segment is sorted tile by tile here and finished by
//     sorted_replicas_merge   : the fallback for segments longer than a tile: global-memory merge passes over the sorted
//                               tiles, run width doubling per launch, ping-pong between two entry buffers. One lane per
//                               entry finds its rank in the sibling run by binary search. Chosen over radix passes
//                               because the tiles come sorted out of the LDS network anyway, segment boundaries stay
//                               where they are (a radix pass over the whole array would need per-segment histograms),
//                               and the host launches it only when the offsets it reads back show such a segment: the
//                               common case pays nothing. A segment of length len ends in buffer (passes(len) & 1) with
//                               passes(len) = the number of widths kSrSortTile << i below len; shorter ones are skipped.
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

namespace ccmi {

namespace {

constexpr int kSrBlock = 256;
constexpr int kSrMaxBlocks = 1024;
constexpr int kSrScanBlock = 1024;
constexpr int kSrSmallTile = 256;   // the LDS image of a call whose longest segment fits it: 4 KB
constexpr int kSrSmallBlock = 128;  // and its workgroup: one compare-exchange per lane at the full width

static_assert(sizeof(ccmi_swap_replica) == 8 && sizeof(SrEntry) == 16, "record sizes");
static_assert((kSrSortTile & (kSrSortTile - 1)) == 0 && kSrSortTile * sizeof(SrEntry) <= 64 * 1024, "tile shape");

// The lanes of a wave with `active` set add one each to counters[seg]: one atomic per distinct segment in the wave.
// Returns the lane's slot among the counter's arrivals. Every lane of the wave calls it (the loop is wave-uniform).
__device__ __forceinline__ uint32_t waveSegAdd(uint32_t* __restrict__ counters, int seg, bool active) {
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long todo = __ballot(active);
  uint32_t slot = 0;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int s = __shfl(seg, leader, 64);
    const bool mine = active && seg == s;
    const unsigned long long m = __ballot(mine);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&counters[s], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (mine) slot = base + (uint32_t)__popcll(m & below);
    todo &= ~m;
  }
  return slot;
}

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
__device__ __forceinline__ bool srLess(const uint4& a, const uint4& b) {
  const uint64_t ka = srKeyOf(a), kb = srKeyOf(b);
  return ka != kb ? ka < kb : a.z < b.z;
}

// the segment of entry k: the last i with offsets[i] <= k (empty segments repeat an offset and are skipped)
__device__ __forceinline__ int srSegmentOf(const long long* __restrict__ offsets, int n, long long k) {
  int lo = 0, hi = n;  // invariant: offsets[lo] <= k < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int srPasses(long long len) {
  int p = 0;
  for (long long w = kSrSortTile; w < len; w <<= 1) p++;
  return p;
}

}  // namespace

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
  __shared__ unsigned long long s[2][kSrScanBlock];
  __shared__ uint32_t mx;
  if (threadIdx.x == 0) mx = 0;
  const int chunk = (n + kSrScanBlock - 1) / kSrScanBlock;
  const int i0 = min(n, (int)threadIdx.x * chunk), i1 = min(n, i0 + chunk);
  unsigned long long sum = 0;
  uint32_t longest = 0;
  for (int i = i0; i < i1; ++i) {
    const uint32_t c = counts[i];
    sum += c;
    longest = c > longest ? c : longest;
    cursor[i] = 0;
  }
  int cur = 0;
  s[0][threadIdx.x] = sum;
  __syncthreads();
  if (longest) atomicMax(&mx, longest);
  for (int d = 1; d < kSrScanBlock; d <<= 1) {
    const unsigned long long v = s[cur][threadIdx.x] + ((int)threadIdx.x >= d ? s[cur][threadIdx.x - d] : 0ull);
    s[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  unsigned long long run = s[cur][threadIdx.x] - sum;  // exclusive
  for (int i = i0; i < i1; ++i) {
    state[2 + i] = run;
    run += counts[i];
  }
  if (threadIdx.x == kSrScanBlock - 1) {
    state[0] = s[cur][threadIdx.x];
    state[2 + n] = s[cur][threadIdx.x];
  }
  if (threadIdx.x == 0) state[1] = mx;  // every atomicMax came before the scan's barriers
}

__global__ __launch_bounds__(kSrBlock) void sorted_replicas_scatter(int R, int n, const uint64_t* __restrict__ keys,
                                                                    const int32_t* __restrict__ segOf,
                                                                    const unsigned long long* __restrict__ offsets,
                                                                    uint32_t* __restrict__ cursor,
                                                                    SrEntry* __restrict__ entries) {
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
        uint4 e;
        e.x = (uint32_t)key;
        e.y = (uint32_t)(key >> 32);
        e.z = (uint32_t)r;
        e.w = 0;
        *reinterpret_cast<uint4*>(entries + at) = e;
      }
    }
  }
}

// kLds: the entries of the workgroup's LDS image. The launcher picks kSrSmallTile when the longest segment of the call
// fits it (more workgroups per CU), else the whole tile; the tile stride of a longer segment is kSrSortTile either way.
template <int kLds>
__global__ __launch_bounds__(kSrBlock) void sorted_replicas_sort(const unsigned long long* __restrict__ offsets,
                                                                 SrEntry* __restrict__ entries) {
  __shared__ uint4 tile[kLds];
  const unsigned long long off0 = offsets[blockIdx.x];
  const long long len = (long long)(offsets[blockIdx.x + 1] - off0);
  if (len < 2) return;
  for (long long t0 = 0; t0 < len; t0 += kSrSortTile) {  // one tile unless the segment is longer than a tile
    const int m = (int)min((long long)kSrSortTile, len - t0);
    if (m > kLds) return;  // not reachable: the launcher chose kLds from the longest segment
    uint4* seg = reinterpret_cast<uint4*>(entries + off0 + t0);
    int width = 2;
    while (width < m) width <<= 1;
    for (int i = (int)threadIdx.x; i < width; i += (int)blockDim.x)
      tile[i] = i < m ? seg[i] : make_uint4(~0u, ~0u, ~0u, ~0u);
    __syncthreads();
    const int half = width >> 1;
    for (int k = 2; k <= width; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = (int)threadIdx.x; t < half; t += (int)blockDim.x) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int p = i | j;
          const uint4 a = tile[i], b = tile[p];
          const bool up = (i & k) == 0;
          if (srLess(b, a) == up) {
            tile[i] = b;
            tile[p] = a;
          }
        }
        __syncthreads();
      }
    for (int i = (int)threadIdx.x; i < m; i += (int)blockDim.x) seg[i] = tile[i];
    __syncthreads();
  }
}

// pass `pass` merges runs of width kSrSortTile << pass; it reads buffer (pass & 1) and writes the other
__global__ __launch_bounds__(kSrBlock) void sorted_replicas_merge(const unsigned long long* __restrict__ offsets, int n,
                                                                  long long total, int pass,
                                                                  SrEntry* __restrict__ bufA,
                                                                  SrEntry* __restrict__ bufB) {
  const long long w = (long long)kSrSortTile << pass;
  const uint4* src = reinterpret_cast<const uint4*>((pass & 1) ? bufB : bufA);
  uint4* dst = reinterpret_cast<uint4*>((pass & 1) ? bufA : bufB);
  const long long stride = (long long)gridDim.x * kSrBlock;
  for (long long k = (long long)blockIdx.x * kSrBlock + threadIdx.x; k < total; k += stride) {
    const int sg = srSegmentOf(reinterpret_cast<const long long*>(offsets), n, k);
    const long long off = (long long)offsets[sg], len = (long long)offsets[sg + 1] - off;
    if (len <= w) continue;  // sorted already; stays in the buffer of its last pass
    const long long j = k - off;
    const long long L = j / (2 * w) * (2 * w);
    const long long mid = min(L + w, len), end = min(L + 2 * w, len);
    const uint4 e = src[k];
    long long rank;
    if (j < mid) {  // left run: the entries before it, plus the right run's entries below it
      long long lo = mid, hi = end;
      while (lo < hi) {
        const long long c = (lo + hi) >> 1;
        if (srLess(src[off + c], e))
          lo = c + 1;
        else
          hi = c;
      }
      rank = (j - L) + (lo - mid);
    } else {  // right run (keys are unique: no tie to break)
      long long lo = L, hi = mid;
      while (lo < hi) {
        const long long c = (lo + hi) >> 1;
        if (srLess(src[off + c], e))
          lo = c + 1;
        else
          hi = c;
      }
      rank = (j - mid) + (lo - L);
    }
    dst[off + L + rank] = e;  // L + rank < end <= len
  }
}

__global__ __launch_bounds__(kSrBlock) void sorted_replicas_gather(const ReplicaRec* __restrict__ replicas, int R,
                                                                   const unsigned long long* __restrict__ offsets, int n,
                                                                   long long total, int anyLong, int scoreOn,
                                                                   int scoreReverse, const SrEntry* __restrict__ bufA,
                                                                   const SrEntry* __restrict__ bufB,
                                                                   ccmi_swap_replica* __restrict__ records,
                                                                   double* __restrict__ scores) {
  const long long stride = (long long)gridDim.x * kSrBlock;
  for (long long pair = (long long)blockIdx.x * kSrBlock + threadIdx.x; 2 * pair < total; pair += stride) {
    int32_t rec[4] = {-1, -1, -1, -1};
    double sc[2] = {0.0, 0.0};
    const int cnt = 2 * pair + 1 < total ? 2 : 1;
    for (int h = 0; h < cnt; ++h) {
      const long long k = 2 * pair + h;
      const SrEntry* buf = bufA;
      if (anyLong) {
        const int sg = srSegmentOf(reinterpret_cast<const long long*>(offsets), n, k);
        if (srPasses((long long)(offsets[sg + 1] - offsets[sg])) & 1) buf = bufB;
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
                                    long long total, long long maxLen, SrEntry* bufA, SrEntry* bufB,
                                    ccmi_swap_replica* records, double* scores, int* launches, hipStream_t stream) {
  if (total < 1 || total > T.R || maxLen < 1 || maxLen > total || n < 1 || !keys || !segOf || !cursor || !state ||
      !bufA || !records || (maxLen > kSrSortTile && !bufB))
    return hipErrorInvalidValue;
  const unsigned long long* offsets = state + 2;
  const int blocks = std::min(kSrMaxBlocks, (T.R + kSrBlock - 1) / kSrBlock);
  hipLaunchKernelGGL(sorted_replicas_scatter, dim3((unsigned)blocks), dim3(kSrBlock), 0, stream, T.R, n, keys, segOf,
                     offsets, cursor, bufA);
  if (maxLen <= kSrSmallTile)
    hipLaunchKernelGGL(sorted_replicas_sort<kSrSmallTile>, dim3((unsigned)n), dim3(kSrSmallBlock), 0, stream, offsets,
                       bufA);
  else
    hipLaunchKernelGGL(sorted_replicas_sort<kSrSortTile>, dim3((unsigned)n), dim3(kSrBlock), 0, stream, offsets, bufA);
  int nl = 2;
  const int eblocks = (int)std::min<long long>(kSrMaxBlocks, (total + kSrBlock - 1) / kSrBlock);
  int pass = 0;
  for (long long w = kSrSortTile; w < maxLen; w <<= 1, ++pass) {
    hipLaunchKernelGGL(sorted_replicas_merge, dim3((unsigned)eblocks), dim3(kSrBlock), 0, stream, offsets, n, total,
                       pass, bufA, bufB);
    nl++;
  }
  const long long pairs = (total + 1) / 2;
  const int gblocks = (int)std::min<long long>(kSrMaxBlocks, (pairs + kSrBlock - 1) / kSrBlock);
  hipLaunchKernelGGL(sorted_replicas_gather, dim3((unsigned)gblocks), dim3(kSrBlock), 0, stream, T.replicas, T.R,
                     offsets, n, total, pass > 0 ? 1 : 0, q.scoreRes >= 0 ? 1 : 0, q.scoreReverse, bufA,
                     pass > 0 ? bufB : bufA, records, scores);
  nl++;
  if (launches) *launches += nl;
  return hipGetLastError();
}

}  // namespace ccmi
