// gfx950 kernels for the partition load response (ccmi_partition_load): the session's partitions ordered by the
// utilization of their current leader (PartitionLoadRunnable.getResult -> ClusterModel.replicasSortedByUtilization ->
// PartitionLoadState), read from the resident chain tables (rLoad, pLeader) and partition records.
//
// K13 partition_load_keys    : one lane per partition (grid-stride): the leader's LoadVec -> the key of the query's
//                              resource, the selection (topic mask, partition number bounds, some current broker
//                              selected) and one 16-byte entry {key bits, rank bits, p} at index p. A partition left
//                              out gets the all-ones key. Per block: the kept count and, over the kept entries, the OR
//                              of the 96 sort bits and the OR of their complements (a bit varies iff set in both).
//     partition_load_plan    : one lane turns those into the pass list: a 1-bit pass on the left-out flag when anything
//                              was left out (a stable partition = the compaction, in partition order), then one 8-bit
//                              pass per digit of (rank, key) in which some bit varies. A uniform digit gets no pass.
//     partition_load_hist    : per tile of 2,048 entries an LDS histogram of the pass's digit -> counts[digit][tile].
//     partition_load_scan    : one workgroup: exclusive scan of counts in digit-major order, in place.
//     partition_load_scatter : per tile the stable scatter. A wave owns 512 consecutive entries and takes them 64 at a
//                              time in order; the rank of an entry among the wave's equal digits is the wave's running
//                              count (LDS) plus the lanes below it in the ballot-built match mask, so equal digits keep
//                              their order: wave order inside the tile, tile order in the scan.
//     partition_load_gather  : one lane per returned record: entry -> partition -> the four utilizations (recomputed
//                              by the function the key came from, so the key's bits are util[resource]'s) and the
//                              partition's current brokers, the leader first, then the others in slot order; five
//                              16-byte stores per 80-byte record.
// Order: ascending on the 96-bit composite (key bits ^ 0x7fff..., rank ^ sign bit): non-negative doubles order as their
// bit patterns, so the flipped bits give descending keys; the entries start in partition order and every pass is
// stable, which is the last criterion. The launches of a slot past the plan's pass count return at once: the host
// launches the most a query can need (1 + 8 key digits + 4 rank digits when the caller gave ranks) without reading the
// plan back. Ping-pong: pass i reads buffer i & 1.
// Every launch is a kernel boundary on the session stream; no workgroup reads another's writes inside a launch.
// Built with -ffp-contract=off: every expression is the reference's IEEE expression.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ccmi.h"
#include "../engine/devtypes.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kKeysBlock = 256;
constexpr int kKeysMaxBlocks = 1024;
constexpr int kSortBlock = 256;                    // 4 waves
constexpr int kSortWaveItems = kPlSortTile / 4;    // consecutive entries of one wave
constexpr int kSortRounds = kSortWaveItems / 64;   // 64 at a time
constexpr int kScanBlock = 1024;
constexpr uint64_t kKeyFlip = 0x7fffffffffffffffull;

static_assert(sizeof(ccmi_partition_load_record) == 80 && sizeof(PlEntry) == 16, "record sizes");
static_assert(kPlSortTile == kSortBlock * 8 && kSortRounds == 8, "tile shape");

// MetricValues.max() of a replica that is the leader: Math.max(Float.MIN_VALUE, max_i v[i]) (ccmi.h has the argument).
// The choice is made on the bits, so it does not depend on how the kernel treats f32 subnormals in a comparison.
__device__ __forceinline__ double plMax(const Window& w, int W) {
  float mx = w.v[0];
  for (int i = 1; i < W; ++i) mx = w.v[i] > mx ? w.v[i] : mx;
  return __float_as_int(mx) > 0 ? (double)mx : 0x1p-149;  // positive and not zero: at least Float.MIN_VALUE
}

// Load.expectedUtilizationFor(resource, wantMaxLoad, wantAvgLoad) (Load.java:81-95); mode 0 default, 1 max, 2 avg
__device__ __forceinline__ double plTerm(const Window& w, int W, int mode, bool latest) {
  if (mode == 1) return plMax(w, W);
  if (latest && mode == 0) return (double)w.v[0];
  return (double)ldAvg(w, W);
}
__device__ __forceinline__ double plUtil(const LoadVec* L, int res, int mode, int W) {
  if (!L || !L->mask) return 0.0;
  double r = 0;
  switch (res) {
    case R_CPU: r += plTerm(L->m[M_CPU], W, mode, false); break;
    case R_DISK: r += plTerm(L->m[M_DISK], W, mode, true); break;
    case R_NW_IN:
      r += plTerm(L->m[M_LBI], W, mode, false);
      r += plTerm(L->m[M_RBI], W, mode, false);
      break;
    default:
      r += plTerm(L->m[M_LBO], W, mode, false);
      r += plTerm(L->m[M_RBO], W, mode, false);
      break;
  }
  return ldMax0(r);
}

__device__ __forceinline__ const LoadVec* plLeaderLoad(const PlTables& T, int p) {
  const int r = T.pLeader[p];
  return (unsigned)r < (unsigned)T.R ? T.rLoad + r : nullptr;
}

__device__ __forceinline__ uint32_t plDigit(const PlEntry& e, uint32_t off, uint32_t mask) {
  return (off < 32 ? e.rank >> off : (uint32_t)(e.key >> (off - 32))) & mask;
}

__device__ __forceinline__ uint32_t waveOr(uint32_t v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v |= (uint32_t)__shfl_xor((int)v, s, 64);
  return v;
}

}  // namespace

__global__ __launch_bounds__(kKeysBlock) void partition_load_keys(PlTables T, PlQuery q, PlEntry* __restrict__ out,
                                                                  PlState* __restrict__ st) {
  __shared__ uint32_t sh[7];  // or[3] | nand[3] | kept
  if (threadIdx.x < 7) sh[threadIdx.x] = 0;
  __syncthreads();
  uint32_t orB[3] = {0, 0, 0}, nandB[3] = {0, 0, 0}, kept = 0;
  const int stride = gridDim.x * kKeysBlock;
  for (int p = blockIdx.x * kKeysBlock + threadIdx.x; p < T.P; p += stride) {
    const PartitionRec rec = T.parts[p];
    const int number = T.pNumber[p];
    bool keep = number >= q.lower && number <= q.upper;
    if (T.topicSel) keep = keep && (unsigned)rec.topic < (unsigned)T.T && T.topicSel[rec.topic] != 0;
    if (T.brokerSel) {
      bool any = false;
#pragma unroll
      for (int k = 0; k < kMaxRf; ++k)
        any = any || (k < rec.n && (unsigned)rec.brokers[k] < (unsigned)T.B && T.brokerSel[rec.brokers[k]] != 0);
      keep = keep && any;
    }
    PlEntry e;
    e.rank = (uint32_t)(T.tieRank ? T.tieRank[p] : p) ^ 0x80000000u;
    e.p = p;
    e.key = ~0ull;
    if (keep) {
      const double u = plUtil(plLeaderLoad(T, p), q.resource, q.mode, T.W);
      e.key = (uint64_t)__double_as_longlong(u) ^ kKeyFlip;
      const uint32_t lo = (uint32_t)e.key, hi = (uint32_t)(e.key >> 32);
      orB[0] |= e.rank;
      orB[1] |= lo;
      orB[2] |= hi;
      nandB[0] |= ~e.rank;
      nandB[1] |= ~lo;
      nandB[2] |= ~hi;
      kept++;
    }
    *reinterpret_cast<uint4*>(out + p) = *reinterpret_cast<const uint4*>(&e);
  }
  // wave, then workgroup (LDS integer atomics: order-free), then one set of global atomics per workgroup
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    orB[k] = waveOr(orB[k]);
    nandB[k] = waveOr(nandB[k]);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) kept += (uint32_t)__shfl_xor((int)kept, s, 64);
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 3; ++k) {
      atomicOr(&sh[k], orB[k]);
      atomicOr(&sh[3 + k], nandB[k]);
    }
    atomicAdd(&sh[6], kept);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    atomicOr(&st->orBits[threadIdx.x], sh[threadIdx.x]);
    atomicOr(&st->nandBits[threadIdx.x], sh[3 + threadIdx.x]);
  } else if (threadIdx.x == 3) {
    atomicAdd(&st->nKept, sh[6]);
  }
}

__global__ void partition_load_plan(PlState* __restrict__ st, int P, int entries, int withRank) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t nKept = st->nKept;
  st->nRecords = (uint32_t)entries < nKept ? (uint32_t)entries : nKept;
  uint32_t np = 0;
  if (nKept < (uint32_t)P && nKept > 0) {  // the left-out flag: bit 63 of the key, bit 95 of the composite
    st->passOff[np] = 95;
    st->passMask[np] = 1;
    st->passN[np] = (uint32_t)P;
    np++;
  }
  if (nKept > 1)
    for (uint32_t d = withRank ? 0 : 4; d < 12; ++d) {
      const uint32_t off = d * 8;
      const uint32_t varies = st->orBits[off >> 5] & st->nandBits[off >> 5];
      if (((varies >> (off & 31)) & 0xffu) == 0) continue;  // every kept entry has the same digit: no pass
      st->passOff[np] = off;
      st->passMask[np] = 0xff;
      st->passN[np] = nKept;
      np++;
    }
  st->nPass = np;
}

__global__ __launch_bounds__(kSortBlock) void partition_load_hist(const PlState* __restrict__ st, int slot,
                                                                  const PlEntry* __restrict__ bufA,
                                                                  const PlEntry* __restrict__ bufB, int tiles,
                                                                  uint32_t* __restrict__ counts) {
  if ((uint32_t)slot >= st->nPass) return;
  __shared__ uint32_t h[256];
  const uint32_t n = st->passN[slot], off = st->passOff[slot], mask = st->passMask[slot];
  const PlEntry* src = (slot & 1) ? bufB : bufA;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)kPlSortTile;
#pragma unroll
  for (int k = 0; k < kPlSortTile / kSortBlock; ++k) {
    const uint32_t i = base + k * kSortBlock + threadIdx.x;
    if (i < n) {
      PlEntry e;
      *reinterpret_cast<uint4*>(&e) = *reinterpret_cast<const uint4*>(src + i);
      atomicAdd(&h[plDigit(e, off, mask)], 1u);
    }
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];  // a tile past n writes its zeros
}

// exclusive scan of counts[0, 256 * tiles) in place
__global__ __launch_bounds__(kScanBlock) void partition_load_scan(const PlState* __restrict__ st, int slot, int tiles,
                                                                  uint32_t* __restrict__ counts) {
  if ((uint32_t)slot >= st->nPass) return;
  (void)scanCountsInPlace<uint32_t, kScanBlock>(counts, 256 * tiles);
}

__global__ __launch_bounds__(kSortBlock) void partition_load_scatter(const PlState* __restrict__ st, int slot,
                                                                     PlEntry* __restrict__ bufA,
                                                                     PlEntry* __restrict__ bufB, int tiles,
                                                                     const uint32_t* __restrict__ offsets) {
  if ((uint32_t)slot >= st->nPass) return;
  const uint32_t n = st->passN[slot], off = st->passOff[slot], mask = st->passMask[slot];
  const uint32_t base = blockIdx.x * (uint32_t)kPlSortTile;
  if (base >= n) return;
  const PlEntry* src = (slot & 1) ? bufB : bufA;
  PlEntry* dst = (slot & 1) ? bufA : bufB;
  __shared__ uint32_t cnt[4][256];   // a wave's running count per digit, its total afterwards
  __shared__ uint32_t wbase[4][256];  // where a wave's entries of a digit start in dst
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
  __syncthreads();
  PlEntry e[kSortRounds];
  uint32_t dg[kSortRounds], loc[kSortRounds];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kSortRounds; ++k) {
    const uint32_t i = base + wave * kSortWaveItems + k * 64 + lane;
    const bool valid = i < n;
    if (valid) *reinterpret_cast<uint4*>(&e[k]) = *reinterpret_cast<const uint4*>(src + i);
    const uint32_t d = valid ? plDigit(e[k], off, mask) : 0u;
    unsigned long long match = __ballot(valid);  // the valid lanes with this lane's digit
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
    if (valid && before == 0) cnt[wave][d] = old + (uint32_t)__popcll(match);  // the lowest lane of each digit
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

__global__ __launch_bounds__(kKeysBlock) void partition_load_gather(PlTables T, PlQuery q,
                                                                    const PlState* __restrict__ st,
                                                                    const PlEntry* __restrict__ bufA,
                                                                    const PlEntry* __restrict__ bufB,
                                                                    ccmi_partition_load_record* __restrict__ out,
                                                                    int cap) {
  const uint32_t nrec = min(st->nRecords, (uint32_t)cap);
  const PlEntry* src = (st->nPass & 1) ? bufB : bufA;
  const uint32_t stride = gridDim.x * kKeysBlock;
  for (uint32_t i = blockIdx.x * kKeysBlock + threadIdx.x; i < nrec; i += stride) {
    const int p = src[i].p;
    union {
      ccmi_partition_load_record r;
      uint4 q4[5];
    } u;
    if ((unsigned)p < (unsigned)T.P) {
      const PartitionRec rec = T.parts[p];
      const LoadVec* L = plLeaderLoad(T, p);
#pragma unroll
      for (int res = 0; res < 4; ++res) u.r.util[res] = plUtil(L, res, q.mode, T.W);
      u.r.partition = p;
      u.r.num_replicas = rec.n;
      // the leader first, then Partition.followers(): _replicas order without the leader. The leader sits in slot 0
      // unless a goal reordered the slots (moveReplicaToEnd, swapSlots), so its broker comes from its replica record.
      const int lr = T.pLeader[p];
      const int lb = (unsigned)lr < (unsigned)T.R ? T.replicas[lr].broker : rec.brokers[0];
      int at = 0;
#pragma unroll
      for (int k = 0; k < kMaxRf; ++k) at = (k < rec.n && rec.brokers[k] == lb) ? k : at;
      u.r.brokers[0] = lb;
#pragma unroll
      for (int k = 1; k < kMaxRf; ++k)  // slots [0, at) move up by one, the slots behind the leader's stay
        u.r.brokers[k] = k < rec.n ? (k <= at ? rec.brokers[k - 1] : rec.brokers[k]) : -1;
    } else {  // not reachable: every entry carries its own index
      for (int res = 0; res < 4; ++res) u.r.util[res] = 0.0;
      u.r.partition = -1;
      u.r.num_replicas = 0;
      for (int k = 0; k < kMaxRf; ++k) u.r.brokers[k] = -1;
    }
    u.r.reserved[0] = u.r.reserved[1] = 0;
    uint4* d = reinterpret_cast<uint4*>(out + i);
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = u.q4[k];
  }
}

// The whole query on stream st: state cleared, keys, plan, `slots` pass slots, gather of at most cap records.
hipError_t launchPartitionLoad(const PlTables& T, const PlQuery& q, PlState* st, PlEntry* bufA, PlEntry* bufB,
                               uint32_t* counts, int tiles, int slots, ccmi_partition_load_record* out, int cap,
                               int* launches, hipStream_t stream) {
  if (T.P < 1 || T.R < 1 || T.W < 1 || T.W > kMaxW || !T.parts || !T.replicas || !T.rLoad || !T.pLeader ||
      !T.pNumber || !st || !bufA || !bufB || !counts || tiles != (T.P + kPlSortTile - 1) / kPlSortTile || slots < 0 ||
      slots > kPlMaxPasses || cap < 0 || cap > T.P || (cap > 0 && !out) || q.resource < 0 || q.resource > 3 || q.mode < 0 || q.mode > 2)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(st, 0, sizeof(PlState), stream);
  if (e != hipSuccess) return e;
  const int keyBlocks = std::min(kKeysMaxBlocks, (T.P + kKeysBlock - 1) / kKeysBlock);
  hipLaunchKernelGGL(partition_load_keys, dim3((unsigned)keyBlocks), dim3(kKeysBlock), 0, stream, T, q, bufA, st);
  hipLaunchKernelGGL(partition_load_plan, dim3(1), dim3(64), 0, stream, st, T.P, q.entries, T.tieRank ? 1 : 0);
  int n = 2;
  for (int s = 0; s < slots; ++s) {
    hipLaunchKernelGGL(partition_load_hist, dim3((unsigned)tiles), dim3(kSortBlock), 0, stream, st, s, bufA, bufB,
                       tiles, counts);
    hipLaunchKernelGGL(partition_load_scan, dim3(1), dim3(kScanBlock), 0, stream, st, s, tiles, counts);
    hipLaunchKernelGGL(partition_load_scatter, dim3((unsigned)tiles), dim3(kSortBlock), 0, stream, st, s, bufA, bufB,
                       tiles, counts);
    n += 3;
  }
  if (cap > 0) {
    const int blocks = std::min(kKeysMaxBlocks, (cap + kKeysBlock - 1) / kKeysBlock);
    hipLaunchKernelGGL(partition_load_gather, dim3((unsigned)blocks), dim3(kKeysBlock), 0, stream, T, q, st, bufA, bufB,
                       out, cap);
    n++;
  }
  if (launches) *launches = n;
  return hipGetLastError();
}

}  // namespace ccmi
