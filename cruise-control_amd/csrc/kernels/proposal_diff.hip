// gfx950 kernels for the proposal diff (ccmi_proposal_diff): AnalyzerUtils.getDiff (AnalyzerUtils.java:63-93) of the
// resident model against the session's initial placement, the ExecutionProposal sets of ExecutionProposal.java:72-78 and
// the sums of OptimizerResult.getMovementStats (OptimizerResult.java:258-278), read from the partition records, the
// replica records, the slot order and the leaders that the chain tables keep current.
//
// K14 proposal_diff_flags  : grid-stride over tiles of kPdTile partitions, the lanes of a workgroup take a tile 256 at
//                            a time in order. Per partition: its PartitionRec (the current brokers in slot order), the
//                            initial brokers and disks, the leader's replica id and its ReplicaRec -> changed or not,
//                            and its share of the five movement sums. One changed-count per tile; the sums go wave ->
//                            LDS -> one set of 64-bit global integer atomics per workgroup (order-free).
//     proposal_diff_scan   : one workgroup: exclusive scan of the tile counts in place; counts[tiles] and the
//                            summary's proposal count get the total.
//     proposal_diff_gather : per tile with changed partitions below the capacity, "changed" is recomputed; the rank of
//                            a changed partition is the tile's offset + the changed ones of the rounds before it in
//                            the tile + those of the waves before it in the round (LDS) + the lanes below it in the
//                            64-bit ballot mask, so the compaction is stable in partition order. A lane whose rank is
//                            below the capacity writes its 160-byte record with ten 16-byte stores.
// Every launch is a kernel boundary on the session stream; no workgroup reads another's writes inside a launch.
// Integer work only apart from the narrowing of the partition size; no scratch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "ccmi.h"
#include "../engine/devtypes.h"
#include "proposal_row.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kPdBlock = 256;  // 4 waves
constexpr int kPdWaves = kPdBlock / 64;
constexpr int kPdRounds = kPdTile / kPdBlock;
constexpr int kPdMaxBlocks = 1024;
constexpr int kPdScanBlock = 1024;
constexpr int kPdSums = 5;  // inter-broker movements and MB, intra-broker movements and MB, leadership movements

static_assert(sizeof(ccmi_proposal_record) == 160 && sizeof(ccmi_proposal_summary) == 64 && sizeof(PdSums) == 64,
              "record sizes");

}  // namespace

__global__ __launch_bounds__(kPdBlock) void proposal_diff_flags(PdTables T, int tiles, uint32_t* __restrict__ counts,
                                                                PdSums* __restrict__ sums) {
  __shared__ uint32_t tileCnt[kPdWaves];
  __shared__ unsigned long long sh[kPdSums];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x < kPdSums) sh[threadIdx.x] = 0;
  unsigned long long acc[kPdSums] = {0, 0, 0, 0, 0};
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t cnt = 0;
#pragma unroll 1
    for (int k = 0; k < kPdRounds; ++k) {
      const int p = tile * kPdTile + k * kPdBlock + (int)threadIdx.x;
      if (p < T.P) {
        PdRow w;
        pdDiff(T, p, w);
        if (w.changed) {
          cnt++;
          const unsigned long long size = (unsigned long long)(long long)w.size;
          if (w.nAdd > 0 || w.nRemove > 0) {  // getMovementStats' if / else-if / else
            acc[0] += 1;
            acc[1] += (unsigned long long)w.nAdd * size;
          } else if (w.nBetween > 0) {
            acc[2] += (unsigned long long)w.nBetween;
            acc[3] += (unsigned long long)w.nBetween * size;
          } else {
            acc[4] += 1;
          }
        }
      }
    }
    cnt = (uint32_t)waveSum(cnt);
    if (lane == 0) tileCnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t t = 0;
      for (int x = 0; x < kPdWaves; ++x) t += tileCnt[x];
      counts[tile] = t;
    }
    __syncthreads();
  }
  // wave, then workgroup (LDS integer atomics: order-free), then one set of global atomics per workgroup
#pragma unroll
  for (int k = 0; k < kPdSums; ++k) acc[k] = waveSum(acc[k]);
  __syncthreads();  // sh is zeroed (a workgroup without a tile has not passed a barrier yet)
  if (lane == 0)
    for (int k = 0; k < kPdSums; ++k)
      if (acc[k]) atomicAdd(&sh[k], acc[k]);
  __syncthreads();
  if (threadIdx.x < kPdSums && sh[threadIdx.x]) atomicAdd(&sums->v[1 + threadIdx.x], sh[threadIdx.x]);
}

// exclusive scan of counts[0, tiles) in place, counts[tiles] = sums->v[0] = the total
__global__ __launch_bounds__(kPdScanBlock) void proposal_diff_scan(int tiles, uint32_t* __restrict__ counts,
                                                                   PdSums* __restrict__ sums) {
  const uint32_t total = scanCountsInPlace<uint32_t, kPdScanBlock>(counts, tiles);
  if (threadIdx.x == kPdScanBlock - 1) {
    counts[tiles] = total;
    sums->v[0] = total;
  }
}

__global__ __launch_bounds__(kPdBlock) void proposal_diff_gather(PdTables T, int tiles,
                                                                 const uint32_t* __restrict__ offsets,
                                                                 ccmi_proposal_record* __restrict__ out, int cap) {
  __shared__ uint32_t waveCnt[kPdWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // the same for every lane of the workgroup: a tile without changed partitions, or with all of them past the capacity
    const uint32_t first = offsets[tile], end = offsets[tile + 1];
    if (first == end || first >= (uint32_t)cap) continue;
    uint32_t run = first;  // the changed partitions of the tile's earlier rounds are ranked below this one's
#pragma unroll 1
    for (int k = 0; k < kPdRounds; ++k) {
      const int p = tile * kPdTile + k * kPdBlock + (int)threadIdx.x;
      PdRow w;
      w.changed = false;
      if (p < T.P) pdDiff(T, p, w);
      const unsigned long long mask = __ballot(w.changed);
      if (lane == 0) waveCnt[wave] = (uint32_t)__popcll(mask);
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int x = 0; x < kPdWaves; ++x) {
        before += x < wave ? waveCnt[x] : 0u;
        total += waveCnt[x];
      }
      const uint32_t rank = run + before + (uint32_t)__popcll(mask & below);
      if (w.changed && rank < (uint32_t)cap) {
        union {
          ccmi_proposal_record r;
          uint4 q4[10];
        } u;
        u.r.partition = p;
        u.r.size = w.size;
        u.r.old_leader = w.oldLeader;
        u.r.old_leader_disk = w.oldLeaderDisk;
        u.r.num_replicas = w.n;
        u.r.flags = w.flags;
        u.r.num_to_add = w.nAdd;
        u.r.num_between_disks = w.nBetween;
#pragma unroll
        for (int x = 0; x < kMaxRf; ++x) {
          u.r.old_replicas[x] = w.oldR[x];
          u.r.new_replicas[x] = w.newR[x];
          u.r.old_disks[x] = w.oldD[x];
          u.r.new_disks[x] = w.newD[x];
        }
        uint4* d = reinterpret_cast<uint4*>(out + rank);
#pragma unroll
        for (int x = 0; x < 10; ++x) d[x] = u.q4[x];
      }
      run += total;
      __syncthreads();  // waveCnt is rewritten in the next round
    }
  }
}

// The whole call on stream st: sums cleared, flags, scan, and the gather of at most cap records.
hipError_t launchProposalDiff(const PdTables& T, uint32_t* counts, int tiles, PdSums* sums, ccmi_proposal_record* out,
                              int cap, int* launches, hipStream_t stream) {
  const bool anyDisk = T.initDisks || T.initLeaderDisks || T.curDisks;
  const bool allDisks = T.initDisks && T.initLeaderDisks && T.curDisks;
  if (T.P < 1 || T.R < 1 || !T.parts || !T.replicas || !T.pOff || !T.pSlots || !T.pLeader || !T.initDist ||
      !T.initLeaders || (anyDisk && !allDisks) || !counts || !sums || tiles != (T.P + kPdTile - 1) / kPdTile || cap < 0 ||
      cap > T.P || (cap > 0 && !out))
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(PdSums), stream);
  if (e != hipSuccess) return e;
  const int blocks = std::min(kPdMaxBlocks, tiles);
  hipLaunchKernelGGL(proposal_diff_flags, dim3((unsigned)blocks), dim3(kPdBlock), 0, stream, T, tiles, counts, sums);
  hipLaunchKernelGGL(proposal_diff_scan, dim3(1), dim3(kPdScanBlock), 0, stream, tiles, counts, sums);
  int n = 2;
  if (cap > 0) {
    hipLaunchKernelGGL(proposal_diff_gather, dim3((unsigned)blocks), dim3(kPdBlock), 0, stream, T, tiles, counts, out,
                       cap);
    n++;
  }
  if (launches) *launches = n;
  return hipGetLastError();
}

}  // namespace ccmi
