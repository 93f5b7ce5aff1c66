// gfx950 kernels for ccmi_execution_plan: what ExecutionTaskPlanner.addExecutionProposals (ExecutionTaskPlanner.java:
// 137-273) builds from the proposals of the resident model (the proposals of ccmi_proposal_diff, recomputed per partition
// by the same pdDiff): the inter-broker tasks in execution-id order, per broker the TreeSet of its inter-broker tasks
// under the ReplicaMovementStrategy chain (AbstractReplicaMovementStrategy.java:28-85), the initial broker order of
// brokerComparator (:518-539), per broker its intra-broker tasks, and the leadership tasks.
//
// K16 execution_plan_classify : tiles of kPdTile partitions, as K14's flags. Per partition pdDiff -> an EpRow (task kinds,
//                               num_to_add, between-disk count, the old leader, dataToMoveInMB), per tile the number of
//                               inter-broker and of leadership tasks, per broker the number of inter-broker and of
//                               intra-broker list entries (the lanes of a wave that share a broker add once), and the
//                               summary sums (wave -> LDS -> one set of 64-bit atomics per workgroup).
//     execution_plan_scan     : four independent workgroups: the exclusive scans of the two tile-count arrays, and
//                               segmentOffsets (segments.h) on the two per-broker count arrays: offsets, totals and
//                               longest segments, cursors cleared. When any intra-broker task exists the inter-broker
//                               lists are empty (maybeDropReplicaSwapTasks): their counts read as zero.
//     execution_plan_number   : the task partitions compacted in partition order (ballot ranks, as K14's gather) into
//                               {rank, partition} keys, for the inter-broker and the leadership tasks. With a
//                               proposal_rank the two lists are then sorted as one segment each by the sort below.
//     execution_plan_ids      : entry i of the numbered list -> idOf[partition] = i and ccmi_plan_task i (one 16-byte
//                               store); the leadership list -> partition indices.
//     execution_plan_scatter  : per partition with tasks, pdDiff again for its brokers; an inter-broker task's key (the
//                               chain's fields most significant first, ending in the execution id) goes to the segments
//                               of the old leader and of every added broker, an intra-broker task's {rank, partition}
//                               key to the segment of its broker (wave-aggregated cursors).
//     launchSegSort           : the shared segmented sort (segments.h) under EpLess, once per list: an LDS bitonic
//                               sort per segment and, for a segment longer than kSegSortTile, merge passes into the
//                               second buffer; a segment of length len ends in buffer (segSortPasses(len) & 1).
//     execution_plan_order    : one lane per broker: its rank among the brokers with tasks under (first task's key, the
//                               longer list, the smaller index) by counting the tuples below its own, staged through
//                               LDS 256 at a time. The tuples are distinct, so the ranks are a permutation.
//     execution_plan_gather   : four entries per lane -> execution ids / partition indices, one 16-byte store.
// Every launch is a kernel boundary on the session stream; no workgroup reads another's writes inside a launch; nothing
// spins or waits on another workgroup. Integer work only.
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

constexpr int kEpBlock = 256;  // 4 waves
constexpr int kEpWaves = kEpBlock / 64;
constexpr int kEpRounds = kPdTile / kEpBlock;
constexpr int kEpMaxBlocks = 1024;
constexpr int kEpScanBlock = 1024;
constexpr int kEpSums = 6;

static_assert(sizeof(ccmi_plan_task) == 16 && sizeof(ccmi_plan_summary) == 64 && sizeof(EpSums) == 64, "record sizes");

// slot k of the new replicas: a replica to add (its broker is no old broker), or one to move between disks (an old
// broker, a new (broker, disk) pair): ExecutionProposal.java:74, :76-78
__device__ __forceinline__ void epSlotKind(const PdRow& w, int k, bool& added, bool& between) {
  bool brokerInOld = false, pairInOld = false;
#pragma unroll
  for (int j = 0; j < kMaxRf; ++j) {
    const bool inj = j < w.n;
    brokerInOld = brokerInOld || (inj && w.newR[k] == w.oldR[j]);
    pairInOld = pairInOld || (inj && w.newR[k] == w.oldR[j] && w.newD[k] == w.oldD[j]);
  }
  added = k < w.n && !brokerInOld;
  between = k < w.n && brokerInOld && !pairInOld;
}

// {proposal_rank, partition}: the order of the caller's collection, ties and a NULL rank by partition index
__device__ __forceinline__ uint64_t epOrderKey(const int32_t* __restrict__ rank, int p) {
  const uint32_t r = rank ? (uint32_t)rank[p] ^ 0x80000000u : 0u;
  return ((uint64_t)r << 32) | (uint32_t)p;
}

__device__ __forceinline__ void epPush(uint64_t& hi, uint64_t& lo, int bits, uint64_t v) {
  if (bits >= 64) {
    hi = lo;
    lo = v;
  } else {
    hi = (hi << bits) | (lo >> (64 - bits));
    lo = (lo << bits) | v;
  }
}

// The chain's comparators as one key, most significant first (at most 3 * 2 + 64 + 31 bits). The class tables:
// PostponeUrpReplicaMovementStrategy.java:47-50 (not under-replicated first), PrioritizeMinIsrWithOfflineReplicasStrategy
// .java:46-53 (under min-ISR, then at min-ISR, then the rest), PrioritizeOneAboveMinIsrWithOfflineReplicasStrategy.java:
// 44-49 (one above min-ISR first); the size comparators on the int64 value, descending or ascending; BASE last.
__device__ __forceinline__ SortEntry epTaskKey(const EpQuery& q, uint32_t st, int64_t data, uint32_t id) {
  uint64_t hi = 0, lo = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= q.n) break;
    const uint64_t biased = (uint64_t)data ^ 0x8000000000000000ull;
    switch (q.strat[i]) {
      case CCMI_STRATEGY_PRIORITIZE_LARGE: epPush(hi, lo, 64, ~biased); break;
      case CCMI_STRATEGY_PRIORITIZE_SMALL: epPush(hi, lo, 64, biased); break;
      case CCMI_STRATEGY_POSTPONE_URP: epPush(hi, lo, 2, (st & CCMI_PSTATE_UNDER_REPLICATED) ? 1 : 0); break;
      case CCMI_STRATEGY_PRIORITIZE_MIN_ISR_WITH_OFFLINE:
        epPush(hi, lo, 2, (st & CCMI_PSTATE_UNDER_MIN_ISR) ? 0 : (st & CCMI_PSTATE_AT_MIN_ISR) ? 1 : 2);
        break;
      case CCMI_STRATEGY_PRIORITIZE_ONE_ABOVE_MIN_ISR_WITH_OFFLINE:
        epPush(hi, lo, 2, (st & CCMI_PSTATE_ONE_ABOVE_MIN_ISR) ? 0 : 1);
        break;
      default: break;
    }
  }
  epPush(hi, lo, 31, id & 0x7fffffffu);
  SortEntry e;
  e.lo = lo;
  e.hi = hi;
  return e;
}

// a broker's list length and, when it has one, its first task's key (the sorted segment is in buffer segSortPasses(len) & 1)
__device__ __forceinline__ uint32_t epHeadLen(const unsigned long long* __restrict__ offsets, int B, int b) {
  return b < B ? (uint32_t)(offsets[b + 1] - offsets[b]) : 0u;
}
__device__ __forceinline__ uint4 epHeadKey(const unsigned long long* __restrict__ offsets, int b, uint32_t len,
                                           const SortEntry* __restrict__ bufA, const SortEntry* __restrict__ bufB) {
  if (len == 0) return make_uint4(0, 0, 0, 0);
  return *reinterpret_cast<const uint4*>(((segSortPasses((long long)len) & 1) ? bufB : bufA) + offsets[b]);
}

}  // namespace

// the order of every list: the 128-bit key, hi then lo (an entry as a uint4: x, y = lo; z, w = hi)
struct EpLess {
  static __device__ __forceinline__ bool less(const uint4& a, const uint4& b) {
    const uint64_t ah = ((uint64_t)a.w << 32) | a.z, bh = ((uint64_t)b.w << 32) | b.z;
    if (ah != bh) return ah < bh;
    return (((uint64_t)a.y << 32) | a.x) < (((uint64_t)b.y << 32) | b.x);
  }
};

__global__ __launch_bounds__(kEpBlock) void execution_plan_classify(EpTables T, int tiles, EpRow* __restrict__ rows,
                                                                    uint32_t* __restrict__ tileInter,
                                                                    uint32_t* __restrict__ tileLeader,
                                                                    uint32_t* __restrict__ interCnt,
                                                                    uint32_t* __restrict__ intraCnt,
                                                                    EpSums* __restrict__ sums) {
  __shared__ uint32_t tileCnt[2][kEpWaves];
  __shared__ unsigned long long sh[kEpSums];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x < kEpSums) sh[threadIdx.x] = 0;
  unsigned long long acc[kEpSums] = {0, 0, 0, 0, 0, 0};
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t cntI = 0, cntL = 0;
#pragma unroll 1
    for (int k = 0; k < kEpRounds; ++k) {  // every lane runs every round: the wave-aggregated adds need the whole wave
      const int p = tile * kPdTile + k * kEpBlock + (int)threadIdx.x;
      PdRow w = {};
      bool inter = false;
      if (p < T.pd.P) {
        pdDiff(T.pd, p, w);
        EpRow row;
        row.flags = 0;
        row.src = -1;
        row.data = 0;
        if (w.changed) {
          // isInterBrokerMovementCompleted (ExecutionProposal.java:120-122) with the cluster at the initial placement
          // and every replica in sync: the new broker list equals the old one as a sequence
#pragma unroll
          for (int x = 0; x < kMaxRf; ++x) inter = inter || (x < w.n && w.newR[x] != w.oldR[x]);
          // maybeAddLeaderChangeTasks (:262-264): hasLeaderAction and the current leader is not the new one by broker
          const bool leader = (w.flags & 2) && w.oldLeader != w.newR[0];
          row.data = (long long)(w.nAdd + w.nBetween) * (long long)w.size;
          row.src = w.oldLeader;
          row.flags = (inter ? EP_INTER : 0) | (leader ? EP_LEADER : 0) | (w.nAdd << 8) | (w.nBetween << 12);
          if (inter) {
            cntI++;
            acc[0] += 1;
            acc[4] += row.data > (long long)INT32_MAX ? 1 : 0;
            acc[5] += w.nAdd > 0 ? 1 : 0;
          }
          if (leader) {
            cntL++;
            acc[3] += 1;
          }
          acc[2] += (unsigned long long)w.nBetween;
        }
        rows[p] = row;
      }
      // the list entries: the old leader and every added broker (applyStrategy, AbstractReplicaMovementStrategy.java:
      // 69, :76), and the broker of every between-disk move (:245-246)
      {
        const int b = inter ? w.oldLeader : -1;
        const bool ok = (unsigned)b < (unsigned)T.B;
        (void)waveSegAdd(interCnt, b, ok);
        acc[1] += ok ? 1 : 0;
      }
#pragma unroll
      for (int x = 0; x < kMaxRf; ++x) {
        bool added, between;
        epSlotKind(w, x, added, between);
        const int b = w.newR[x];
        const bool inRange = (unsigned)b < (unsigned)T.B;
        const bool okA = w.changed && inter && added && inRange;
        (void)waveSegAdd(interCnt, b, okA);
        acc[1] += okA ? 1 : 0;
        (void)waveSegAdd(intraCnt, b, w.changed && between && inRange);
      }
    }
    cntI = (uint32_t)waveSum(cntI);
    cntL = (uint32_t)waveSum(cntL);
    if (lane == 0) {
      tileCnt[0][wave] = cntI;
      tileCnt[1][wave] = cntL;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      uint32_t t = 0;
      for (int x = 0; x < kEpWaves; ++x) t += tileCnt[threadIdx.x][x];
      (threadIdx.x == 0 ? tileInter : tileLeader)[tile] = t;
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kEpSums; ++k) acc[k] = waveSum(acc[k]);
  __syncthreads();  // sh is zeroed (a workgroup without a tile has not passed a barrier yet)
  if (lane == 0)
    for (int k = 0; k < kEpSums; ++k)
      if (acc[k]) atomicAdd(&sh[k], acc[k]);
  __syncthreads();
  if (threadIdx.x < kEpSums && sh[threadIdx.x]) atomicAdd(&sums->v[threadIdx.x], sh[threadIdx.x]);
}

// state: two segment blocks of B + 3 words {total, longest, offsets[B + 1]} (inter, intra), then {0, inter-broker tasks}
// and {0, leadership tasks}: the offsets of the two numbered lists as one segment each.
// Workgroup 0 / 1: the tile counts of the inter-broker / leadership tasks, scanned in place, counts[tiles] = the total.
// Workgroup 2 / 3: the per-broker counts of the inter / intra lists.
__global__ __launch_bounds__(kEpScanBlock) void execution_plan_scan(int tiles, uint32_t* __restrict__ tileInter,
                                                                    uint32_t* __restrict__ tileLeader, int B,
                                                                    const uint32_t* __restrict__ interCnt,
                                                                    const uint32_t* __restrict__ intraCnt,
                                                                    uint32_t* __restrict__ cursors,
                                                                    const EpSums* __restrict__ sums,
                                                                    unsigned long long* __restrict__ state) {
  const bool dropped = sums->v[2] > 0;  // maybeDropReplicaSwapTasks
  if (blockIdx.x < 2) {
    uint32_t* counts = blockIdx.x == 0 ? tileInter : tileLeader;
    const unsigned long long total = scanCountsInPlace<unsigned long long, kEpScanBlock>(counts, tiles);
    if (threadIdx.x == 0) {
      counts[tiles] = (uint32_t)total;
      unsigned long long* off = state + 2 * ((size_t)B + 3) + 2 * blockIdx.x;
      off[0] = 0;
      off[1] = blockIdx.x == 0 && dropped ? 0ull : total;
    }
    return;
  }
  if (blockIdx.x > 3) return;
  const int list = (int)blockIdx.x - 2;
  segmentOffsets<kEpScanBlock>(list == 0 ? interCnt : intraCnt, B, list == 0 && dropped,
                               state + (size_t)list * ((size_t)B + 3), cursors + (size_t)list * B);
}

// The task partitions in partition order: entry rank = the tile's offset + the tasks of the tile's earlier rounds + those
// of the waves before it in the round + the lanes below it in the ballot. list 0: inter-broker tasks, 1: leadership.
__global__ __launch_bounds__(kEpBlock) void execution_plan_number(int P, int tiles, const EpRow* __restrict__ rows,
                                                                  const int32_t* __restrict__ rank,
                                                                  const uint32_t* __restrict__ tileInter,
                                                                  const uint32_t* __restrict__ tileLeader, int doInter,
                                                                  SortEntry* __restrict__ interList,
                                                                  SortEntry* __restrict__ leaderList) {
  __shared__ uint32_t waveCnt[2][kEpWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t firstI = tileInter[tile], endI = tileInter[tile + 1];
    const uint32_t firstL = tileLeader[tile], endL = tileLeader[tile + 1];
    if ((firstI == endI || !doInter) && firstL == endL) continue;  // the same for every lane of the workgroup
    uint32_t runI = firstI, runL = firstL;
#pragma unroll 1
    for (int k = 0; k < kEpRounds; ++k) {
      const int p = tile * kPdTile + k * kEpBlock + (int)threadIdx.x;
      const int flags = p < P ? rows[p].flags : 0;
      const bool isI = doInter && (flags & EP_INTER), isL = (flags & EP_LEADER) != 0;
      const unsigned long long mI = __ballot(isI), mL = __ballot(isL);
      if (lane == 0) {
        waveCnt[0][wave] = (uint32_t)__popcll(mI);
        waveCnt[1][wave] = (uint32_t)__popcll(mL);
      }
      __syncthreads();
      uint32_t beforeI = 0, totalI = 0, beforeL = 0, totalL = 0;
#pragma unroll
      for (int x = 0; x < kEpWaves; ++x) {
        beforeI += x < wave ? waveCnt[0][x] : 0u;
        totalI += waveCnt[0][x];
        beforeL += x < wave ? waveCnt[1][x] : 0u;
        totalL += waveCnt[1][x];
      }
      if (isI || isL) {
        SortEntry e;
        e.hi = 0;
        e.lo = epOrderKey(rank, p);
        const uint32_t ri = runI + beforeI + (uint32_t)__popcll(mI & below);
        const uint32_t rl = runL + beforeL + (uint32_t)__popcll(mL & below);
        if (isI && ri < endI) interList[ri] = e;
        if (isL && rl < endL) leaderList[rl] = e;
      }
      runI += totalI;
      runL += totalL;
      __syncthreads();  // waveCnt is rewritten in the next round
    }
  }
}

__global__ __launch_bounds__(kEpBlock) void execution_plan_ids(int P, const EpRow* __restrict__ rows, long long numInter,
                                                               const SortEntry* __restrict__ interList,
                                                               long long numLeader,
                                                               const SortEntry* __restrict__ leaderList,
                                                               int32_t* __restrict__ idOf,
                                                               ccmi_plan_task* __restrict__ tasks,
                                                               int32_t* __restrict__ leaderOut) {
  const long long stride = (long long)gridDim.x * kEpBlock;
  for (long long i = (long long)blockIdx.x * kEpBlock + threadIdx.x; i < numInter + numLeader; i += stride) {
    if (i < numInter) {
      const int p = (int)(uint32_t)interList[i].lo;
      if ((unsigned)p < (unsigned)P) {
        const EpRow row = rows[p];
        idOf[p] = (int)i;
        union {
          ccmi_plan_task t;
          uint4 q;
        } u;
        u.t.partition = p;
        u.t.num_to_add = (row.flags >> 8) & 15;
        u.t.data_to_move_mb = row.data;
        *reinterpret_cast<uint4*>(tasks + i) = u.q;
      }
    } else {
      leaderOut[i - numInter] = (int32_t)(uint32_t)leaderList[i - numInter].lo;
    }
  }
}

__global__ __launch_bounds__(kEpBlock) void execution_plan_scatter(EpTables T, EpQuery q, const EpRow* __restrict__ rows,
                                                                   const int32_t* __restrict__ idOf, int doInter,
                                                                   const unsigned long long* __restrict__ interOff,
                                                                   const unsigned long long* __restrict__ intraOff,
                                                                   uint32_t* __restrict__ cursors,
                                                                   SortEntry* __restrict__ interEntries,
                                                                   SortEntry* __restrict__ intraEntries) {
  uint32_t* curInter = cursors;
  uint32_t* curIntra = cursors + T.B;
  const int stride = gridDim.x * kEpBlock;
  for (int base = blockIdx.x * kEpBlock; base < T.pd.P; base += stride) {  // wave-uniform trip count
    const int p = base + (int)threadIdx.x;
    PdRow w = {};
    EpRow row;
    row.flags = 0;
    row.src = -1;
    row.data = 0;
    if (p < T.pd.P) row = rows[p];
    const bool inter = doInter && (row.flags & EP_INTER);
    const bool has = inter || ((row.flags >> 12) & 15) != 0;
    SortEntry key, okey;
    key.lo = key.hi = okey.lo = okey.hi = 0;
    if (has) {
      pdDiff(T.pd, p, w);
      if (inter) key = epTaskKey(q, T.state ? T.state[p] : 0u, row.data, (uint32_t)idOf[p]);
      okey.lo = epOrderKey(T.rank, p);
    }
    {
      const int b = inter ? row.src : -1;
      const bool ok = (unsigned)b < (unsigned)T.B;
      const uint32_t slot = waveSegAdd(curInter, b, ok);
      if (ok) {
        const unsigned long long at = interOff[b] + slot;
        if (at < interOff[b + 1]) interEntries[at] = key;  // always: the counts came from the same rows
      }
    }
#pragma unroll
    for (int x = 0; x < kMaxRf; ++x) {
      bool added, between;
      epSlotKind(w, x, added, between);
      const int b = w.newR[x];
      const bool inRange = (unsigned)b < (unsigned)T.B;
      const bool okA = has && inter && added && inRange;
      const uint32_t slotA = waveSegAdd(curInter, b, okA);
      if (okA) {
        const unsigned long long at = interOff[b] + slotA;
        if (at < interOff[b + 1]) interEntries[at] = key;
      }
      const bool okB = has && between && inRange;
      const uint32_t slotB = waveSegAdd(curIntra, b, okB);
      if (okB) {
        const unsigned long long at = intraOff[b] + slotB;
        if (at < intraOff[b + 1]) intraEntries[at] = okey;
      }
    }
  }
}

// brokerComparator's initial order (ExecutionTaskPlanner.java:518-539) over the brokers with tasks: the chain on the
// first tasks (equal keys are the same task), then the longer list, then the smaller index. order is preset to -1.
__global__ __launch_bounds__(kEpBlock) void execution_plan_order(const unsigned long long* __restrict__ offsets, int B,
                                                                 const SortEntry* __restrict__ bufA,
                                                                 const SortEntry* __restrict__ bufB,
                                                                 int32_t* __restrict__ order) {
  __shared__ uint4 headKey[kEpBlock];
  __shared__ uint32_t headLen[kEpBlock];
  const int b = blockIdx.x * kEpBlock + (int)threadIdx.x;
  const uint32_t myLen = epHeadLen(offsets, B, b);
  const uint4 myKey = epHeadKey(offsets, b, myLen, bufA, bufB);
  uint32_t rank = 0;
  for (int c0 = 0; c0 < B; c0 += kEpBlock) {
    const uint32_t l = epHeadLen(offsets, B, c0 + (int)threadIdx.x);
    headKey[threadIdx.x] = epHeadKey(offsets, c0 + (int)threadIdx.x, l, bufA, bufB);
    headLen[threadIdx.x] = l;
    __syncthreads();
    const int m = min(kEpBlock, B - c0);
    if (myLen > 0)
      for (int j = 0; j < m; ++j) {
        const uint32_t ol = headLen[j];
        if (ol == 0) continue;
        const uint4 ok = headKey[j];
        bool first;  // broker c0 + j comes before b
        if (EpLess::less(ok, myKey))
          first = true;
        else if (EpLess::less(myKey, ok))
          first = false;
        else
          first = ol != myLen ? ol > myLen : c0 + j < b;
        rank += first ? 1u : 0u;
      }
    __syncthreads();
  }
  if (myLen > 0 && rank < (uint32_t)B) order[rank] = b;
}

// out[k] = the low bits of entry k (mask: an execution id's 31 bits, or a partition index's 32): four per lane
__global__ __launch_bounds__(kEpBlock) void execution_plan_gather(const unsigned long long* __restrict__ offsets, int n,
                                                                  long long total, int anyLong, uint32_t mask,
                                                                  const SortEntry* __restrict__ bufA,
                                                                  const SortEntry* __restrict__ bufB,
                                                                  int32_t* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kEpBlock;
  for (long long quad = (long long)blockIdx.x * kEpBlock + threadIdx.x; 4 * quad < total; quad += stride) {
    int32_t v[4] = {-1, -1, -1, -1};
    const int cnt = (int)min(4ll, total - 4 * quad);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      if (h < cnt) {
        const long long k = 4 * quad + h;
        const SortEntry* buf = bufA;
        if (anyLong) {
          const int sg = segmentOf(offsets, n, k);
          if (segSortPasses((long long)(offsets[sg + 1] - offsets[sg])) & 1) buf = bufB;
        }
        v[h] = (int32_t)((uint32_t)buf[k].lo & mask);
      }
    }
    if (cnt == 4) {
      *reinterpret_cast<int4*>(out + 4 * quad) = make_int4(v[0], v[1], v[2], v[3]);  // out is 16-byte aligned
    } else {
#pragma unroll
      for (int h = 0; h < 4; ++h)
        if (h < cnt) out[4 * quad + h] = v[h];
    }
  }
}

// First half of a call on stream st: sums and counts cleared, classify, scan. The host then reads sums and state back.
// counts and cursors hold 2 * B words (inter, intra); state 2 * (B + 3) + 4 words.
hipError_t launchExecutionPlanCount(const EpTables& T, int tiles, EpRow* rows, uint32_t* tileInter,
                                    uint32_t* tileLeader, uint32_t* counts, uint32_t* cursors, EpSums* sums,
                                    unsigned long long* state, int* launches, hipStream_t stream) {
  const PdTables& D = T.pd;
  const bool anyDisk = D.initDisks || D.initLeaderDisks || D.curDisks;
  const bool allDisks = D.initDisks && D.initLeaderDisks && D.curDisks;
  if (D.P < 1 || D.R < 1 || T.B < 1 || !D.parts || !D.replicas || !D.pOff || !D.pSlots || !D.pLeader || !D.initDist ||
      !D.initLeaders || (anyDisk && !allDisks) || tiles != (D.P + kPdTile - 1) / kPdTile || !rows || !tileInter ||
      !tileLeader || !counts || !cursors || !sums || !state)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(EpSums), stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(counts, 0, 2 * (size_t)T.B * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const int blocks = std::min(kEpMaxBlocks, tiles);
  hipLaunchKernelGGL(execution_plan_classify, dim3((unsigned)blocks), dim3(kEpBlock), 0, stream, T, tiles, rows,
                     tileInter, tileLeader, counts, counts + T.B, sums);
  hipLaunchKernelGGL(execution_plan_scan, dim3(4), dim3(kEpScanBlock), 0, stream, tiles, tileInter, tileLeader, T.B,
                     counts, counts + T.B, cursors, sums, state);
  if (launches) *launches += 2;
  return hipGetLastError();
}

// Second half, when every list fits. numInter is 0 when the inter-broker tasks were dropped. bufA / bufB hold
// numInter + numLeader + interTotal + intraTotal entries each, in that order; order holds B words.
hipError_t launchExecutionPlanFill(const EpTables& T, const EpQuery& q, int tiles, const EpRow* rows,
                                   const uint32_t* tileInter, const uint32_t* tileLeader, uint32_t* cursors,
                                   const unsigned long long* state, long long numInter, long long numLeader,
                                   long long interTotal, long long interMax, long long intraTotal, long long intraMax,
                                   SortEntry* bufA, SortEntry* bufB, int32_t* idOf, ccmi_plan_task* tasks,
                                   int32_t* interOut, int32_t* order, int32_t* intraOut, int32_t* leaderOut,
                                   int* launches, hipStream_t stream) {
  const int P = T.pd.P, B = T.B;
  if (numInter < 0 || numInter > P || numLeader < 0 || numLeader > P || interTotal < 0 || intraTotal < 0 ||
      interMax > interTotal || intraMax > intraTotal || numInter + numLeader + interTotal + intraTotal < 1 || !rows ||
      !tileInter || !tileLeader || !cursors || !state || !bufA || !bufB || !idOf || !order || q.n < 0 || q.n > 4 ||
      (numInter > 0 && !tasks) || (interTotal > 0 && !interOut) || (intraTotal > 0 && !intraOut) ||
      (numLeader > 0 && !leaderOut))
    return hipErrorInvalidValue;
  const unsigned long long* interOff = state + 2;
  const unsigned long long* intraOff = state + ((size_t)B + 3) + 2;
  const unsigned long long* numOff = state + 2 * ((size_t)B + 3);
  const unsigned long long* leadOff = numOff + 2;
  SortEntry *numA = bufA, *numB = bufB;
  SortEntry *leadA = bufA + numInter, *leadB = bufB + numInter;
  SortEntry *interA = leadA + numLeader, *interB = leadB + numLeader;
  SortEntry *intraA = interA + interTotal, *intraB = interB + interTotal;
  int nl = 0;
  hipError_t e = hipMemsetAsync(order, 0xff, (size_t)B * sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
  const int doInter = numInter > 0 ? 1 : 0;
  const int pblocks = std::min(kEpMaxBlocks, (P + kEpBlock - 1) / kEpBlock);
  if (numInter + numLeader > 0) {
    hipLaunchKernelGGL(execution_plan_number, dim3((unsigned)std::min(kEpMaxBlocks, tiles)), dim3(kEpBlock), 0, stream, P,
                       tiles, rows, T.rank, tileInter, tileLeader, doInter, numA, leadA);
    nl++;
    const SortEntry *numSorted = numA, *leadSorted = leadA;
    if (T.rank) {  // the caller's order; without one the compaction is in order already
      if (numInter > 1) {
        nl += launchSegSort<EpLess>(numOff, 1, numInter, numInter, numA, numB, stream);
        if (segSortPasses(numInter) & 1) numSorted = numB;
      }
      if (numLeader > 1) {
        nl += launchSegSort<EpLess>(leadOff, 1, numLeader, numLeader, leadA, leadB, stream);
        if (segSortPasses(numLeader) & 1) leadSorted = leadB;
      }
    }
    const int iblocks = (int)std::min<long long>(kEpMaxBlocks, (numInter + numLeader + kEpBlock - 1) / kEpBlock);
    hipLaunchKernelGGL(execution_plan_ids, dim3((unsigned)iblocks), dim3(kEpBlock), 0, stream, P, rows, numInter,
                       numSorted, numLeader, leadSorted, idOf, tasks, leaderOut);
    nl++;
  }
  if (interTotal + intraTotal > 0) {
    hipLaunchKernelGGL(execution_plan_scatter, dim3((unsigned)pblocks), dim3(kEpBlock), 0, stream, T, q, rows, idOf,
                       doInter, interOff, intraOff, cursors, interA, intraA);
    nl++;
  }
  if (interTotal > 0) {
    nl += launchSegSort<EpLess>(interOff, B, interTotal, interMax, interA, interB, stream);
    hipLaunchKernelGGL(execution_plan_order, dim3((unsigned)((B + kEpBlock - 1) / kEpBlock)), dim3(kEpBlock), 0, stream,
                       interOff, B, interA, interB, order);
    const long long quads = (interTotal + 3) / 4;
    hipLaunchKernelGGL(execution_plan_gather,
                       dim3((unsigned)std::min<long long>(kEpMaxBlocks, (quads + kEpBlock - 1) / kEpBlock)),
                       dim3(kEpBlock), 0, stream, interOff, B, interTotal, interMax > kSegSortTile ? 1 : 0, 0x7fffffffu,
                       interA, interB, interOut);
    nl += 2;
  }
  if (intraTotal > 0) {
    nl += launchSegSort<EpLess>(intraOff, B, intraTotal, intraMax, intraA, intraB, stream);
    const long long quads = (intraTotal + 3) / 4;
    hipLaunchKernelGGL(execution_plan_gather,
                       dim3((unsigned)std::min<long long>(kEpMaxBlocks, (quads + kEpBlock - 1) / kEpBlock)),
                       dim3(kEpBlock), 0, stream, intraOff, B, intraTotal, intraMax > kSegSortTile ? 1 : 0, 0xffffffffu,
                       intraA, intraB, intraOut);
    nl++;
  }
  if (launches) *launches += nl;
  return hipGetLastError();
}

}  // namespace ccmi
