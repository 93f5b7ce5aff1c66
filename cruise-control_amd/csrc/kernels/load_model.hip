// gfx950 kernels of ccmi_builder_populate_from_aggregator (K18): MonitorUtils.populatePartitionLoad over every row of
// an aggregate, from the rows K17's agg_rows left in the aggregator's device buffer to the model builder's columns. The
// per-replica arithmetic is engine/replica_load.h (shared with the host unit test); this file is the batching around it.
//     load_classify : one lane per aggregate row. Reads the partition's slice of the topology and repeats the checks of
//                     ccmi_builder_populate_partition in its order: every replica's broker against the builder's
//                     sorted id table, duplicates among the (at most 8) replicas, then, for a partition that is not
//                     offline, exactly one replica on the leader's broker. Emits the replica count of a partition that
//                     will be populated (0: empty range or offline), the leader's position, and on a complaint
//                     (entity << 2 | code) into one word by atomicMin: rows are in ascending entity order, so the
//                     minimum is the complaint the per-row loop would have raised first.
//     load_offsets  : one workgroup, exclusive scan of (populated, replicas) packed in 64 bits (segments.h
//                     blockExclusiveScan): the compacted partition rank and replica offset of every row, the totals.
//     load_columns  : one lane per row writes its partition's three columns and its replicas' five, plus a descriptor
//                     word per replica (row, n, leader position, own position) for the next kernel.
//     load_values   : replica_load [R'][6][W]. A workgroup takes tiles of kAggBlock / W whole replicas; one lane per
//                     (replica, window) reads the replica's descriptor and the row's six picked leader floats, runs
//                     replicaLoadWindow once and puts its six results where they belong in a 6 KB LDS image of the
//                     tile's slice of replica_load; the workgroup then streams the image out, a wave storing 256
//                     contiguous bytes. (The first version mapped lanes over the flat output index and had each lane
//                     keep one of six results: six lanes repeated one double division and the kernel was VALU-bound at
//                     12 % of the HBM peak, DESIGN.md "K18 measured".) No MFMA.
// Every launch is a kernel boundary on the aggregator's stream; no workgroup reads another's writes inside a launch. The
// only atomic is the integer minimum of load_classify (order-free); every float is computed by one lane from one row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../engine/aggregator.h"
#include "../engine/devtypes.h"
#include "../engine/replica_load.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kLoadScanBlock = 1024;
constexpr int kLoadValueBlocks = 2048;  // workgroups of load_values' grid-stride pass

inline unsigned loadGrid(long long n) {
  return (unsigned)std::max<long long>(1, std::min<long long>(kAggMaxBlocks, (n + kAggBlock - 1) / kAggBlock));
}

__device__ __forceinline__ bool loadKnownBroker(const int32_t* __restrict__ ids, int n, int32_t id) {
  int lo = 0, hi = n;  // the first index with ids[i] >= id
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < id)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && ids[lo] == id;
}

}  // namespace

__global__ __launch_bounds__(kAggBlock) void load_classify(LoadTopology T, LoadRows R, LoadScratch S) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long row = (long long)blockIdx.x * kAggBlock + threadIdx.x; row < R.k; row += stride) {
    const long long e = R.entities[row];
    const int32_t off = T.replicaOffset[e];
    const int n = T.replicaOffset[e + 1] - off;  // 0..kMaxReplicas: the host refused anything else
    const int32_t* ids = T.replicaBroker + off;
    int code = 0, leaders = 0, leaderIdx = 0;
    for (int i = 0; i < n && !code; ++i) {
      const int32_t id = ids[i];
      if (!loadKnownBroker(T.knownBrokers, T.numKnown, id)) {
        code = kLoadErrUnknownBroker;
        break;
      }
      for (int j = 0; j < i; ++j)
        if (ids[j] == id) code = kLoadErrDuplicateBroker;
    }
    const int32_t leader = T.leader[e];
    uint32_t kept = 0;
    if (!code && n > 0 && leader >= 0) {  // an offline partition is checked and skipped
      for (int i = 0; i < n; ++i)
        if (ids[i] == leader) {
          leaders++;
          leaderIdx = i;
        }
      if (leaders != 1)
        code = kLoadErrLeader;
      else
        kept = (uint32_t)n;
    }
    if (code) atomicMin(&S.state[kLoadStateError], ((unsigned long long)e << 2) | (unsigned long long)code);
    S.kept[row] = kept;
    S.leaderIdx[row] = (uint8_t)leaderIdx;
  }
}

__global__ __launch_bounds__(kLoadScanBlock) void load_offsets(LoadScratch S, long long k) {
  const long long chunk = (k + kLoadScanBlock - 1) / kLoadScanBlock;
  const long long i0 = min(k, (long long)threadIdx.x * chunk), i1 = min(k, i0 + chunk);
  unsigned long long sum = 0, total;  // populated partitions << 32 | their replicas (both below 2^31)
  for (long long i = i0; i < i1; ++i) {
    const uint32_t c = S.kept[i];
    sum += c ? (1ull << 32) | c : 0ull;
  }
  unsigned long long run = blockExclusiveScan<unsigned long long, kLoadScanBlock>(sum, &total);
  for (long long i = i0; i < i1; ++i) {
    const uint32_t c = S.kept[i];
    S.rank[i] = (uint32_t)(run >> 32);
    S.replicaBase[i] = (uint32_t)run;
    run += c ? (1ull << 32) | c : 0ull;
  }
  if (threadIdx.x == 0) {
    S.state[kLoadStatePartitions] = total >> 32;
    S.state[kLoadStateReplicas] = total & 0xffffffffull;
  }
}

void loadLaunchClassify(const LoadTopology& T, const LoadRows& R, const LoadScratch& S, hipStream_t st) {
  (void)hipMemsetAsync(S.state, 0xff, sizeof(unsigned long long), st);  // kLoadNoError
  hipLaunchKernelGGL(load_classify, dim3(loadGrid(R.k)), dim3(kAggBlock), 0, st, T, R, S);
  hipLaunchKernelGGL(load_offsets, dim3(1), dim3(kLoadScanBlock), 0, st, S, R.k);
}

__global__ __launch_bounds__(kAggBlock) void load_columns(LoadTopology T, LoadRows R, LoadScratch S, LoadColumns C) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long row = (long long)blockIdx.x * kAggBlock + threadIdx.x; row < R.k; row += stride) {
    const int n = (int)S.kept[row];
    if (n == 0) continue;
    const long long e = R.entities[row];
    const uint32_t p = S.rank[row], r0 = S.replicaBase[row];  // p < P', r0 + n <= R': the scan's totals
    const int32_t off = T.replicaOffset[e];
    const int leaderIdx = S.leaderIdx[row];
    C.pTopic[p] = T.topic[e];
    C.pNumber[p] = T.number[e];
    C.pEnd[p] = C.baseReplica + (int32_t)(r0 + (uint32_t)n);
    for (int i = 0; i < n; ++i) {
      const uint32_t r = r0 + (uint32_t)i;
      C.rBroker[r] = T.replicaBroker[off + i];
      C.rPartition[r] = C.basePartition + (int32_t)p;
      C.rLeader[r] = i == leaderIdx ? 1 : 0;
      C.rOffline[r] = T.offline && T.offline[off + i] ? 1 : 0;
      C.rLogdir[r] = T.logdir ? T.logdir[off + i] : -1;
      C.rDesc[r] = ((unsigned long long)row << 16) | ((unsigned long long)n << 8) |
                   ((unsigned long long)leaderIdx << 4) | (unsigned long long)i;
    }
  }
}

void loadLaunchColumns(const LoadTopology& T, const LoadRows& R, const LoadScratch& S, const LoadColumns& C,
                       hipStream_t st) {
  hipLaunchKernelGGL(load_columns, dim3(loadGrid(R.k)), dim3(kAggBlock), 0, st, T, R, S, C);
}

__global__ __launch_bounds__(kAggBlock) void load_values(LoadRows R, LoadColumns C, long long numReplicas) {
  __shared__ float tile[kAggBlock * rload::kMetrics];
  const int W = R.W, per = rload::kMetrics * W;  // floats of one replica, at most 30
  const int perTile = kAggBlock / W;             // whole replicas of a tile: perTile * W lanes compute, perTile * per floats
  const long long tiles = (numReplicas + perTile - 1) / perTile;
  const int t = (int)threadIdx.x;
  for (long long i = blockIdx.x; i < tiles; i += gridDim.x) {  // uniform in the workgroup
    const long long r0 = i * perTile;
    const int nr = (int)min((long long)perTile, numReplicas - r0);
    if (t < nr * W) {
      const int lr = t / W, w = t - lr * W;
      const unsigned long long d = C.rDesc[r0 + lr];  // r0 + lr < R'
      const float* v = R.values + (long long)(d >> 16) * R.M * W + w;
      float lead[rload::kMetrics], out[rload::kMetrics];
#pragma unroll
      for (int j = 0; j < rload::kMetrics; ++j) lead[j] = v[(long long)R.metricOf[j] * W];
      rload::replicaLoadWindow(lead, (int)(d & 15u), (int)((d >> 4) & 15u), (int)((d >> 8) & 255u), out);
#pragma unroll
      for (int m = 0; m < rload::kMetrics; ++m) tile[lr * per + m * W + w] = out[m];  // below perTile * per <= 1536
    }
    __syncthreads();
    float* dst = C.load + r0 * per;  // the tile's replicas are consecutive in replica_load: (r0 + nr) * per <= R' * per
    const int n = nr * per;
    for (int k = t; k < n; k += kAggBlock) dst[k] = tile[k];
    __syncthreads();
  }
}

void loadLaunchLoads(const LoadRows& R, const LoadColumns& C, long long numReplicas, hipStream_t st) {
  if (numReplicas == 0) return;
  const int perTile = kAggBlock / R.W;
  const long long tiles = (numReplicas + perTile - 1) / perTile;
  hipLaunchKernelGGL(load_values, dim3((unsigned)std::min<long long>(kLoadValueBlocks, tiles)), dim3(kAggBlock), 0, st, R,
                     C, numReplicas);
}

}  // namespace ccmi
