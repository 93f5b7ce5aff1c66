// gfx950 kernels of ccmi_aggregator (K17): MetricSampleAggregator on the device. The per-entity state machine and the
// value formulas are engine/aggregator_entity.h (RawMetricValues transcribed, shared with the host unit test); this file
// is the batching around it. State layout: AggTables in devtypes.h (entity-minor).
//
// add_samples (the host has already turned the batch's timestamps into accepted flags and the roll-out events):
//     agg_count    : runOff[e] = accepted samples of entity e, one atomic per distinct entity in a wave (waveSegAdd)
//     agg_scan     : one workgroup, exclusive scan in place; runOff[E] = the total
//     agg_scatter  : order[runOff[e] + slot] = batch position; the slot is an atomic's arrival order, so
//     agg_replay   : one lane per entity first sorts its own run by batch position (runs are one or two long), then
//                    replays in batch order the roll-out events (updateOldestWindowIndex + resetWindowIndices, taken by
//                    every present entity, sampled or not) and its own samples (addSample; the first accepted sample of
//                    an absent entity creates its RawMetricValues at the oldest window of that moment). No result
//                    depends on an atomic's arrival order.
// completeness walk, per window newest to oldest, no host synchronisation in between (WindowState.maybeInclude):
//     agg_walk_init / agg_walk_group_total : the interested entities and groups and their totals
//     agg_walk_entities : fillInValidRatios' loop: validEntitiesForWindow, per-group valid counts (waveSegAdd) and
//                         invalid flags, the valid and extrapolated counts
//     agg_walk_groups   : validGroupsForWindow, the group-granularity entity count, the merge count of the groups
//     agg_walk_merge    : the ENTITY_GROUP filter and the merge count of the entities
//     agg_walk_apply    : every lane takes the include decision from the finished counters ((float) n / total >=
//                         (double) ratio with n > 0); on inclusion the retainAlls and the extrapolation counts
//     agg_walk_final    : the "no window included" clear and the final counts
// aggregate / peek: agg_cover (covered entities per tile of kAggTile), agg_cover_scan, agg_rows (stable compaction in id
// order by ballot ranks, one lane per covered entity writes its row through aggregateWindow).
// Every launch is a kernel boundary on the aggregator's stream; no workgroup reads another's writes inside a launch.
// All counters are integer atomics (order-free); the floats of a row are computed by one lane from one entity's state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../engine/aggregator.h"
#include "../engine/aggregator_entity.h"
#include "../engine/devtypes.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kAggWaves = kAggBlock / 64;
constexpr int kAggRounds = kAggTile / kAggBlock;
constexpr int kAggScanBlock = 1024;

__device__ __forceinline__ agg::RawView aggView(const AggTables& T, long long e, long long oldest) {
  agg::RawView r;
  r.counts = T.counts + e;
  r.values = T.values + e;
  r.countStride = T.E;
  r.windowStride = (long long)T.M * T.E;
  r.metricStride = T.E;
  r.fn = T.fn;
  r.oldest = oldest;
  r.valid = T.valid[e];
  r.extrap = T.extrap[e];
  r.L = T.L;
  r.M = T.M;
  r.minSamples = T.minSamples;
  r.halfMin = T.halfMin;
  return r;
}

// every lane of the wave calls it; one atomic per wave
__device__ __forceinline__ void waveCount(unsigned long long* dst, unsigned long long v) {
  v = waveSum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

__device__ __forceinline__ bool aggCovered(const AggTables& T, const AggWalk& W, int source, long long e) {
  return (source == 0 ? W.inter[e] : source == 1 ? W.validE[e] : T.present[e]) != 0;
}

__device__ __forceinline__ bool aggInclude(const unsigned long long* ctr, int j, const AggWalkOptions& o) {
  const unsigned long long* c = ctr + kAggCtrHead + j * kAggCtrPerWindow;
  const unsigned long long nE = c[kAwMergeE], nG = c[kAwMergeG];
  if (nE == 0 || nG == 0) return false;
  const float rE = (float)nE / (float)ctr[kAcTotalE], rG = (float)nG / (float)ctr[kAcTotalG];
  return (double)rE >= o.minEntityRatio && (double)rG >= o.minGroupRatio;
}

inline unsigned aggGrid(long long n) {
  return (unsigned)std::max<long long>(1, std::min<long long>(kAggMaxBlocks, (n + kAggBlock - 1) / kAggBlock));
}

}  // namespace

// ------------------------------------------------------------------------------------------------ add_samples
__global__ __launch_bounds__(kAggBlock) void agg_count(const int32_t* __restrict__ entity,
                                                       const uint8_t* __restrict__ accepted, long long n,
                                                       uint32_t* __restrict__ runOff) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < n; base += stride) {  // wave-uniform
    const long long i = base + threadIdx.x;
    const bool active = i < n && accepted[i];
    waveSegAdd(runOff, active ? entity[i] : 0, active);
  }
}

__global__ __launch_bounds__(kAggScanBlock) void agg_scan(uint32_t* __restrict__ counts, int n) {
  const uint32_t total = scanCountsInPlace<uint32_t, kAggScanBlock>(counts, n);
  if (threadIdx.x == 0) counts[n] = total;
}

__global__ __launch_bounds__(kAggBlock) void agg_scatter(const int32_t* __restrict__ entity,
                                                         const uint8_t* __restrict__ accepted, long long n,
                                                         const uint32_t* __restrict__ runOff,
                                                         uint32_t* __restrict__ cursor, uint32_t* __restrict__ order) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < n; base += stride) {  // wave-uniform
    const long long i = base + threadIdx.x;
    const bool active = i < n && accepted[i];
    const int e = active ? entity[i] : 0;
    const uint32_t slot = waveSegAdd(cursor, e, active);
    if (active) order[runOff[e] + slot] = (uint32_t)i;  // slot < the entity's count: inside [runOff[e], runOff[e + 1])
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_replay(AggTables T, const int64_t* __restrict__ timeMs,
                                                        const double* __restrict__ values,
                                                        const uint32_t* __restrict__ runOff, uint32_t* __restrict__ order,
                                                        const AggRollEvent* __restrict__ events, int numEvents,
                                                        long long startOldest, long long windowMs) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long e = (long long)blockIdx.x * kAggBlock + threadIdx.x; e < T.E; e += stride) {
    const uint32_t off = runOff[e], len = runOff[e + 1] - off;
    bool present = T.present[e] != 0;
    if (len == 0 && (!present || numEvents == 0)) continue;
    for (uint32_t i = 1; i < len; ++i) {  // the run by batch position
      const uint32_t v = order[off + i];
      uint32_t k = i;
      for (; k > 0 && order[off + k - 1] > v; --k) order[off + k] = order[off + k - 1];
      order[off + k] = v;
    }
    agg::RawView r = aggView(T, e, present ? startOldest : agg::kFresh);
    long long aggOldest = startOldest;
    int ev = 0;
    for (uint32_t k = 0; k <= len; ++k) {
      const long long pos = k < len ? (long long)order[off + k] : 0x7fffffffffffffffLL;
      for (; ev < numEvents && events[ev].pos <= pos; ++ev) {  // the roll-outs up to and including this sample's own
        if (present) {
          agg::updateOldestWindowIndex(r, events[ev].newOldest);
          agg::resetWindowIndices(r, events[ev].prevOldest, events[ev].numReset);
        }
        aggOldest = events[ev].newOldest;
      }
      if (k == len) break;
      if (!present) {  // computeIfAbsent: a new RawMetricValues at the aggregator's oldest window
        present = true;
        agg::updateOldestWindowIndex(r, aggOldest);
      }
      agg::addSample(r, timeMs[pos] / windowMs + 1, values + pos * T.M);
    }
    T.valid[e] = r.valid;
    T.extrap[e] = r.extrap;
    T.present[e] = 1;
  }
}

void aggLaunchAddSamples(const AggTables& T, const int32_t* entity, const int64_t* timeMs, const double* values,
                         const uint8_t* accepted, int64_t n, const AggRollEvent* events, int numEvents,
                         long long startOldest, long long windowMs, uint32_t* runOff, uint32_t* cursor, uint32_t* order,
                         hipStream_t st) {
  (void)hipMemsetAsync(runOff, 0, sizeof(uint32_t) * ((size_t)T.E + 1), st);
  (void)hipMemsetAsync(cursor, 0, sizeof(uint32_t) * (size_t)T.E, st);
  hipLaunchKernelGGL(agg_count, dim3(aggGrid(n)), dim3(kAggBlock), 0, st, entity, accepted, (long long)n, runOff);
  hipLaunchKernelGGL(agg_scan, dim3(1), dim3(kAggScanBlock), 0, st, runOff, T.E);
  hipLaunchKernelGGL(agg_scatter, dim3(aggGrid(n)), dim3(kAggBlock), 0, st, entity, accepted, (long long)n, runOff,
                     cursor, order);
  hipLaunchKernelGGL(agg_replay, dim3(aggGrid(T.E)), dim3(kAggBlock), 0, st, T, timeMs, values, runOff, order, events,
                     numEvents, startOldest, windowMs);
}

// ------------------------------------------------------------------------------------------------ completeness
__global__ __launch_bounds__(kAggBlock) void agg_walk_init(AggTables T, AggWalk W, const uint8_t* __restrict__ mask) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < T.E; base += stride) {  // wave-uniform
    const long long e = base + threadIdx.x;
    bool in = false;
    if (e < T.E) {
      in = (mask ? mask[e] : T.present[e]) != 0;
      W.inter[e] = in;
      W.validE[e] = in;
      W.extrapCnt[e] = 0;
      if (in) {
        W.ginter[T.group[e]] = 1;  // every writer stores the same value
        W.validG[T.group[e]] = 1;
      }
    }
    waveCount(&W.ctr[kAcTotalE], in ? 1 : 0);
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_walk_group_total(AggTables T, AggWalk W) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < T.G; base += stride) {
    const long long g = base + threadIdx.x;
    waveCount(&W.ctr[kAcTotalG], g < T.G && W.ginter[g] ? 1 : 0);
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_walk_entities(AggTables T, AggWalk W, int j, long long window,
                                                               int maxExtrapolations) {
  const int a = (int)(window % T.L);
  unsigned long long* c = W.ctr + kAggCtrHead + j * kAggCtrPerWindow;
  uint32_t* gCnt = W.gValidCnt + (size_t)j * T.G;
  uint8_t* gInv = W.gInvalid + (size_t)j * T.G;
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < T.E; base += stride) {  // wave-uniform
    const long long e = base + threadIdx.x;
    bool ok = false, extrapolated = false;
    int g = 0;
    if (e < T.E && W.inter[e]) {
      g = T.group[e];
      const bool valid = (T.valid[e] >> a) & 1u;  // an absent entity's words are clear
      const bool x = (T.extrap[e] >> a) & 1u;
      if (valid) {
        extrapolated = x;
        ok = W.extrapCnt[e] + (x ? 1 : 0) <= maxExtrapolations;
      }
      if (!ok) gInv[g] = 1;
    }
    if (e < T.E) W.vfw[e] = ok;
    waveSegAdd(gCnt, g, ok);
    waveCount(&c[kAwValid], ok ? 1 : 0);
    waveCount(&c[kAwExtrap], extrapolated ? 1 : 0);
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_walk_groups(AggTables T, AggWalk W, int j) {
  unsigned long long* c = W.ctr + kAggCtrHead + j * kAggCtrPerWindow;
  const uint32_t* gCnt = W.gValidCnt + (size_t)j * T.G;
  const uint8_t* gInv = W.gInvalid + (size_t)j * T.G;
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < T.G; base += stride) {  // wave-uniform
    const long long g = base + threadIdx.x;
    bool vw = false;
    uint32_t n = 0;
    bool merged = false;
    if (g < T.G) {
      n = gCnt[g];
      vw = n > 0 && !gInv[g];
      W.gValidW[g] = vw;
      merged = vw && W.validG[g];
    }
    waveCount(&c[kAwGroups], vw ? 1 : 0);
    waveCount(&c[kAwGroupGran], vw ? n : 0);
    waveCount(&c[kAwMergeG], merged ? 1 : 0);
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_walk_merge(AggTables T, AggWalk W, int j, int groupGranularity) {
  unsigned long long* c = W.ctr + kAggCtrHead + j * kAggCtrPerWindow;
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < T.E; base += stride) {  // wave-uniform
    const long long e = base + threadIdx.x;
    bool merged = false;
    if (e < T.E) {
      bool f = W.vfw[e] != 0;
      if (f && groupGranularity) f = W.gValidW[T.group[e]] != 0;
      W.vfw[e] = f;
      merged = f && W.validE[e];
    }
    waveCount(&c[kAwMergeE], merged ? 1 : 0);
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_walk_apply(AggTables T, AggWalk W, int j, long long window,
                                                            AggWalkOptions o) {
  if (!aggInclude(W.ctr, j, o)) return;  // the same counters in every lane: a uniform decision
  const int a = (int)(window % T.L);
  const long long n = T.E > T.G ? T.E : T.G;
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long i = (long long)blockIdx.x * kAggBlock + threadIdx.x; i < n; i += stride) {
    if (i < T.E) {
      const bool f = W.vfw[i] != 0;
      if (!f) W.validE[i] = 0;
      if (f && ((T.extrap[i] >> a) & 1u)) W.extrapCnt[i] += 1;
    }
    if (i < T.G && !W.gValidW[i]) W.validG[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // words no lane reads in this launch
    W.ctr[kAggCtrHead + j * kAggCtrPerWindow + kAwIncluded] = 1;
    W.ctr[kAcIncluded] += 1;
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_walk_final(AggTables T, AggWalk W) {
  const bool none = W.ctr[kAcIncluded] == 0;
  const long long n = T.E > T.G ? T.E : T.G;
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < n; base += stride) {  // wave-uniform
    const long long i = base + threadIdx.x;
    bool ve = false, vg = false;
    if (i < T.E) {
      if (none) W.validE[i] = 0;
      ve = W.validE[i] != 0;
    }
    if (i < T.G) {
      if (none) W.validG[i] = 0;
      vg = W.validG[i] != 0;
    }
    waveCount(&W.ctr[kAcValidE], ve ? 1 : 0);
    waveCount(&W.ctr[kAcValidG], vg ? 1 : 0);
  }
}

void aggLaunchWalk(const AggTables& T, const AggWalk& W, const uint8_t* mask, long long firstWindow, int numWindows,
                   const AggWalkOptions& o, hipStream_t st) {
  const int nw = std::max(numWindows, 1);
  (void)hipMemsetAsync(W.ctr, 0, sizeof(unsigned long long) * (kAggCtrHead + (size_t)nw * kAggCtrPerWindow), st);
  (void)hipMemsetAsync(W.ginter, 0, (size_t)T.G, st);
  (void)hipMemsetAsync(W.validG, 0, (size_t)T.G, st);
  (void)hipMemsetAsync(W.gValidCnt, 0, sizeof(uint32_t) * (size_t)nw * T.G, st);
  (void)hipMemsetAsync(W.gInvalid, 0, (size_t)nw * T.G, st);
  const dim3 ge(aggGrid(T.E)), gg(aggGrid(T.G)), gb(aggGrid(std::max(T.E, T.G))), blk(kAggBlock);
  hipLaunchKernelGGL(agg_walk_init, ge, blk, 0, st, T, W, mask);
  hipLaunchKernelGGL(agg_walk_group_total, gg, blk, 0, st, T, W);
  for (int j = 0; j < numWindows; ++j) {
    const long long w = firstWindow - j;
    hipLaunchKernelGGL(agg_walk_entities, ge, blk, 0, st, T, W, j, w, o.maxExtrapolations);
    hipLaunchKernelGGL(agg_walk_groups, gg, blk, 0, st, T, W, j);
    hipLaunchKernelGGL(agg_walk_merge, ge, blk, 0, st, T, W, j, o.groupGranularity);
    hipLaunchKernelGGL(agg_walk_apply, gb, blk, 0, st, T, W, j, w, o);
  }
  hipLaunchKernelGGL(agg_walk_final, gb, blk, 0, st, T, W);
}

// ------------------------------------------------------------------------------------------------ rows
__global__ __launch_bounds__(kAggBlock) void agg_cover(AggTables T, AggWalk W, int source, int tiles,
                                                       uint32_t* __restrict__ tileOff) {
  __shared__ uint32_t tileCnt;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (threadIdx.x == 0) tileCnt = 0;
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll 1
    for (int k = 0; k < kAggRounds; ++k) {
      const long long e = (long long)tile * kAggTile + k * kAggBlock + threadIdx.x;
      const bool c = e < T.E && aggCovered(T, W, source, e);
      mine += (uint32_t)__popcll(__ballot(c));
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&tileCnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) tileOff[tile] = tileCnt;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kAggScanBlock) void agg_cover_scan(uint32_t* __restrict__ tileOff, int tiles,
                                                                unsigned long long* __restrict__ ctr) {
  const uint32_t total = scanCountsInPlace<uint32_t, kAggScanBlock>(tileOff, tiles);
  if (threadIdx.x == 0) {
    tileOff[tiles] = total;
    ctr[kAcCovered] = total;
  }
}

void aggLaunchCover(const AggTables& T, const AggWalk& W, int source, uint32_t* tileOff, hipStream_t st) {
  const int tiles = (T.E + kAggTile - 1) / kAggTile;
  hipLaunchKernelGGL(agg_cover, dim3((unsigned)std::min(tiles, kAggMaxBlocks)), dim3(kAggBlock), 0, st, T, W, source,
                     tiles, tileOff);
  hipLaunchKernelGGL(agg_cover_scan, dim3(1), dim3(kAggScanBlock), 0, st, tileOff, tiles, W.ctr);
}

__global__ __launch_bounds__(kAggBlock) void agg_rows(AggTables T, AggWalk W, int source, int tiles,
                                                      const uint32_t* __restrict__ tileOff,
                                                      const long long* __restrict__ windows, int numWindows,
                                                      long long oldest, int maxExtrapolations, long long capacity,
                                                      int32_t* __restrict__ entities, float* __restrict__ values,
                                                      uint8_t* __restrict__ extrapolations,
                                                      uint8_t* __restrict__ invalid) {
  __shared__ uint32_t waveCnt[kAggWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    long long base = tileOff[tile];
    if (base >= capacity || tileOff[tile + 1] == (uint32_t)base) continue;  // uniform in the workgroup
#pragma unroll 1
    for (int k = 0; k < kAggRounds; ++k) {
      const long long e = (long long)tile * kAggTile + k * kAggBlock + threadIdx.x;
      const bool c = e < T.E && aggCovered(T, W, source, e);
      const unsigned long long m = __ballot(c);
      if (lane == 0) waveCnt[wave] = (uint32_t)__popcll(m);
      __syncthreads();
      long long rank = base + __popcll(m & ((1ull << lane) - 1ull));
      uint32_t all = 0;
      for (int w = 0; w < kAggWaves; ++w) {
        if (w < wave) rank += waveCnt[w];
        all += waveCnt[w];
      }
      base += all;
      __syncthreads();
      if (c && rank < capacity) {
        entities[rank] = (int32_t)e;
        float* out = values + rank * T.M * numWindows;
        uint8_t* ex = extrapolations + rank * numWindows;
        bool bad = true;
        if (T.present[e]) {
          const agg::RawView r = aggView(T, e, oldest);
          for (int j = 0; j < numWindows; ++j) ex[j] = (uint8_t)agg::aggregateWindow(r, windows[j], out + j, numWindows);
          bad = !agg::isValid(r, maxExtrapolations);
        } else {  // ValuesAndExtrapolations.empty
          for (int j = 0; j < numWindows; ++j) {
            ex[j] = (uint8_t)agg::kExNoValid;
            for (int mm = 0; mm < T.M; ++mm) out[(long long)mm * numWindows + j] = 0.0f;
          }
        }
        if (invalid) invalid[rank] = bad;
      }
    }
  }
}

void aggLaunchRows(const AggTables& T, const AggWalk& W, int source, const uint32_t* tileOff, const long long* windows,
                   int numWindows, long long oldest, int maxExtrapolations, int64_t capacity, int32_t* entities,
                   float* values, uint8_t* extrapolations, uint8_t* invalid, hipStream_t st) {
  const int tiles = (T.E + kAggTile - 1) / kAggTile;
  hipLaunchKernelGGL(agg_rows, dim3((unsigned)std::min(tiles, kAggMaxBlocks)), dim3(kAggBlock), 0, st, T, W, source,
                     tiles, tileOff, windows, numWindows, oldest, maxExtrapolations, (long long)capacity, entities, values,
                     extrapolations, invalid);
}

// ------------------------------------------------------------------------------------------------ state, remove
__global__ __launch_bounds__(kAggBlock) void agg_state_sums(AggTables T, unsigned long long* __restrict__ sums) {
  const long long n = (long long)T.L * T.E;
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long base = (long long)blockIdx.x * kAggBlock; base < n; base += stride) {  // wave-uniform
    const long long i = base + threadIdx.x;
    waveCount(&sums[0], i < n ? T.counts[i] : 0);
    waveCount(&sums[1], i < T.E && T.present[i] ? 1 : 0);
  }
}

void aggLaunchStateSums(const AggTables& T, unsigned long long* sums, hipStream_t st) {
  (void)hipMemsetAsync(sums, 0, 2 * sizeof(unsigned long long), st);
  hipLaunchKernelGGL(agg_state_sums, dim3(aggGrid((long long)T.L * T.E)), dim3(kAggBlock), 0, st, T, sums);
}

__global__ __launch_bounds__(kAggBlock) void agg_remove(AggTables T, const int32_t* __restrict__ ids, long long n,
                                                        uint32_t* __restrict__ removed) {
  const long long stride = (long long)gridDim.x * kAggBlock;
  for (long long i = (long long)blockIdx.x * kAggBlock + threadIdx.x; i < n; i += stride) {
    const long long e = ids[i];
    if (!T.present[e]) continue;  // an id named twice: both lanes store the same zeros
    for (int a = 0; a < T.L; ++a) T.counts[(long long)a * T.E + e] = 0;
    T.valid[e] = 0;
    T.extrap[e] = 0;
    T.present[e] = 0;
    *removed = 1;
  }
}

void aggLaunchRemove(const AggTables& T, const int32_t* ids, int64_t n, uint32_t* removed, hipStream_t st) {
  (void)hipMemsetAsync(removed, 0, sizeof(uint32_t), st);
  hipLaunchKernelGGL(agg_remove, dim3(aggGrid(n)), dim3(kAggBlock), 0, st, T, ids, (long long)n, removed);
}

}  // namespace ccmi
