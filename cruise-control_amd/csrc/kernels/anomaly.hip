// gfx950 kernels of the metric anomaly finders (K19): PercentileMetricAnomalyFinder and SlowBrokerFinder over the
// history rows (an aggregate) and the current rows (peekCurrentWindow) that K17's agg_rows left on the device. The
// percentile and isDataSufficient are engine/percentile.h (shared with the host unit test); this file is the batching.
//
//     anom_row_of    : rowOf[entity] = its row in a row set (the array is cleared to -1 before)
//     anom_history   : one lane per (current row, slot). A slot is a metric (percentile finder) or the log flush time /
//                      the per-byte log flush time (slow broker finder, with its two history filters). The lane widens
//                      its history to double into its own LDS column (lane-minor, no bank shared within a wave) and takes
//                      the order statistics there by rank counting: no private array is indexed dynamically and no lane
//                      reads another's column, so the kernel has no barrier. The percentile finder writes a flag and a
//                      staged record per item; the slow broker finder writes the row's current values, its history hits,
//                      its skip flag and one sort entry per slot keyed by the current value (a skipped row and a NaN
//                      get keys behind every number), and counts the active rows and their NaNs.
//     the sort       : the segment toolkit's launchSegSort over the two segments of k entries (kernels/segments.h)
//     anom_peer_base : two lanes read the two adjacent order statistics of their sorted segment
//     anom_slow_update : one lane per entity, current or not: suspect, the score update, the classification, the
//                      diagnostic byte; the counts are wave-aggregated
//     anom_scan / anom_gather, anom_slow_gather : flags -> exclusive scan in place -> the ordered records
// Every launch is a kernel boundary on the aggregator's stream; no workgroup reads another's writes inside a launch.
// Counters are integer atomics (order-free); every double is computed by one lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../engine/aggregator.h"
#include "../engine/devtypes.h"
#include "../engine/percentile.h"
#include "segments.h"

namespace ccmi {

namespace {

constexpr int kAnomScanBlock = 1024;

// the ccmi_slow_broker diagnostic bits (include/ccmi.h CCMI_SLOW_DIAG_*)
constexpr int kDiagSkipped = 1, kDiagFlushHistory = 2, kDiagFlushPeers = 4, kDiagPerByteHistory = 8,
              kDiagPerBytePeers = 16, kDiagOverThreshold = 32, kDiagSuspect = 64;

// every lane of the wave calls it; one atomic per wave
__device__ __forceinline__ void anomCount(unsigned long long* dst, unsigned long long v) {
  v = waveSum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

inline unsigned anomGrid(long long n) {
  return (unsigned)std::max<long long>(1, std::min<long long>(kAnomMaxBlocks, (n + kAnomBlock - 1) / kAnomBlock));
}

// entries as the sort moves them (x, y = lo; z, w = hi): by key, then by row (rows are distinct)
struct AnomLess {
  static __device__ __forceinline__ bool less(const uint4& a, const uint4& b) {
    const uint64_t ah = ((uint64_t)a.w << 32) | a.z, bh = ((uint64_t)b.w << 32) | b.z;
    if (ah != bh) return ah < bh;
    return (((uint64_t)a.y << 32) | a.x) < (((uint64_t)b.y << 32) | b.x);
  }
};

struct LdsColumn {  // a lane's history in LDS, lane-minor
  const double* p;
  __device__ __forceinline__ double operator()(int i) const { return p[i * kAnomBlock]; }
};

struct SortedKeys {  // a sorted segment read back as doubles
  const SortEntry* p;
  __device__ __forceinline__ double operator()(int i) const { return pct::fromOrderedKey(p[i].hi); }
};

}  // namespace

__global__ __launch_bounds__(kAnomBlock) void anom_row_of(const int32_t* __restrict__ entities, long long k,
                                                          int32_t* __restrict__ rowOf) {
  const long long stride = (long long)gridDim.x * kAnomBlock;
  for (long long r = (long long)blockIdx.x * kAnomBlock + threadIdx.x; r < k; r += stride) rowOf[entities[r]] = (int32_t)r;
}

void anomLaunchRowOf(const AnomRows& rows, int32_t E, int32_t* rowOf, hipStream_t st) {
  (void)hipMemsetAsync(rowOf, 0xff, sizeof(int32_t) * (size_t)E, st);
  if (rows.k > 0)
    hipLaunchKernelGGL(anom_row_of, dim3(anomGrid(rows.k)), dim3(kAnomBlock), 0, st, rows.entities, rows.k, rowOf);
}

template <bool kSlow>
__global__ __launch_bounds__(kAnomBlock) void anom_history(AnomRows H, AnomRows C,
                                                           const int32_t* __restrict__ historyRowOf,
                                                           const uint8_t* __restrict__ interestedMetrics,
                                                           AnomPercentile pp, AnomSlow sp, uint32_t* __restrict__ flags,
                                                           AnomRecord* __restrict__ staged, AnomSlowScratch S) {
  __shared__ double col[kAnomMaxHistory * kAnomBlock];
  double* mine = col + threadIdx.x;
  const LdsColumn get{mine};
  const int slots = kSlow ? 2 : C.M;
  const int Wv = H.W < kAnomMaxHistory ? H.W : kAnomMaxHistory;  // H.W <= 31 by the aggregator's contract
  const long long items = C.k * slots;
  const long long stride = (long long)gridDim.x * kAnomBlock;
  for (long long base = (long long)blockIdx.x * kAnomBlock; base < items; base += stride) {  // wave-uniform
    const long long item = base + threadIdx.x;
    const bool live = item < items;
    bool active = false, skipped = false, nan = false;
    int s = 0;
    if (live) {
      const long long c = item / slots;
      s = (int)(item - c * slots);
      const int32_t e = C.entities[c];
      const long long h = historyRowOf[e];
      const float* cv = C.values + c * C.M;
      if (!kSlow) {
        uint32_t flag = 0;
        if (h >= 0 && interestedMetrics[s]) {
          const float* hv = H.values + (h * H.M + s) * H.W;
          for (int i = 0; i < Wv; ++i) mine[i * kAnomBlock] = (double)hv[i];
          const double u = pct::evaluate(get, Wv, pp.upper);
          if (!(u <= 1.0)) {  // SIGNIFICANT_METRIC_VALUE_THRESHOLD
            const double hi = u * (1.0 + pp.upperMargin);
            const double lo = pct::evaluate(get, Wv, pp.lower) * pp.lowerMargin;
            const double cur = (double)cv[s];
            if (cur > hi || cur < lo) {
              flag = 1;
              staged[item] = AnomRecord{e, s, cur, hi, lo};
            }
          }
        }
        flags[item] = flag;
      } else {
        // latest() is a Java float: the current bytes are a float sum, widened afterwards
        const float bytesF = cv[sp.mIn] + cv[sp.mRepl];
        const double bytes = (double)bytesF;
        skipped = bytes < sp.bytesThreshold;
        const double flush = (double)cv[sp.mFlush];
        const double cur = s == 0 ? flush : flush / bytes;
        bool hit = false;
        if (!skipped && h >= 0) {
          const float* hv = H.values + h * H.M * H.W;
          int n = 0;
          for (int i = 0; i < Wv; ++i) {  // doubleArray(): the history is widened first
            const double f = (double)hv[(long long)sp.mFlush * H.W + i];
            if (s == 0) {
              if (f > 5.0) mine[(n++) * kAnomBlock] = f;
            } else {
              const double total = (double)hv[(long long)sp.mIn * H.W + i] + (double)hv[(long long)sp.mRepl * H.W + i];
              if (total >= sp.bytesThreshold) mine[(n++) * kAnomBlock] = f / total;
            }
          }
          if (pct::isDataSufficient(n, sp.historyPercentile, sp.historyPercentile))
            hit = cur > pct::evaluate(get, n, sp.historyPercentile) * sp.historyMargin;
        }
        nan = !skipped && cur != cur;
        active = !skipped;
        S.cur[s * C.k + c] = cur;
        S.historyHit[s * C.k + c] = hit;
        if (s == 0) S.skipped[c] = skipped;
        SortEntry en;
        en.lo = (uint64_t)c;
        en.hi = skipped ? pct::kKeyNone : nan ? pct::kKeyNaN : pct::orderedKey(cur);
        S.sortA[s * C.k + c] = en;
      }
    }
    if (kSlow) {
      anomCount(&S.ctr[kAnActive], live && s == 0 && active ? 1 : 0);
      anomCount(&S.ctr[kAnSkipped], live && s == 0 && skipped ? 1 : 0);
      anomCount(&S.ctr[kAnNaNFlush], live && s == 0 && nan ? 1 : 0);
      anomCount(&S.ctr[kAnNaNPerByte], live && s == 1 && nan ? 1 : 0);
    }
  }
}

__global__ __launch_bounds__(kAnomScanBlock) void anom_scan(uint32_t* __restrict__ counts, int n) {
  const uint32_t total = scanCountsInPlace<uint32_t, kAnomScanBlock>(counts, n);
  if (threadIdx.x == 0) counts[n] = total;
}

void anomLaunchPercentile(const AnomRows& history, const AnomRows& current, const int32_t* historyRowOf,
                          const uint8_t* interestedMetrics, const AnomPercentile& p, uint32_t* flags, AnomRecord* staged,
                          hipStream_t st) {
  const long long items = current.k * current.M;
  hipLaunchKernelGGL(anom_history<false>, dim3(anomGrid(items)), dim3(kAnomBlock), 0, st, history, current, historyRowOf,
                     interestedMetrics, p, AnomSlow{}, flags, staged, AnomSlowScratch{});
  hipLaunchKernelGGL(anom_scan, dim3(1), dim3(kAnomScanBlock), 0, st, flags, (int)items);
}

__global__ __launch_bounds__(kAnomBlock) void anom_gather(const uint32_t* __restrict__ flags,
                                                          const AnomRecord* __restrict__ staged, long long items,
                                                          long long capacity, AnomRecord* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kAnomBlock;
  for (long long i = (long long)blockIdx.x * kAnomBlock + threadIdx.x; i < items; i += stride) {
    const uint32_t rank = flags[i];
    if (flags[i + 1] != rank && (long long)rank < capacity) out[rank] = staged[i];
  }
}

void anomLaunchGather(const uint32_t* flags, const AnomRecord* staged, long long items, long long capacity,
                      AnomRecord* out, hipStream_t st) {
  hipLaunchKernelGGL(anom_gather, dim3(anomGrid(items)), dim3(kAnomBlock), 0, st, flags, staged, items, capacity, out);
}

// ------------------------------------------------------------------------------------------------ slow brokers
__global__ __launch_bounds__(64) void anom_peer_base(AnomSlowScratch S, const SortEntry* __restrict__ sorted,
                                                     long long k, double peerPercentile) {
  const int s = (int)threadIdx.x;
  if (s >= 2) return;
  const int n = (int)S.ctr[kAnActive];
  const int nans = (int)S.ctr[kAnNaNFlush + s];
  const bool evaluated = pct::isDataSufficient(n, peerPercentile, peerPercentile);  // false for n < 2
  double base = pct::quietNaN();
  if (evaluated) {
    const SortEntry* seg = sorted + (long long)s * k;  // n <= k: the active rows sort first
    const double only = seg[0].hi == pct::kKeyNaN ? pct::quietNaN() : pct::fromOrderedKey(seg[0].hi);
    base = pct::evaluateSorted(SortedKeys{seg}, n - nans, n, only, peerPercentile);
  }
  S.base[s] = base;
  if (s == 0) S.ctr[kAnPeerEvaluated] = evaluated ? 1 : 0;
}

void anomLaunchSlowRows(const AnomRows& history, const AnomRows& current, const int32_t* historyRowOf,
                        const AnomSlow& p, const AnomSlowScratch& S, hipStream_t st) {
  (void)hipMemsetAsync(S.ctr, 0, sizeof(unsigned long long) * kAnomCtrWords, st);
  const long long k = current.k;
  const SortEntry* sorted = S.sortA;
  if (k > 0) {
    hipLaunchKernelGGL(anom_history<true>, dim3(anomGrid(2 * k)), dim3(kAnomBlock), 0, st, history, current,
                       historyRowOf, (const uint8_t*)nullptr, AnomPercentile{}, p, (uint32_t*)nullptr,
                       (AnomRecord*)nullptr, S);
    launchSegSort<AnomLess>(S.offsets, 2, 2 * k, k, S.sortA, S.sortB, st);
    if (segSortPasses(k) & 1) sorted = S.sortB;
  }
  hipLaunchKernelGGL(anom_peer_base, dim3(1), dim3(64), 0, st, S, sorted, k, p.peerPercentile);
}

__global__ __launch_bounds__(kAnomBlock) void anom_slow_update(AnomRows C, const int32_t* __restrict__ currentRowOf,
                                                               int32_t E, AnomSlow sp, AnomSlowScratch S,
                                                               AnomScores scores, long long timeMs,
                                                               uint32_t* __restrict__ flags, uint8_t* __restrict__ kind,
                                                               uint8_t* __restrict__ diag) {
  const bool peers = S.ctr[kAnPeerEvaluated] != 0;
  const double base0 = S.base[0], base1 = S.base[1];
  const long long stride = (long long)gridDim.x * kAnomBlock;
  for (long long b = (long long)blockIdx.x * kAnomBlock; b < E; b += stride) {  // wave-uniform
    const long long e = b + threadIdx.x;
    int scored = 0, demote = 0, remove = 0;
    if (e < E) {
      const long long c = currentRowOf[e];
      bool suspect = false;
      int d = 0;
      if (c >= 0) {
        if (S.skipped[c]) {
          d = kDiagSkipped;
        } else {
          const double flush = S.cur[c], perByte = S.cur[C.k + c];
          if (S.historyHit[c]) d |= kDiagFlushHistory;
          if (peers && flush > base0 * sp.peerMargin) d |= kDiagFlushPeers;
          if (S.historyHit[C.k + c]) d |= kDiagPerByteHistory;
          if (peers && perByte > base1 * sp.peerMargin) d |= kDiagPerBytePeers;
          if (flush > sp.flushThreshold) d |= kDiagOverThreshold;
          suspect = (d & (kDiagFlushHistory | kDiagFlushPeers)) && (d & (kDiagPerByteHistory | kDiagPerBytePeers)) &&
                    (d & kDiagOverThreshold);
          if (suspect) d |= kDiagSuspect;
        }
      }
      bool has = scores.has[e] != 0;
      int32_t score = scores.score[e];
      long long since = scores.since[e];
      if (suspect) {  // putIfAbsent(now); compute(v == null ? 1 : min(v + 1, decommission))
        if (!has) {
          has = true;
          since = timeMs;
          score = 1;
        } else {
          score = score + 1 < sp.decommission ? score + 1 : sp.decommission;
        }
      } else if (has) {  // --score == 0: recovered, out of both maps
        --score;
        if (score == 0) {
          has = false;
          since = 0;
        }
      }
      int kd = 0;
      if (suspect) kd = score == sp.decommission ? 2 : score >= sp.demotion ? 1 : 0;
      scores.has[e] = has;
      scores.score[e] = score;
      scores.since[e] = since;
      flags[e] = kd != 0;
      kind[e] = (uint8_t)kd;
      diag[e] = (uint8_t)d;
      scored = has;
      demote = kd == 1;
      remove = kd == 2;
    }
    anomCount(&S.ctr[kAnScored], scored);
    anomCount(&S.ctr[kAnDemote], demote);
    anomCount(&S.ctr[kAnRemove], remove);
  }
}

void anomLaunchSlowUpdate(const AnomRows& current, const int32_t* currentRowOf, int32_t E, const AnomSlow& p,
                          const AnomSlowScratch& S, const AnomScores& scores, long long timeMs, uint32_t* flags,
                          uint8_t* kind, uint8_t* diag, hipStream_t st) {
  hipLaunchKernelGGL(anom_slow_update, dim3(anomGrid(E)), dim3(kAnomBlock), 0, st, current, currentRowOf, E, p, S, scores,
                     timeMs, flags, kind, diag);
  hipLaunchKernelGGL(anom_scan, dim3(1), dim3(kAnomScanBlock), 0, st, flags, (int)E);
}

__global__ __launch_bounds__(kAnomBlock) void anom_score_flags(AnomScores scores, int32_t E, uint32_t* __restrict__ flags,
                                                               uint8_t* __restrict__ kind) {
  const long long stride = (long long)gridDim.x * kAnomBlock;
  for (long long e = (long long)blockIdx.x * kAnomBlock + threadIdx.x; e < E; e += stride) {
    flags[e] = scores.has[e] != 0;
    kind[e] = 0;
  }
}

void anomLaunchScoreFlags(const AnomScores& scores, int32_t E, uint32_t* flags, uint8_t* kind, hipStream_t st) {
  hipLaunchKernelGGL(anom_score_flags, dim3(anomGrid(E)), dim3(kAnomBlock), 0, st, scores, E, flags, kind);
  hipLaunchKernelGGL(anom_scan, dim3(1), dim3(kAnomScanBlock), 0, st, flags, (int)E);
}

__global__ __launch_bounds__(kAnomBlock) void anom_slow_gather(const uint32_t* __restrict__ flags,
                                                               const uint8_t* __restrict__ kind, AnomScores scores,
                                                               int32_t E, long long capacity,
                                                               AnomSlowRecord* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kAnomBlock;
  for (long long e = (long long)blockIdx.x * kAnomBlock + threadIdx.x; e < E; e += stride) {
    const uint32_t rank = flags[e];
    if (flags[e + 1] != rank && (long long)rank < capacity)
      out[rank] = AnomSlowRecord{(int32_t)e, (int32_t)kind[e], scores.score[e], 0, scores.since[e]};
  }
}

void anomLaunchSlowGather(const uint32_t* flags, const uint8_t* kind, const AnomScores& scores, int32_t E,
                          long long capacity, AnomSlowRecord* out, hipStream_t st) {
  hipLaunchKernelGGL(anom_slow_gather, dim3(anomGrid(E)), dim3(kAnomBlock), 0, st, flags, kind, scores, E, capacity, out);
}

}  // namespace ccmi
