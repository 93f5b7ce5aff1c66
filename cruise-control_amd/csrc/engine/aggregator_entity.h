// The per-entity half of K17 (ccmi_aggregator), written once for the device kernels (kernels/aggregator.hip) and for
// the host unit test (tests/cpp/test_aggregator_entity.cpp): RawMetricValues and the WindowIndexedArrays it extends
// (cruise-control-core monitor/sampling/aggregator/RawMetricValues.java, common/WindowIndexedArrays.java), transcribed
// method by method. The validity and extrapolation bits are a state machine over the calls an entity has seen (the
// !_extrapolations.get(i) short-circuit, the edge rules around the current window); nothing here derives them from the
// counts. RawView::oldest is the entity's own _oldestWindowIndex, so currentWindowIndex() is oldest + length - 1, which
// early in an aggregator's life is ahead of the aggregator's current window.
//
// Arithmetic types are Java's: a stored value is the (float) of a double expression; values[i] / counts[i] is a float
// division; the AVG_ADJACENT total is a float sum widened to double, divided in double and rounded to float once.
// Compile with -ffp-contract=off.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CCMI_AGG __host__ __device__ __forceinline__
#else
#define CCMI_AGG inline
#endif

namespace ccmi {
namespace agg {

constexpr int kFnAvg = 0, kFnMax = 1, kFnLatest = 2;  // AggregationFunction, ccmi_aggregation_function
// Extrapolation.java in declaration order
constexpr int kExNone = 0, kExAvgAvailable = 1, kExAvgAdjacent = 2, kExForcedInsufficient = 3, kExNoValid = 4;
constexpr int kMaxKeep = 32;                     // windows kept (num_windows + 1): one bit each in a 32-bit word
constexpr int kInvalidIndex = -1;                // WindowIndexedArrays.INVALID_INDEX
constexpr long long kFresh = 0x7fffffffffffffffLL;  // _oldestWindowIndex of a new RawMetricValues (Long.MAX_VALUE)

// One entity's RawMetricValues over strided storage: counts[a * countStride], values[a * windowStride + m *
// metricStride] for array index a and metric m (the device lays both out entity-minor, the host test densely).
struct RawView {
  uint8_t* counts;
  float* values;
  long long countStride, windowStride, metricStride;
  const uint8_t* fn;  // [M] aggregation function per metric
  long long oldest;   // _oldestWindowIndex
  uint32_t valid, extrap;  // _validity, _extrapolations: bit a = array index a
  int L, M, minSamples, halfMin;  // length(), metrics, _minSamplesPerWindow, _halfMinRequiredSamples
};

CCMI_AGG int halfMinRequired(int minSamples) { return minSamples / 2 > 1 ? minSamples / 2 : 1; }

CCMI_AGG int cnt(const RawView& r, int a) { return (int)r.counts[(long long)a * r.countStride]; }
CCMI_AGG float& val(const RawView& r, int a, int m) {
  return r.values[(long long)a * r.windowStride + (long long)m * r.metricStride];
}
CCMI_AGG bool bit(uint32_t w, int a) { return (w >> a) & 1u; }
CCMI_AGG int popcount32(uint32_t w) {
  int n = 0;
  for (; w; w &= w - 1) n++;
  return n;
}

// ---- WindowIndexedArrays
CCMI_AGG int arrayIndex(const RawView& r, long long windowIndex) { return (int)(windowIndex % r.L); }
CCMI_AGG long long currentWindowIndex(const RawView& r) { return r.oldest + r.L - 1; }
CCMI_AGG long long lastWindowIndex(const RawView& r) { return currentWindowIndex(r) - 1; }
CCMI_AGG int firstArrayIndex(const RawView& r) { return arrayIndex(r, r.oldest); }
CCMI_AGG int lastArrayIndex(const RawView& r) { return arrayIndex(r, lastWindowIndex(r)); }
CCMI_AGG int prevArrayIndex(const RawView& r, int a) {
  return a == firstArrayIndex(r) ? kInvalidIndex : (a + r.L - 1) % r.L;
}
CCMI_AGG int nextArrayIndex(const RawView& r, int a) { return a == lastArrayIndex(r) ? kInvalidIndex : (a + 1) % r.L; }
CCMI_AGG bool inValidWindowRange(const RawView& r, long long w) { return w >= r.oldest && w <= lastWindowIndex(r); }

// ---- RawMetricValues: the bits
CCMI_AGG void resetValidityAndExtrapolation(RawView& r, int a) {
  r.valid &= ~(1u << a);
  r.extrap &= ~(1u << a);
}
CCMI_AGG bool updateEnoughSamples(RawView& r, int a) {
  if (cnt(r, a) == r.minSamples) {
    r.valid |= 1u << a;
    r.extrap &= ~(1u << a);
    return true;
  }
  return cnt(r, a) >= r.minSamples;
}
CCMI_AGG bool updateAvgAdjacent(RawView& r, int a) {
  const int p = prevArrayIndex(r, a), n = nextArrayIndex(r, a);
  if (p == kInvalidIndex || n == kInvalidIndex) return false;
  if (cnt(r, p) >= r.minSamples && cnt(r, n) >= r.minSamples) {
    r.valid |= 1u << a;
    r.extrap |= 1u << a;
    return true;
  }
  return false;
}
CCMI_AGG bool updateForcedInsufficient(RawView& r, int a) {
  if (cnt(r, a) > 0) {
    r.valid |= 1u << a;
    r.extrap |= 1u << a;
    return true;
  }
  return false;
}
CCMI_AGG void maybeUpdateValidityAndExtrapolationFor(RawView& r, int a) {
  if (!updateEnoughSamples(r, a) && !bit(r.extrap, a) && !updateForcedInsufficient(r, a) && !updateAvgAdjacent(r, a))
    resetValidityAndExtrapolation(r, a);
}
CCMI_AGG bool hasTwoLeftNeighbours(const RawView& r, int a) {
  const int p = prevArrayIndex(r, a);
  return p != kInvalidIndex && prevArrayIndex(r, p) != kInvalidIndex;
}
CCMI_AGG bool hasTwoRightNeighbours(const RawView& r, int a) {
  const int n = nextArrayIndex(r, a);
  return n != kInvalidIndex && nextArrayIndex(r, n) != kInvalidIndex;
}
CCMI_AGG void maybeUpdateValidityAndExtrapolationOfPrevAndNextFor(RawView& r, int a) {
  if (cnt(r, a) >= r.minSamples) {
    if (a != arrayIndex(r, currentWindowIndex(r)) && hasTwoLeftNeighbours(r, a)) {
      const int p = prevArrayIndex(r, a);
      if (cnt(r, p) == 0) updateAvgAdjacent(r, p);
    }
    if (hasTwoRightNeighbours(r, a)) {
      const int n = nextArrayIndex(r, a);
      if (cnt(r, n) == 0) updateAvgAdjacent(r, n);
    }
  }
}

// Math.max(double, double): a NaN wins, and -0.0 < 0.0
CCMI_AGG double javaMax(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  if (a == 0.0 && b == 0.0) {
    union {
      double d;
      uint64_t u;
    } ua;
    ua.d = a;
    return (ua.u >> 63) ? b : a;
  }
  return a > b ? a : b;
}

// ---- RawMetricValues: the calls
// addSample(sample, windowIndex, metricDef); sample[m] is the sample's double of metric m. Returns false when the
// sample is dropped (older than the oldest window). A window index above currentWindowIndex() is the reference's
// IllegalArgumentException; the aggregator never produces one, and it is dropped here.
CCMI_AGG bool addSample(RawView& r, long long windowIndex, const double* sample) {
  if (windowIndex < r.oldest || windowIndex > currentWindowIndex(r)) return false;
  const int a = arrayIndex(r, windowIndex);
  const int c = cnt(r, a);
  for (int m = 0; m < r.M; ++m) {
    float& v = val(r, a, m);
    const double nv = sample[m];
    switch (r.fn[m]) {
      case kFnAvg:
        v = (float)(c == 0 ? nv : (double)v + nv);
        break;
      case kFnMax:
        v = (float)(c == 0 ? nv : javaMax((double)v, nv));
        break;
      default:
        v = (float)nv;
        break;
    }
  }
  r.counts[(long long)a * r.countStride] = (uint8_t)(c + 1);
  maybeUpdateValidityAndExtrapolationFor(r, a);
  maybeUpdateValidityAndExtrapolationOfPrevAndNextFor(r, a);
  return true;
}

// updateOldestWindowIndex(newOldestWindowIndex). On a new RawMetricValues lastWindowIndex() overflows to a negative
// number in Java and the test below it is false: the same here without the overflow.
CCMI_AGG void updateOldestWindowIndex(RawView& r, long long newOldest) {
  const bool fresh = r.oldest == kFresh;
  const long long prevLast = fresh ? 0 : lastWindowIndex(r);
  r.oldest = newOldest;
  if (!fresh && prevLast >= r.oldest) maybeUpdateValidityAndExtrapolationFor(r, arrayIndex(r, prevLast));
}

// resetWindowIndices(startingWindowIndex, numWindowIndicesToReset); returns the abandoned samples
CCMI_AGG int resetWindowIndices(RawView& r, long long start, int n) {
  int abandoned = 0;
  for (long long i = start; i < start + n; ++i) {
    const int a = arrayIndex(r, i);
    abandoned += cnt(r, a);
    r.counts[(long long)a * r.countStride] = 0;
    resetValidityAndExtrapolation(r, a);
  }
  return abandoned;
}

CCMI_AGG bool isValid(const RawView& r, int maxAllowedWindowsWithExtrapolation) {
  const int cur = arrayIndex(r, currentWindowIndex(r));
  const bool allValid = popcount32(r.valid) - (bit(r.valid, cur) ? 1 : 0) == r.L - 1;
  const int numExtrap = popcount32(r.extrap) - (bit(r.extrap, cur) ? 1 : 0);
  return allValid && numExtrap <= maxAllowedWindowsWithExtrapolation;
}

CCMI_AGG int numSamples(const RawView& r) {
  int n = 0;
  for (int a = 0; a < r.L; ++a) n += cnt(r, a);
  return n;
}

CCMI_AGG float getValue(const RawView& r, int m, int a) {
  if (cnt(r, a) == 0) return 0.0f;
  return r.fn[m] == kFnAvg ? val(r, a, m) / (float)cnt(r, a) : val(r, a, m);
}

// One window of aggregate(windowIndices, metricDef): out[m * outStride] gets the float of metric m, the return value is
// the window's Extrapolation. The window check of the reference is the caller's (peekCurrentWindow skips it).
CCMI_AGG int aggregateWindow(const RawView& r, long long windowIndex, float* out, long long outStride) {
  const int a = arrayIndex(r, windowIndex);
  const int c = cnt(r, a);
  if (c >= r.halfMin) {
    for (int m = 0; m < r.M; ++m) out[m * outStride] = getValue(r, m, a);
    return c < r.minSamples ? kExAvgAvailable : kExNone;
  }
  if (a != firstArrayIndex(r) && a != lastArrayIndex(r) && cnt(r, prevArrayIndex(r, a)) >= r.minSamples &&
      cnt(r, nextArrayIndex(r, a)) >= r.minSamples) {
    const int p = prevArrayIndex(r, a), n = nextArrayIndex(r, a);
    for (int m = 0; m < r.M; ++m) {
      const float mid = c == 0 ? 0.0f : val(r, a, m);
      const float ftotal = (val(r, p, m) + mid) + val(r, n, m);
      const double total = (double)ftotal;
      out[m * outStride] = r.fn[m] == kFnAvg ? (float)(total / (double)(cnt(r, p) + c + cnt(r, n)))
                                             : (float)(total / (double)(c > 0 ? 3 : 2));
    }
    return kExAvgAdjacent;
  }
  if (c > 0) {
    for (int m = 0; m < r.M; ++m) out[m * outStride] = getValue(r, m, a);
    return kExForcedInsufficient;
  }
  for (int m = 0; m < r.M; ++m) out[m * outStride] = 0.0f;
  return kExNoValid;
}

}  // namespace agg
}  // namespace ccmi
