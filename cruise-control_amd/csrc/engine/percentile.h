// The percentile of K19 (ccmi_aggregator_metric_anomalies, ccmi_slow_broker_finder), written once for the device kernels
// (kernels/anomaly.hip) and for the host unit test (tests/cpp/test_percentile.cpp): commons-math3 3.6.1's
// stat.descriptive.rank.Percentile with its defaults (LEGACY estimation, NaNStrategy.REMOVED), and
// PercentileMetricAnomalyFinderUtils.isDataSufficient of cruise-control-core.
//
// evaluate(p) over n values, p in (0, 100]:
//   n == 0 -> NaN; n == 1 -> that value (a NaN too); the NaNs are dropped (none left -> NaN), n = what remains;
//   pos = (p / 100) * (n + 1), divided first, in double; p / 100 == 1 makes pos exactly n;
//   pos < 1 -> the minimum; pos >= n -> the maximum;
//   else k = (int) floor(pos), d = pos - floor(pos): sorted[k - 1] + d * (sorted[k] - sorted[k - 1]).
// The library selects with <, so -0.0 and 0.0 are interchangeable as order statistics.
// Values come through an accessor `get(i)` (an LDS column on the device, a vector on the host), never through an
// indexed private array. Compile with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CCMI_PCT __host__ __device__ __forceinline__
#else
#define CCMI_PCT inline
#endif

namespace ccmi {
namespace pct {

constexpr int kIntMax = 0x7fffffff;  // Java's (int) of +Infinity

CCMI_PCT double quietNaN() { return __builtin_nan(""); }

// (int) Math.ceil(100 / (p > 50.0 ? 100 - p : p)): Integer.MAX_VALUE for p = 0 and p = 100 (a division by zero in
// double), decided before the division so that no infinity is ever cast; a negative quotient (p outside [0, 100])
// saturates as Java's cast does.
CCMI_PCT int minNumValues(double p) {
  const double den = p > 50.0 ? 100.0 - p : p;
  if (den != den) return 0;  // (int) NaN
  if (den == 0.0) return kIntMax;
  const double q = ceil(100.0 / den);
  if (q >= 2147483647.0) return kIntMax;
  if (q <= -2147483648.0) return -kIntMax - 1;
  return (int)q;
}

// PercentileMetricAnomalyFinderUtils.isDataSufficient
CCMI_PCT bool isDataSufficient(int sampleCount, double upperPercentile, double lowerPercentile) {
  const int a = minNumValues(upperPercentile), b = minNumValues(lowerPercentile);
  return sampleCount >= (a > b ? a : b);
}

// Where the percentile sits among n sorted values (n >= 1, none of them NaN): 0 = the minimum, 1 = the maximum,
// 2 = between sorted[*k - 1] and sorted[*k] at the fraction *d.
CCMI_PCT int position(double p, int n, int* k, double* d) {
  const double q = p / 100.0;
  const double pos = q == 1.0 ? (double)n : q * (double)(n + 1);
  *k = 0;
  *d = 0.0;
  if (pos < 1.0) return 0;
  if (pos >= (double)n) return 1;
  const double f = floor(pos);
  *k = (int)f;
  *d = pos - f;
  return 2;
}

// the value of rank r (0-based) among the non-NaN values of get(0 .. n), by counting: v has rank r iff
// #(w < v) <= r < #(w <= v). A NaN compares false either way, so it neither counts nor is chosen.
template <class Get>
CCMI_PCT double selectRank(const Get& get, int n, int r) {
  double out = quietNaN();
  for (int i = 0; i < n; ++i) {
    const double v = get(i);
    int less = 0, leq = 0;
    for (int j = 0; j < n; ++j) {
      const double w = get(j);
      less += w < v ? 1 : 0;
      leq += w <= v ? 1 : 0;
    }
    if (less <= r && r < leq) out = v;
  }
  return out;
}

// Percentile.evaluate(p) over get(0 .. n), NaNs included in n.
template <class Get>
CCMI_PCT double evaluate(const Get& get, int n, double p) {
  if (n == 0) return quietNaN();
  if (n == 1) return get(0);
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const double v = get(i);
    m += v == v ? 1 : 0;
  }
  if (m == 0) return quietNaN();
  int k;
  double d;
  const int where = position(p, m, &k, &d);
  if (where == 0) return selectRank(get, n, 0);
  if (where == 1) return selectRank(get, n, m - 1);
  const double lo = selectRank(get, n, k - 1), hi = selectRank(get, n, k);
  return lo + d * (hi - lo);
}

// The same over values that are sorted already with the NaNs taken out: sorted(0 .. m) ascending, n = m + the NaNs
// dropped, `only` = the single value when n == 1 (it may be the NaN).
template <class Get>
CCMI_PCT double evaluateSorted(const Get& sorted, int m, int n, double only, double p) {
  if (n == 0) return quietNaN();
  if (n == 1) return only;
  if (m == 0) return quietNaN();
  int k;
  double d;
  const int where = position(p, m, &k, &d);
  if (where == 0) return sorted(0);
  if (where == 1) return sorted(m - 1);
  const double lo = sorted(k - 1), hi = sorted(k);
  return lo + d * (hi - lo);
}

// An order-preserving 64-bit key of a double that is not NaN (-0.0 sorts just below 0.0), and its inverse.
CCMI_PCT uint64_t orderedKey(double v) {
  union {
    double d;
    uint64_t u;
  } c;
  c.d = v;
  return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
CCMI_PCT double fromOrderedKey(uint64_t key) {
  union {
    double d;
    uint64_t u;
  } c;
  c.u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return c.d;
}
constexpr uint64_t kKeyNaN = 0xfffffffffffffffeull;   // behind every number (+Infinity is 0xfff0000000000000)
constexpr uint64_t kKeyNone = 0xffffffffffffffffull;  // no value at all: last

}  // namespace pct
}  // namespace ccmi
