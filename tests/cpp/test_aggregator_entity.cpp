// Host unit check of engine/aggregator_entity.h, the text the K17 kernels compile too: replays scripts of RawMetricValues
// calls and compares counts, validity and extrapolation bits and aggregated floats bit for bit with what the Python
// restatement (tests/metric_aggregator_support.py) recorded into the script. Stand-alone: g++ only, no HIP.
//
// Script (whitespace-separated tokens), one per line:
//   case KEEP MIN_SAMPLES M F0..F(M-1)      a new RawMetricValues
//   oldest W                                updateOldestWindowIndex
//   add W D0..D(M-1)                        addSample; the doubles as 64-bit patterns in hex
//   reset START N                           resetWindowIndices
//   state C0..C(KEEP-1) VALID EXTRAP        expected counts and bit words
//   values A F0..F(M-1)                     expected stored floats of array index A (32-bit patterns in hex)
//   isvalid MAX 0|1                         expected isValid(MAX)
//   agg N W0..W(N-1) X0..X(N-1) F[m][i]...  expected aggregate: codes, then M * N float patterns
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "aggregator_entity.h"

using namespace ccmi::agg;

static uint32_t bitsOf(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (f != f) ? 0x7fc00000u : u;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s script\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  std::vector<uint8_t> counts, fn;
  std::vector<float> values;
  RawView r{};
  long checks = 0, lineNo = 0, cases = 0;
  auto fail = [&](const char* what) {
    std::fprintf(stderr, "line %ld: %s mismatch: %s\n", lineNo, what, line.c_str());
    return 1;
  };
  while (std::getline(in, line)) {
    lineNo++;
    std::istringstream ss(line);
    std::string op;
    if (!(ss >> op)) continue;
    if (op == "case") {
      int keep, minS, M;
      ss >> keep >> minS >> M;
      fn.assign(M, 0);
      for (int m = 0; m < M; ++m) {
        int f;
        ss >> f;
        fn[m] = (uint8_t)f;
      }
      counts.assign(keep, 0);
      values.assign((size_t)keep * M, 0.0f);
      r = RawView{};
      r.counts = counts.data();
      r.values = values.data();
      r.countStride = 1;
      r.windowStride = M;
      r.metricStride = 1;
      r.fn = fn.data();
      r.oldest = kFresh;
      r.L = keep;
      r.M = M;
      r.minSamples = minS;
      r.halfMin = halfMinRequired(minS);
      cases++;
    } else if (op == "oldest") {
      long long w;
      ss >> w;
      updateOldestWindowIndex(r, w);
    } else if (op == "add") {
      long long w;
      ss >> w;
      std::vector<double> v(r.M);
      for (int m = 0; m < r.M; ++m) {
        uint64_t u;
        ss >> std::hex >> u >> std::dec;
        std::memcpy(&v[m], &u, 8);
      }
      addSample(r, w, v.data());
    } else if (op == "reset") {
      long long start;
      int n;
      ss >> start >> n;
      resetWindowIndices(r, start, n);
    } else if (op == "state") {
      for (int a = 0; a < r.L; ++a) {
        int c;
        ss >> c;
        if (c != (int)counts[a]) return fail("count");
      }
      uint32_t v, x;
      ss >> v >> x;
      if (v != r.valid) return fail("validity");
      if (x != r.extrap) return fail("extrapolation");
      int total = 0;
      for (int a = 0; a < r.L; ++a) total += counts[a];
      if (total != numSamples(r)) return fail("numSamples");
      checks++;
    } else if (op == "values") {
      int a;
      ss >> a;
      for (int m = 0; m < r.M; ++m) {
        uint32_t u;
        ss >> std::hex >> u >> std::dec;
        if (u != bitsOf(values[(size_t)a * r.M + m])) return fail("stored value");
      }
      checks++;
    } else if (op == "isvalid") {
      int mx, want;
      ss >> mx >> want;
      if ((int)isValid(r, mx) != want) return fail("isValid");
      checks++;
    } else if (op == "agg") {
      int n;
      ss >> n;
      std::vector<long long> w(n);
      for (auto& x : w) ss >> x;
      std::vector<int> codes(n);
      for (auto& x : codes) ss >> x;
      std::vector<float> out((size_t)r.M * n);
      for (int i = 0; i < n; ++i)
        if (aggregateWindow(r, w[i], out.data() + i, n) != codes[i]) return fail("extrapolation code");
      for (size_t k = 0; k < out.size(); ++k) {
        uint32_t u;
        ss >> std::hex >> u >> std::dec;
        if (u != bitsOf(out[k])) return fail("aggregated float");
      }
      checks++;
    } else {
      return fail("unknown op");
    }
  }
  if (cases == 0 || checks == 0) {
    std::fprintf(stderr, "empty script\n");
    return 1;
  }
  std::printf("aggregator entity ok: %ld cases, %ld checks\n", cases, checks);
  return 0;
}
