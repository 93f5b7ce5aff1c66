// Host unit check of engine/percentile.h, the header the K19 kernels compile: replays cases the Python restatement
// (tests/metric_anomaly_support.py) recorded and compares bit for bit (NaNs as one, -0.0 as 0.0: Percentile selects with
// <, so the sign of a zero is not determined). Build: g++ -O1 -std=c++17 -ffp-contract=off. Lines of the script:
//   pct <p> <n> <value>*n <expected>     evaluate, and evaluateSorted over the sorted non-NaN values
//   min <p> <expected int>               minNumValues
//   suf <count> <upper> <lower> <0|1>    isDataSufficient
// doubles are hexadecimal bit patterns.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "percentile.h"

namespace {

double fromBits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

uint64_t canonical(double d) {
  if (d != d) return 0x7ff8000000000000ull;
  if (d == 0.0) return 0;
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

double readDouble(std::istringstream& in) {
  std::string w;
  in >> w;
  return fromBits(std::stoull(w, nullptr, 16));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  std::string line;
  long lineNo = 0, checked = 0;
  while (std::getline(f, line)) {
    lineNo++;
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "pct") {
      const double p = readDouble(in);
      int n;
      in >> n;
      std::vector<double> v((size_t)n);
      for (double& x : v) x = readDouble(in);
      const double want = readDouble(in);
      const double got = ccmi::pct::evaluate([&](int i) { return v[(size_t)i]; }, n, p);
      std::vector<double> sorted;
      for (double x : v)
        if (x == x) sorted.push_back(x);
      // through the ordered keys, as the peer percentile of the kernels sorts them
      std::vector<uint64_t> keys;
      for (double x : sorted) keys.push_back(ccmi::pct::orderedKey(x));
      std::sort(keys.begin(), keys.end());
      const double got2 = ccmi::pct::evaluateSorted([&](int i) { return ccmi::pct::fromOrderedKey(keys[(size_t)i]); },
                                                    (int)keys.size(), n, n ? v[0] : 0.0, p);
      for (size_t i = 0; i < keys.size(); ++i)
        if (keys[i] >= ccmi::pct::kKeyNaN) {
          std::fprintf(stderr, "line %ld: a number's key reaches the NaN key\n", lineNo);
          return 1;
        }
      if (canonical(got) != canonical(want) || canonical(got2) != canonical(want)) {
        std::fprintf(stderr, "line %ld: evaluate %a / sorted %a, expected %a\n", lineNo, got, got2, want);
        return 1;
      }
    } else if (op == "min") {
      const double p = readDouble(in);
      long long want;
      in >> want;
      if (ccmi::pct::minNumValues(p) != want) {
        std::fprintf(stderr, "line %ld: minNumValues %d, expected %lld\n", lineNo, ccmi::pct::minNumValues(p), want);
        return 1;
      }
    } else if (op == "suf") {
      int count, want;
      in >> count;
      const double upper = readDouble(in), lower = readDouble(in);
      in >> want;
      if ((int)ccmi::pct::isDataSufficient(count, upper, lower) != want) {
        std::fprintf(stderr, "line %ld: isDataSufficient disagrees\n", lineNo);
        return 1;
      }
    } else if (!op.empty()) {
      std::fprintf(stderr, "line %ld: unknown op %s\n", lineNo, op.c_str());
      return 2;
    } else {
      continue;
    }
    checked++;
  }
  std::printf("percentile ok: %ld cases\n", checked);
  return checked ? 0 : 1;
}
