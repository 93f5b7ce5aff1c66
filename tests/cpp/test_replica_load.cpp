// Host unit check of engine/replica_load.h, the header the K18 kernels compile (kernels/load_model.hip). Reads a script
// of partitions recorded from the oracle's restatement of MonitorUtils.populatePartitionLoad (oc_ingest_partition) and
// compares every replica's load bit for bit:
//   case <W> <n> <leaderIdx>
//   lead <6 * W float bit patterns, hex>          the aggregated leader metrics [6][W]
//   want <n * 6 * W float bit patterns, hex>      the replicas' loads [n][6][W]
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I cruise-control_amd/csrc/engine tests/cpp/test_replica_load.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "replica_load.h"

namespace {

float fromBits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
uint32_t toBits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

bool readHex(std::istringstream& in, size_t n, std::vector<uint32_t>& out) {
  out.clear();
  std::string tok;
  while (out.size() < n && (in >> tok)) out.push_back((uint32_t)std::stoul(tok, nullptr, 16));
  return out.size() == n && !(in >> tok);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s script\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  using namespace ccmi::rload;
  std::string line;
  long lineNo = 0, cases = 0, floats = 0;
  int W = 0, n = 0, leaderIdx = 0;
  std::vector<uint32_t> lead, want;
  while (std::getline(f, line)) {
    lineNo++;
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "case") {
      if (!(in >> W >> n >> leaderIdx) || W < 1 || W > 5 || n < 1 || n > kMaxReplicas || leaderIdx < 0 || leaderIdx >= n) {
        std::fprintf(stderr, "line %ld: bad case\n", lineNo);
        return 2;
      }
      lead.clear();
    } else if (kind == "lead") {
      if (!readHex(in, (size_t)kMetrics * W, lead)) {
        std::fprintf(stderr, "line %ld: bad lead\n", lineNo);
        return 2;
      }
    } else if (kind == "want") {
      if (lead.empty() || !readHex(in, (size_t)n * kMetrics * W, want)) {
        std::fprintf(stderr, "line %ld: bad want\n", lineNo);
        return 2;
      }
      for (int i = 0; i < n; ++i)
        for (int w = 0; w < W; ++w) {
          float in6[kMetrics], out6[kMetrics];
          for (int m = 0; m < kMetrics; ++m) in6[m] = fromBits(lead[(size_t)m * W + w]);
          replicaLoadWindow(in6, i, leaderIdx, n, out6);
          for (int m = 0; m < kMetrics; ++m) {
            const uint32_t expect = want[((size_t)i * kMetrics + m) * W + w];
            if (toBits(out6[m]) != expect) {
              std::fprintf(stderr, "line %ld: replica %d of %d (leader %d), metric %d, window %d: got %08x, want %08x\n",
                           lineNo, i, n, leaderIdx, m, w, toBits(out6[m]), expect);
              return 1;
            }
            floats++;
          }
        }
      cases++;
    } else {
      std::fprintf(stderr, "line %ld: unknown line %s\n", lineNo, kind.c_str());
      return 2;
    }
  }
  if (cases == 0) {
    std::fprintf(stderr, "empty script\n");
    return 2;
  }
  std::printf("replica load ok: %ld partitions, %ld floats\n", cases, floats);
  return 0;
}
