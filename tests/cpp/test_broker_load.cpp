// engine/broker_load.h built for the host: answers the queries of tests/test_broker_load_cpp.py, one per line on stdin.
// Doubles travel as the hex of their bits, so nothing is rounded on the way.
//   avg n v..            -> value            ValueAndCount over v in order
//   latest n (t v)..     -> value            ValueAndTime over (time, value) in order
//   convert type v       -> value            HolderUtils.convertUnit
//   cpu w0 w1 w2 cpu in out fol pin pout -> value | null     estimateLeaderCpuUtilPerCore
//   version follower enough availHex     -> version minRequired availHex      maybeSetBrokerRawMetrics and the rest
//   enough mt t mp led   -> 0 | 1            enoughTopicPartitionMetrics
//   tphash topicHash partition -> int        TopicPartition.hashCode
//   order n (hash)..     -> flagged idx..    keys in insertion order -> the list-bin iteration order
//   def type             -> metric def id
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "broker_load.h"

namespace bl = ccmi::bl;

static double rd() {
  std::string s;
  std::cin >> s;
  const uint64_t u = std::stoull(s, nullptr, 16);
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}
static void wr(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  std::printf("%016" PRIx64 "\n", u);
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "avg" || cmd == "latest") {
      const bool latest = cmd == "latest";
      int n;
      std::cin >> n;
      bl::Holder h;
      bl::holderReset(h);
      for (int i = 0; i < n; ++i) {
        long long t = 0;
        if (latest) std::cin >> t;
        const double v = rd();
        bl::holderRecord(h, latest, v, t);
      }
      wr(bl::holderValue(h, latest));
    } else if (cmd == "convert") {
      int t;
      std::cin >> t;
      wr(bl::convertUnit(rd(), t));
    } else if (cmd == "cpu") {
      bl::CpuWeights w;
      w.leaderBytesIn = rd();
      w.leaderBytesOut = rd();
      w.followerBytesIn = rd();
      double a[6], out;
      for (double& x : a) x = rd();
      if (bl::cpuUtilPerCore(w, a[0], a[1], a[2], a[3], a[4], a[5], &out)) wr(out);
      else std::printf("null\n");
    } else if (cmd == "version") {
      int follower, enough;
      std::string hex;
      std::cin >> follower >> enough >> hex;
      bl::Prepared p{};
      p.avail = std::stoull(hex, nullptr, 16);
      p.enough = enough;
      bl::versionLogic(p, follower != 0);
      std::printf("%d %d %016" PRIx64 "\n", p.version, p.minRequired, (uint64_t)p.avail);
    } else if (cmd == "enough") {
      int mt, t, mp, led;
      std::cin >> mt >> t >> mp >> led;
      std::printf("%d\n", bl::enoughMetrics(mt, t, mp, led) ? 1 : 0);
    } else if (cmd == "tphash") {
      int th, part;
      std::cin >> th >> part;
      std::printf("%d\n", bl::topicPartitionHash(th, part));
    } else if (cmd == "def") {
      int t;
      std::cin >> t;
      std::printf("%d\n", bl::metricDefOf(t));
    } else if (cmd == "order") {
      int n;
      std::cin >> n;
      std::vector<uint32_t> h(n);
      for (int i = 0; i < n; ++i) {
        int x;
        std::cin >> x;
        h[i] = bl::spread(x);
      }
      // what mp_hash_order does per key: rank = i here (the keys come in insertion order)
      const uint32_t capFinal = bl::tableCapacity((uint32_t)n);
      std::vector<int> order(n, -1);
      bool flagged = false;
      for (int i = 0; i < n; ++i) {
        const uint32_t capAt = bl::tableCapacity((uint32_t)i);
        uint32_t earlier = 0, pos = 0;
        for (int j = 0; j < n; ++j) {
          if (j < i && bl::sameBucket(h[j], h[i], capAt)) earlier++;
          if (j != i && bl::iteratesBefore(h[j], (uint32_t)j, h[i], (uint32_t)i, capFinal)) pos++;
        }
        order[pos] = i;
        flagged |= bl::binFlagged(earlier);
      }
      std::printf("%d", flagged ? 1 : 0);
      for (int i : order) std::printf(" %d", i);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
