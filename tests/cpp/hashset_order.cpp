// The iteration order of a JDK 11 HashSet from jsem.h's JHashSet (tree bins included), for the K20 tests.
// stdin: "<S|R> <n>", then n lines "<hashCode> <name>" in insertion order. S: equal hashes in a tree bin compare by
// name (String.compareTo on bytes); R: by insertion rank (TopicPartition is not Comparable: the JVM falls back to
// identity hashes there). stdout: the n indices in iteration order.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "jsem.h"

struct Ops {
  const std::vector<std::string>* names;
  bool byName;
  int cmp(int a, int b) const {
    if (!byName) return a < b ? -1 : a > b ? 1 : 0;
    const int c = (*names)[a].compare((*names)[b]);
    return c < 0 ? -1 : c > 0 ? 1 : 0;
  }
};

int main() {
  std::string mode;
  int n = 0;
  if (!(std::cin >> mode >> n)) return 2;
  std::vector<std::string> names(n);
  std::vector<int32_t> hashes(n);
  for (int i = 0; i < n; ++i) {
    long long h;
    if (!(std::cin >> h >> names[i])) return 2;
    hashes[i] = (int32_t)h;
  }
  const Ops ops{&names, mode == "S"};
  ccmi::JHashSet<Ops> set(&ops);
  for (int i = 0; i < n; ++i) set.add(i, hashes[i]);
  std::vector<int32_t> order;
  set.order(order);
  for (int32_t i : order) std::printf("%d\n", i);
  return 0;
}
