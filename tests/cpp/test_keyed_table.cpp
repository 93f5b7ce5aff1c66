// Unit checks of engine/keyed_table.h (built and run by tests/test_keyed_table_cpp.py, CPU only): random insert, key
// update and remove sequences on the mirror against a sorted reference (one std::map per broker), with a shadow of the
// device table fed only by the writes the mirror hands out — so a missing row or length write shows as a difference
// between the shadow and the reference. Covers the slot bookkeeping, the full block (upsert refused, nothing changed),
// the "rows below a key" count and the sorted view.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "keyed_table.h"

using namespace ccmi;

static int fails = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
      ++fails;                           \
    }                                    \
  } while (0)

struct Shadow {  // what the device would hold after the writes
  int stride;
  std::vector<int32_t> len, rep;
  std::vector<uint64_t> key;
  Shadow(int B, int s) : stride(s), len(B, 0), rep((size_t)B * s, -1), key((size_t)B * s, 0) {}
  void row(const KeyedMirror::Write& w) {
    rep[(size_t)w.b * stride + w.slot] = w.rep;
    key[(size_t)w.b * stride + w.slot] = w.key;
  }
};

static void compare(const KeyedMirror& m, const Shadow& sh, const std::vector<std::map<uint64_t, int>>& ref, int B,
                    int R, std::mt19937_64& rng, int step) {
  for (int b = 0; b < B; ++b) {
    CHECK(m.len(b) == (int)ref[b].size(), "step %d broker %d: len %d, reference %zu", step, b, m.len(b), ref[b].size());
    CHECK(sh.len[b] == m.len(b), "step %d broker %d: device length %d, mirror %d", step, b, sh.len[b], m.len(b));
    std::map<uint64_t, int> got;
    for (int s = 0; s < m.len(b); ++s) {
      CHECK(sh.rep[(size_t)b * sh.stride + s] == m.rep(b, s) && sh.key[(size_t)b * sh.stride + s] == m.key(b, s),
            "step %d broker %d slot %d: device row differs from the mirror", step, b, s);
      CHECK(m.slotOf(m.rep(b, s)) == s && m.brokerOf(m.rep(b, s)) == b, "step %d broker %d slot %d: replica's slot", step,
            b, s);
      got[m.key(b, s)] = m.rep(b, s);
    }
    CHECK(got == ref[b], "step %d broker %d: rows differ from the reference", step, b);
    // the sorted view and the rows-below count at every key, between keys and at the ends
    std::vector<int32_t> v;
    m.sorted(b, v);
    size_t i = 0;
    for (const auto& e : ref[b]) {
      CHECK(i < v.size() && v[i] == e.second, "step %d broker %d: sorted view at %zu", step, b, i);
      CHECK(m.below(b, e.first) == (int)i, "step %d broker %d: below(key of row %zu) = %d", step, b, i, m.below(b, e.first));
      CHECK(m.below(b, e.first + 1) == (int)i + 1, "step %d broker %d: below(key + 1) of row %zu", step, b, i);
      CHECK(m.atOrBelow(b, e.first) == (int)i + 1, "step %d broker %d: atOrBelow(key of row %zu)", step, b, i);
      ++i;
    }
    CHECK(m.atOrBelow(b, ~0ull) == (int)ref[b].size(), "step %d broker %d: atOrBelow(the largest key)", step, b);
    CHECK(v.size() == ref[b].size(), "step %d broker %d: sorted view size", step, b);
    CHECK(m.below(b, 0) == 0 && m.below(b, ~0ull) == (int)ref[b].size(), "step %d broker %d: below at the ends", step, b);
    const uint64_t probe = rng() >> 20;
    int want = 0;
    for (const auto& e : ref[b]) want += e.first < probe ? 1 : 0;
    CHECK(m.below(b, probe) == want, "step %d broker %d: below(random key)", step, b);
  }
  int placed = 0;
  for (int r = 0; r < R; ++r) placed += m.brokerOf(r) >= 0 ? 1 : 0;
  size_t total = 0;
  for (int b = 0; b < B; ++b) total += ref[b].size();
  CHECK((size_t)placed == total, "step %d: %d replicas placed, reference %zu", step, placed, total);
}

int main() {
  const int B = 7, R = 90, stride = 12;  // stride below R / B * 2: blocks fill up and upserts are refused
  std::mt19937_64 rng(20240917);
  KeyedMirror m;
  m.reset(B, R, stride);
  Shadow sh(B, stride);
  std::vector<std::map<uint64_t, int>> ref(B);
  std::vector<int> where(R, -1);
  std::vector<uint64_t> keyOf(R, 0);
  int refused = 0, inserts = 0, updates = 0, removes = 0, moved = 0, noops = 0;
  for (int step = 0; step < 20000; ++step) {
    const int r = (int)(rng() % R);
    const int op = (int)(rng() % 4);
    KeyedMirror::Write w{};
    if (op <= 1) {  // insert (on a random broker when r is nowhere) or key update in place
      const int b = where[r] >= 0 ? where[r] : (int)(rng() % B);
      const uint64_t k = (rng() >> 20) * (uint64_t)R + (uint64_t)r;  // unique per replica, as Model::replicaKey
      bool lenChanged = false;
      const bool ok = m.upsert(b, r, k, &w, &lenChanged);
      if (!ok) {
        CHECK(where[r] < 0 && (int)ref[b].size() == stride, "step %d: upsert refused on a block with room", step);
        ++refused;
      } else {
        CHECK(lenChanged == (where[r] < 0), "step %d: lenChanged", step);
        CHECK(w.b == b && w.rep == r && w.key == k && w.slot >= 0 && w.slot < stride, "step %d: upsert's write", step);
        if (where[r] >= 0) {
          ref[b].erase(keyOf[r]);
          ++updates;
        } else {
          ++inserts;
        }
        ref[b][k] = r;
        where[r] = b;
        keyOf[r] = k;
        sh.row(w);
        if (lenChanged) sh.len[b] = m.len(b);
      }
    } else {  // remove from its broker, or from a broker it is not on (no-op)
      const bool wrong = op == 3 && (rng() & 1);
      const int b = wrong || where[r] < 0 ? (int)(rng() % B) : where[r];
      bool mv = false;
      const bool did = m.remove(b, r, &w, &mv);
      CHECK(did == (where[r] == b), "step %d: remove returned %d", step, (int)did);
      if (did) {
        ref[b].erase(keyOf[r]);
        where[r] = -1;
        if (mv) {
          CHECK(w.rep >= 0 && w.rep != r, "step %d: the moved row", step);
          sh.row(w);
          ++moved;
        }
        sh.len[b] = m.len(b);
        ++removes;
      } else {
        ++noops;
      }
    }
    if (step % 97 == 0 || step > 19900) compare(m, sh, ref, B, R, rng, step);
  }
  compare(m, sh, ref, B, R, rng, 20000);
  CHECK(refused > 0 && inserts > 100 && updates > 100 && removes > 100 && moved > 50 && noops > 50,
        "coverage: refused %d inserts %d updates %d removes %d moved %d noops %d", refused, inserts, updates, removes, moved,
        noops);
  if (fails) return 1;
  std::printf("keyed table ok: %d inserts, %d updates, %d removes (%d moved a row), %d refused, %d no-ops\n", inserts,
              updates, removes, moved, refused, noops);
  return 0;
}
