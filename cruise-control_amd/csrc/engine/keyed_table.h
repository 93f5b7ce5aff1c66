// Host mirror of the queue scans' keyed membership table (devtypes.h KeyedRow, SOP_QUEUE): per broker a block of
// `stride` row slots in no particular order and a length; per replica the slot it occupies. A replica that joins,
// leaves or changes its key costs one row write and at most one length write on the device (removal moves the block's
// last row into the hole), whatever the broker's size. The mirror answers what the sorted snapshot used to: a slot's
// replica, and how many of a broker's rows sort below a key. Host-only (no device types): tests/cpp drives it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ccmi {

class KeyedMirror {
 public:
  // one device write the caller has to carry out: row `slot` of broker `b` now holds (rep, key); rep < 0: only the
  // broker's length changed
  struct Write {
    int32_t b, slot, rep;
    uint64_t key;
  };
  void reset(int B, int R, int stride) {
    B_ = B;
    stride_ = stride;
    len_.assign((size_t)B, 0);
    rep_.assign((size_t)B * (size_t)stride, -1);
    key_.assign((size_t)B * (size_t)stride, 0);
    slotOf_.assign((size_t)R, -1);
    brokerOf_.assign((size_t)R, -1);
  }
  int stride() const { return stride_; }
  int brokers() const { return B_; }
  int len(int b) const { return len_[(size_t)b]; }
  int rep(int b, int slot) const { return rep_[(size_t)b * stride_ + slot]; }
  uint64_t key(int b, int slot) const { return key_[(size_t)b * stride_ + slot]; }
  int slotOf(int r) const { return slotOf_[(size_t)r]; }      // -1: in no block
  int brokerOf(int r) const { return brokerOf_[(size_t)r]; }  // the block r sits in, -1: none

  // r is on b with `key`: inserted at the block's end, or its key rewritten in place. False (nothing changed) when
  // the block is full. *w: the row to write; lenChanged: the length word too.
  bool upsert(int b, int r, uint64_t key, Write* w, bool* lenChanged) {
    const size_t base = (size_t)b * stride_;
    int s = brokerOf_[(size_t)r] == b ? slotOf_[(size_t)r] : -1;
    *lenChanged = s < 0;
    if (s < 0) {
      if (len_[(size_t)b] >= stride_) return false;
      s = len_[(size_t)b]++;
      slotOf_[(size_t)r] = s;
      brokerOf_[(size_t)r] = b;
      rep_[base + s] = r;
    }
    key_[base + s] = key;
    *w = Write{b, s, r, key};
    return true;
  }
  // r leaves b's block (no-op when it is not there): the last row moves into its slot. Returns the writes (0..1 row
  // writes; the length always changes when anything does) in w[0]; *moved: w[0] is a row write.
  bool remove(int b, int r, Write* w, bool* moved) {
    *moved = false;
    if (brokerOf_[(size_t)r] != b) return false;
    const size_t base = (size_t)b * stride_;
    const int s = slotOf_[(size_t)r], last = --len_[(size_t)b];
    slotOf_[(size_t)r] = -1;
    brokerOf_[(size_t)r] = -1;
    if (s != last) {
      const int x = rep_[base + last];
      rep_[base + s] = x;
      key_[base + s] = key_[base + last];
      slotOf_[(size_t)x] = s;
      *w = Write{b, s, x, key_[base + s]};
      *moved = true;
    } else {
      *w = Write{b, s, -1, 0};
    }
    rep_[base + last] = -1;
    return true;
  }
  // rows of b whose key is below `k` (the index the row with key k has, or would have, in b's sorted view)
  int below(int b, uint64_t k) const {
    const size_t base = (size_t)b * stride_;
    int n = 0;
    for (int s = 0, e = len_[(size_t)b]; s < e; ++s) n += key_[base + s] < k ? 1 : 0;
    return n;
  }
  // rows of b whose key is `k` or below: what a continuation behind the row with key k passes over (not below(k + 1),
  // which wraps at the largest key)
  int atOrBelow(int b, uint64_t k) const {
    const size_t base = (size_t)b * stride_;
    int n = 0;
    for (int s = 0, e = len_[(size_t)b]; s < e; ++s) n += key_[base + s] <= k ? 1 : 0;
    return n;
  }
  // b's replicas in key order (the sorted snapshot of the block), for the paths that need whole sorted rows
  void sorted(int b, std::vector<int32_t>& out) const;

 private:
  int B_ = 0, stride_ = 0;
  std::vector<int32_t> len_;     // [B]
  std::vector<int32_t> rep_;     // [B * stride] replica per slot (-1 past the length)
  std::vector<uint64_t> key_;    // [B * stride]
  std::vector<int32_t> slotOf_, brokerOf_;  // [R]
};

inline void KeyedMirror::sorted(int b, std::vector<int32_t>& out) const {
  const size_t base = (size_t)b * stride_;
  const int n = len_[(size_t)b];
  out.resize((size_t)n);
  std::vector<int32_t> ord((size_t)n);
  for (int s = 0; s < n; ++s) ord[(size_t)s] = s;
  std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return key_[base + x] < key_[base + y]; });
  for (int s = 0; s < n; ++s) out[(size_t)s] = rep_[base + ord[(size_t)s]];
}

}  // namespace ccmi
