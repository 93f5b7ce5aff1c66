// Host unit check of engine/devbuf.h: Carver's layout guarantee and DevBuf's growth rule, over allocation functions
// backed by malloc that count their calls. Build: g++ -O1 -std=c++17. Prints "devbuf ok: <n> checks" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "devbuf.h"

namespace {

long checks = 0;
int allocs = 0, frees = 0;
bool failNext = false;
std::set<void*> live;
std::vector<size_t> asked;

void* countedAlloc(size_t bytes) {
  if (failNext) {
    failNext = false;
    throw std::runtime_error("out of memory (test)");
  }
  allocs++;
  asked.push_back(bytes);
  void* p = std::aligned_alloc(256, bytes);
  live.insert(p);
  return p;
}

void countedFree(void* p) {
  frees++;
  if (!live.erase(p)) {
    std::fprintf(stderr, "free of a block that is not live\n");
    std::exit(1);
  }
  std::free(p);
}

#define CHECK(c)                                                       \
  do {                                                                 \
    checks++;                                                          \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);             \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

struct E24 {
  char b[24];
};

struct Piece {
  uintptr_t at;
  size_t bytes;
};

// four pieces of element type P with the given counts, sized over a null base and placed over a real one
template <class P>
void carve(const size_t (&counts)[4]) {
  P* q[4];
  ccmi::Carver sizing(nullptr);
  for (int i = 0; i < 4; ++i) {
    sizing.take(q[i], counts[i]);
    CHECK(q[i] == nullptr);
  }
  std::vector<char> store(sizing.off + 256);
  char* base = (char*)(((uintptr_t)store.data() + 255) & ~(uintptr_t)255);
  ccmi::Carver placing(base);
  Piece pc[4];
  for (int i = 0; i < 4; ++i) {
    placing.take(q[i], counts[i]);
    pc[i] = Piece{(uintptr_t)q[i], sizeof(P) * counts[i]};
  }
  CHECK(placing.off == sizing.off);
  for (int i = 0; i < 4; ++i) {
    CHECK(pc[i].at % 256 == 0);
    CHECK(pc[i].at >= (uintptr_t)base);
    const uintptr_t next = i < 3 ? pc[i + 1].at : (uintptr_t)base + placing.off;
    CHECK(next > pc[i].at);  // a zero-count piece is still a pointer of its own
    CHECK(next - pc[i].at >= ccmi::align256(pc[i].bytes));
    // a list finished with whole 16-byte stores stays inside its piece
    CHECK(next - pc[i].at >= ((pc[i].bytes + 15) & ~(size_t)15));
  }
}

template <class P>
void carveAll() {
  const size_t sets[][4] = {{0, 1, 63, 64}, {65, 0, 0, 1}, {64, 65, 63, 0}, {1, 1, 1, 1}, {0, 0, 0, 0}};
  for (const auto& s : sets) carve<P>(s);
}

}  // namespace

namespace ccmi {
void* deviceAlloc(size_t bytes) { return countedAlloc(bytes); }
void deviceFree(void* p) noexcept { countedFree(p); }
void* pinnedAlloc(size_t bytes) { return countedAlloc(bytes); }
void pinnedFree(void* p) noexcept { countedFree(p); }
}  // namespace ccmi

template <class Buf>
void growth() {
  const int a0 = allocs, f0 = frees;
  {
    Buf b;
    CHECK(!b && b.get() == nullptr && b.capacity() == 0);
    CHECK(b.ensure(0) == nullptr && allocs == a0);  // nothing asked, nothing allocated
    void* p = b.ensure(1000);                       // a first allocation is exact to 256
    CHECK(p && b && b.get() == p && b.capacity() == 1024 && asked.back() == 1024);
    CHECK(allocs == a0 + 1 && frees == f0);
    CHECK(b.ensure(10) == p && b.ensure(1024) == p && allocs == a0 + 1);  // a smaller request keeps the pointer
    void* q = b.ensure(1025);  // a regrowth: align256(bytes + bytes / 4), the old block freed exactly once
    CHECK(q && b.capacity() == ccmi::align256(1025 + 1025 / 4) && asked.back() == b.capacity());
    CHECK(allocs == a0 + 2 && frees == f0 + 1 && live.count(q) == 1 && live.size() == 1);
    CHECK(b.ensure(1000) == q && allocs == a0 + 2);

    Buf moved(std::move(b));  // a moved-from buffer owns nothing and frees nothing
    CHECK(!b && b.capacity() == 0 && moved.get() == q && moved.capacity() == ccmi::align256(1025 + 1025 / 4));
    Buf assigned;
    assigned.ensure(1);
    CHECK(assigned.capacity() == 256 && allocs == a0 + 3);
    assigned = std::move(moved);  // the target's block goes, the source's moves in
    CHECK(frees == f0 + 2 && assigned.get() == q && !moved && live.size() == 1);

    failNext = true;  // a throwing allocator leaves the buffer empty and reusable
    bool threw = false;
    try {
      assigned.ensure(1 << 20);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw && !assigned && assigned.capacity() == 0 && frees == f0 + 3 && live.empty());
    void* r = assigned.ensure(300);  // empty again, so a first allocation
    CHECK(r && assigned.capacity() == 512 && allocs == a0 + 4);
  }
  CHECK(frees == f0 + 4 && allocs == a0 + 4 && live.empty());  // the destructor freed the one live block
}

// carve: the two passes of one layout over a buffer
void carving() {
  const int a0 = allocs;
  ccmi::DevBuf b;
  int32_t* x = nullptr;
  E24* y = nullptr;
  uint8_t* z = nullptr;
  int passes = 0;
  auto layout = [&](ccmi::Carver& c) {
    passes++;
    c.take(x, 65);
    c.take(y, 0);
    c.take(z, 1);
  };
  const size_t bytes = ccmi::carve(b, layout);
  CHECK(passes == 2 && bytes == 512 + 256 + 256 && b.capacity() == bytes && allocs == a0 + 1);
  CHECK((char*)x == (char*)b.get() && (char*)y == (char*)x + 512 && (char*)z == (char*)y + 256);
  CHECK(ccmi::carve(b, layout) == bytes && allocs == a0 + 1 && (char*)x == (char*)b.get());  // room enough: no regrowth
}

int main() {
  CHECK(ccmi::align256(0) == 0 && ccmi::align256(1) == 256 && ccmi::align256(256) == 256 && ccmi::align256(257) == 512);
  carveAll<uint8_t>();
  carveAll<int32_t>();
  carveAll<double>();
  carveAll<E24>();
  static_assert(sizeof(E24) == 24, "element sizes 1, 4, 8 and 24");
  growth<ccmi::DevBuf>();
  growth<ccmi::PinBuf>();
  carving();
  std::printf("devbuf ok: %ld checks\n", checks);
  return 0;
}
