// csrc/dev_mem.h against the stand-in HIP of tests/cpp/fake_hip: ownership (moves, release, no leak at exit) and every growth
// policy to the byte; the counting arena against the real one, and the take that does not fit.  Built with -fsanitize=address,undefined by tests/test_ownership_cpp.py; exits 0 and prints "ok" when all hold.
#include "dev_mem.h"

#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

using namespace o3s;
using fake_hip::frees;
using fake_hip::mallocs;
using fake_hip::sizes;

static int failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

// the sizes hipMalloc was asked for since the last call
static std::vector<size_t> asked() {
  std::vector<size_t> v;
  v.swap(sizes);
  return v;
}
using V = std::vector<size_t>;

static void ownership() {
  const int m0 = mallocs, f0 = frees;
  {
    DevMem a;
    CHECK(a.p == nullptr && a.cap == 0);
    CHECK(a.alloc(100) == hipSuccess && a.p && a.cap == 100);
    void* block = a.p;
    DevMem b(std::move(a));  // a moved-from owner is empty and frees nothing
    CHECK(a.p == nullptr && a.cap == 0 && b.p == block && b.cap == 100);
    a.release();
    CHECK(frees == f0);
    DevMem c;
    CHECK(c.alloc(50) == hipSuccess);
    c = std::move(b);  // move assignment frees the target's old block exactly once
    CHECK(frees == f0 + 1 && c.p == block && c.cap == 100 && b.p == nullptr && b.cap == 0);
    c = std::move(c);  // onto itself: nothing happens
    CHECK(frees == f0 + 1 && c.p == block);
    c.release();  // release() twice frees once
    c.release();
    CHECK(frees == f0 + 2 && c.p == nullptr && c.cap == 0);
    CHECK(c.as<double>() == nullptr);
    DevMem d;
    CHECK(d.alloc(8) == hipSuccess);  // freed by its destructor
  }
  CHECK(mallocs - m0 == 3 && frees - f0 == 3);
  asked();
}

static void policy_alloc() {  // alloc (work buffers): grows when bytes > cap or empty; bytes, or 16 for 0; contents lost
  DevMem a;
  CHECK(a.alloc(1000) == hipSuccess && a.cap == 1000);
  void* first = a.p;
  CHECK(a.alloc(1000) == hipSuccess && a.alloc(1) == hipSuccess && a.alloc(0) == hipSuccess && a.p == first && a.cap == 1000);  // fits
  CHECK(a.alloc(1001) == hipSuccess && a.cap == 1001);  // below the doubling threshold of the other policies: still tight
  CHECK(a.alloc(5000) == hipSuccess && a.cap == 5000);
  DevMem z;
  CHECK(z.alloc(0) == hipSuccess && z.p && z.cap == 16);
  CHECK(z.alloc(16) == hipSuccess && z.alloc(17) == hipSuccess && z.cap == 17);
  CHECK(asked() == (V{1000, 1001, 5000, 16, 17}));
  fake_hip::fail_next_malloc = true;  // a failed allocation leaves an empty owner (the old block went first)
  CHECK(a.alloc(6000) != hipSuccess && a.p == nullptr && a.cap == 0);
  asked();
}

static void policy_ensure() {  // ensure (the map arrays): grows when bytes > cap; bytes + bytes / 2 + 4096, at least 2 * cap; keeps `keep` bytes
  DevMem a;
  CHECK(a.ensure(0, 0, nullptr) == hipSuccess && a.p == nullptr);  // nothing asked, nothing made
  CHECK(a.ensure(1000, 0, nullptr) == hipSuccess && a.cap == 1000 + 500 + 4096);  // 5596
  void* first = a.p;
  CHECK(a.ensure(5596, 0, nullptr) == hipSuccess && a.ensure(0, 0, nullptr) == hipSuccess && a.p == first && a.cap == 5596);  // fits
  DevMem b;
  CHECK(b.ensure(20000, 0, nullptr) == hipSuccess && b.cap == 20000 + 10000 + 4096);    // 34096
  CHECK(b.ensure(34097, 0, nullptr) == hipSuccess && b.cap == 2 * 34096);               // 34097 + 17048 + 4096 = 55241 < 68192: doubled
  CHECK(b.ensure(100000, 0, nullptr) == hipSuccess && b.cap == 100000 + 50000 + 4096);  // 154096 >= 2 * 68192: the formula
  CHECK(asked() == (V{5596, 34096, 68192, 154096}));
}

static void policy_ensure_keep() {
  DevMem a;
  CHECK(a.ensure(100, 0, nullptr) == hipSuccess && a.cap == 100 + 50 + 4096);  // 4246
  for (int k = 0; k < 100; ++k) a.as<unsigned char>()[k] = (unsigned char)(k + 1);
  const int c0 = fake_hip::copies, s0 = fake_hip::syncs, f0 = frees;
  void* old = a.p;
  CHECK(a.ensure(4247, 100, nullptr) == hipSuccess && a.p != old);
  CHECK(a.cap == 4247 + 2123 + 4096);  // 10466 >= 2 * 4246: the formula
  CHECK(fake_hip::copies == c0 + 1 && fake_hip::syncs == s0 + 1 && frees == f0 + 1);  // copied on the stream, drained, the old block freed once
  bool kept = true;
  for (int k = 0; k < 100; ++k) kept = kept && a.as<unsigned char>()[k] == (unsigned char)(k + 1);
  CHECK(kept);
  CHECK(a.ensure(20000, 0, nullptr) == hipSuccess && fake_hip::copies == c0 + 1);  // keep 0: no copy
  fake_hip::fail_next_malloc = true;  // a failed allocation leaves everything as it was
  old = a.p;
  const size_t cap = a.cap;
  CHECK(a.ensure(1 << 20, 16, nullptr) != hipSuccess && a.p == old && a.cap == cap);
  asked();
}

static void policy_arena() {  // Arena::reserve: grows when bytes > cap; bytes + bytes / 4 + 4096, at least 2 * had; always resets `used`
  Arena a;
  CHECK(a.reserve(0) == hipSuccess && a.mem.p == nullptr);
  CHECK(a.reserve(8000) == hipSuccess && a.mem.cap == 8000 + 2000 + 4096);  // 14096
  char* base = a.mem.as<char>();
  CHECK(a.take<double>(10) == reinterpret_cast<double*>(base) && a.used == 256 && a.take<char>(1) == base + 256 && a.used == 512);
  CHECK(a.reserve(14096) == hipSuccess && a.mem.as<char>() == base && a.used == 0);  // fits; used is reset
  CHECK(a.reserve(14097) == hipSuccess && a.mem.cap == 2 * 14096);                   // 14097 + 3524 + 4096 = 21717 < 28192: doubled
  CHECK(a.reserve(100000) == hipSuccess && a.mem.cap == 100000 + 25000 + 4096);      // above it: the formula
  a.take<char>(1);
  a.release();
  CHECK(a.mem.p == nullptr && a.mem.cap == 0 && a.used == 0);
  CHECK(asked() == (V{14096, 28192, 129096}));
}

// a layout over every element size the work areas use (1, 4, 8, 12 bytes), all of one count
struct Twelve {
  uint32_t w[3];
};
struct ToyArea {
  static constexpr size_t kSlack = 512;
  char* c;
  uint32_t* u;
  double* d;
  Twelve* t;
  template <class A>
  void lay(A& a, size_t count) {
    take(a, c, count);
    take(a, u, count);
    take(a, d, count);
    take(a, t, count);
  }
};

static void layouts() {  // the counting arena adds up what Arena::take hands out, to the byte
  Arena a;
  for (size_t count : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, ((size_t)1 << 20) + 1}) {
    const size_t bytes = measure<ToyArea>(count);
    CHECK(bytes == Arena::pad(count) + Arena::pad(count * 4) + Arena::pad(count * 8) + Arena::pad(count * 12));
    CHECK(layout_bytes<ToyArea>(count) == bytes + 512);
    ToyArea w{};
    CHECK(lay_out(a, w, count) == hipSuccess && !a.refused);
    CHECK(a.used == bytes && a.mem.cap >= bytes + 512);
    char* base = a.mem.as<char>();
    CHECK(w.c == base && reinterpret_cast<char*>(w.u) == base + Arena::pad(count));
    CHECK(reinterpret_cast<char*>(w.t) + Arena::pad(count * 12) == base + bytes);
    if (count) w.t[count - 1].w[2] = 7u;  // the last word of the last array is inside the block (the sanitizer watches)
  }
  for (size_t size : {(size_t)1, (size_t)4, (size_t)8, (size_t)12})  // each element size alone, across a padding boundary
    for (size_t count : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, ((size_t)1 << 20) + 1}) {
      ArenaCount c;
      CHECK(a.reserve(count * size + 256) == hipSuccess);
      if (size == 1) c.take<char>(count), a.take<char>(count);
      if (size == 4) c.take<uint32_t>(count), a.take<uint32_t>(count);
      if (size == 8) c.take<double>(count), a.take<double>(count);
      if (size == 12) c.take<Twelve>(count), a.take<Twelve>(count);
      CHECK(c.used == a.used && c.used == ((count * size + 255) / 256) * 256 && !a.refused);
    }
  // a layout laid into a reservation that is too small is reported, and nothing points anywhere
  Arena small;
  ToyArea w{};
  CHECK(lay_out_in(small, 0, w, 1) != hipSuccess && small.refused && small.used == 0);
  CHECK(w.c == nullptr && w.u == nullptr && w.d == nullptr && w.t == nullptr);
  CHECK(lay_out_in(small, 0, w, 0) == hipSuccess && !small.refused);  // nothing asked, nothing refused
  asked();
}

static void checked_take() {  // a take that does not fit: nullptr, the flag latched, `used` as it was; reserve clears the flag
  Arena a;
  CHECK(a.reserve(4096) == hipSuccess && a.mem.cap == 4096 + 1024 + 4096);  // 9216 = 36 * 256
  const size_t cap = a.mem.cap;
  char* base = a.mem.as<char>();
  CHECK(a.take<char>(cap) == base && a.used == cap && !a.refused);  // fits exactly
  CHECK(a.take<char>(0) == base + cap && a.used == cap && !a.refused);  // nothing more asked: nothing refused
  CHECK(a.take<char>(1) == nullptr && a.refused && a.used == cap);
  CHECK(a.reserve(cap) == hipSuccess && a.mem.as<char>() == base && !a.refused && a.used == 0);
  CHECK(a.take<char>(cap + 1) == nullptr && a.refused && a.used == 0);  // one byte more than there is
  CHECK(a.reserve(cap) == hipSuccess && !a.refused);
  CHECK(a.take<double>(32) == reinterpret_cast<double*>(base) && a.used == 256);
  CHECK(a.take<uint32_t>((cap - 256) / 4 + 1) == nullptr && a.refused && a.used == 256);  // one element past the rest
  CHECK(a.take<uint32_t>((cap - 256) / 4) == reinterpret_cast<uint32_t*>(base + 256) && a.used == cap);  // the rest exactly
  CHECK(a.refused);  // latched until the next reserve
  CHECK(a.reserve(1) == hipSuccess && !a.refused && a.used == 0);
  base[cap - 1] = 1;  // the block is all there
  asked();
}

static void policy_cells() {  // NormalsWork::cells: grows when ncells * 8 > cap; ncells * 8 + 4096; contents lost
  DevMem c;
  CHECK(c.fit(0, 4096) == hipSuccess && c.p == nullptr);
  CHECK(c.fit(1000 * 8, 4096) == hipSuccess && c.cap == 8000 + 4096);
  void* first = c.p;
  CHECK(c.fit(12096, 4096) == hipSuccess && c.p == first);                  // fits
  CHECK(c.fit(12097, 4096) == hipSuccess && c.cap == 12097 + 4096);         // no doubling in this policy
  CHECK(c.fit(1 << 20, 4096) == hipSuccess && c.cap == (1 << 20) + 4096);
  CHECK(asked() == (V{12096, 16193, (1 << 20) + 4096}));
}

static void policy_devbuf() {  // DevBuf::ensure: grows when bytes > cap; bytes + bytes / 8 + 256, at least 2 * had; bumps *gen before it moves
  uint64_t gen = 0;
  {
    DevBuf b{&gen};
    b.release();  // empty: no bump
    CHECK(gen == 0);
    CHECK(b.ensure(0) == hipSuccess && gen == 0 && b.p == nullptr);
    CHECK(b.ensure(8000) == hipSuccess && b.cap == 8000 + 1000 + 256 && gen == 1);  // 9256
    void* first = b.p;
    CHECK(b.ensure(9256) == hipSuccess && b.ensure(1) == hipSuccess && b.p == first && gen == 1);  // fits: no bump
    CHECK(b.ensure(9257) == hipSuccess && b.cap == 2 * 9256 && gen == 2);                      // 9257 + 1157 + 256 = 10670 < 18512: doubled
    CHECK(b.ensure(100000) == hipSuccess && b.cap == 100000 + 12500 + 256 && gen == 3);        // above it: the formula
    b.release();
    CHECK(gen == 4 && b.p == nullptr && b.cap == 0);
    b.release();  // twice: one free, one bump
    CHECK(gen == 4);
    CHECK(b.ensure(64) == hipSuccess && gen == 5 && b.cap == 64 + 8 + 256);  // after a release it starts tight again
    DevBuf unwired;  // d_loc: no generation to report to
    CHECK(unwired.ensure(100) == hipSuccess && unwired.cap == 100 + 12 + 256);
  }
  CHECK(gen == 6);  // the destructor released a held block
  CHECK(asked() == (V{9256, 18512, 112756, 328, 368}));
}

int main() {
  ownership();
  policy_alloc();
  policy_ensure();
  policy_ensure_keep();
  policy_arena();
  layouts();
  checked_take();
  policy_cells();
  policy_devbuf();
  CHECK(mallocs == frees);  // at program end, frees equal allocations
  std::printf("mallocs %d frees %d\n", mallocs, frees);
  if (failed) return 1;
  std::printf("ok\n");
  return 0;
}
