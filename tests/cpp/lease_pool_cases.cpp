// csrc/lease_pool.h: what a leased work area may rely on, single-threaded and under eight threads.  Built twice by
// tests/test_ownership_cpp.py (-fsanitize=thread and -fsanitize=address,undefined); exits 0 and prints "ok" when all hold.
#include "lease_pool.h"

#include <atomic>
#include <cstdio>
#include <memory>
#include <set>
#include <thread>
#include <vector>

using o3s::LeasePool;

static std::atomic<int> failed{0};
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

// an area that counts its constructions and destructions; Tag keeps the pools of the cases apart (one pool per type, for good)
template <int Tag>
struct Area {
  static inline std::atomic<int> made{0}, gone{0};
  int key = -1;                // the key it was first given under (-1: fresh)
  std::atomic<int> holder{0};  // the mark: who holds the area right now
  Area() { ++made; }
  ~Area() { ++gone; }
};

static void keys_and_drop() {
  using A = Area<1>;
  LeasePool<A>& pool = LeasePool<A>::get();
  CHECK(&pool == &LeasePool<A>::get());  // one pool per type
  // holding `count` leases at once yields `count` distinct areas
  std::vector<std::unique_ptr<A>> held;
  std::set<A*> distinct;
  for (int k = 0; k < 5; ++k) {
    held.push_back(pool.take(0));
    held.back()->key = 0;
    distinct.insert(held.back().get());
  }
  CHECK(distinct.size() == 5 && A::made == 5);
  for (auto& a : held) pool.give(0, std::move(a));
  held.clear();
  // take(k) never returns an area given under another key
  std::unique_ptr<A> one = pool.take(1);
  CHECK(one->key == -1 && A::made == 6);  // fresh, although five areas of key 0 are idle
  one->key = 1;
  pool.give(1, std::move(one));
  for (int k = 0; k < 5; ++k) {
    held.push_back(pool.take(0));
    CHECK(held.back()->key == 0);
  }
  CHECK(A::made == 6);  // all five came out of the pool again
  std::unique_ptr<A> again = pool.take(1);
  CHECK(again->key == 1 && A::made == 6);
  pool.give(1, std::move(again));
  // drop_idle(k) destroys exactly the idle areas of k: two of key 0 are idle, three are held, one of key 1 is idle
  pool.give(0, std::move(held[3]));
  pool.give(0, std::move(held[4]));
  held.resize(3);
  CHECK(A::gone == 0);
  pool.drop_idle(0);
  CHECK(A::gone == 2);
  for (auto& a : held) CHECK(a && a->key == 0 && a->holder == 0);  // the held ones are alive (the sanitizer would tell otherwise)
  std::unique_ptr<A> other = pool.take(1);
  CHECK(other->key == 1 && A::made == 6);  // the other key's area was left alone
  pool.give(1, std::move(other));
  pool.drop_idle(0);  // nothing idle under the key: nothing happens
  CHECK(A::gone == 2);
  for (auto& a : held) pool.give(0, std::move(a));
  pool.drop_idle(0);
  pool.drop_idle(1);
  CHECK(A::gone == 6 && A::made == 6);
  CHECK(pool.take(0)->key == -1 && A::made == 7);  // an emptied pool makes fresh areas (this one dies with its unique_ptr)
  pool.give(0, nullptr);                           // a lease that was moved from gives nothing back
  CHECK(A::gone == 7);
}

static void eight_threads() {
  using A = Area<2>;
  constexpr int kThreads = 8, kRounds = 1000, kKeys = 2;
  LeasePool<A>& pool = LeasePool<A>::get();
  // out[k]: leases of key k that are out, counted from BEFORE take() to AFTER give() — never less than the areas that are out of
  // the pool, so its peak bounds from above the number of areas the pool can have had to make for the key
  std::atomic<int> out[kKeys], peak[kKeys];
  for (int k = 0; k < kKeys; ++k) out[k] = peak[k] = 0;
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&, t] {
      for (int r = 0; r < kRounds; ++r) {
        const int key = (t + r) % kKeys;
        const int now = ++out[key];
        for (int seen = peak[key]; now > seen && !peak[key].compare_exchange_weak(seen, now);) {
        }
        std::unique_ptr<A> a = pool.take(key);
        if (a->key == -1) a->key = key;
        CHECK(a->key == key);  // never an area given under the other key
        int nobody = 0;
        CHECK(a->holder.compare_exchange_strong(nobody, t + 1));  // no area is ever held by two threads at once
        std::this_thread::yield();
        CHECK(a->holder.exchange(0) == t + 1);
        pool.give(key, std::move(a));
        --out[key];
      }
    });
  for (std::thread& th : threads) th.join();
  // a fresh area is made only when no area of the key is idle, i.e. when every area made for it is out: per key, the areas ever
  // made are at most the peak number out at once
  int made_bound = 0;
  for (int k = 0; k < kKeys; ++k) made_bound += peak[k];
  std::printf("made %d, peak out %d + %d\n", (int)A::made, (int)peak[0], (int)peak[1]);
  CHECK(A::made <= made_bound && A::made >= 1 && A::gone == 0);
  int idle[kKeys] = {0, 0};
  for (int k = 0; k < kKeys; ++k) {
    const int before = A::gone;
    pool.drop_idle(k);
    idle[k] = A::gone - before;
    CHECK(idle[k] <= peak[k]);  // ... per key
  }
  CHECK(idle[0] + idle[1] == A::made && A::gone == A::made);  // everything went back, nothing was lost or made twice
}

int main() {
  keys_and_drop();
  eight_threads();
  if (failed) return 1;
  std::printf("ok\n");
  return 0;
}
