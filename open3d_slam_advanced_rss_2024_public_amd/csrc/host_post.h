// The host post: how every small device-to-host answer of this library comes back (a count, six bounds, the sums of a
// registration pass).  A kernel tail stores the values and then a sequence number into pinned, host-coherent memory; the host
// spins on the sequence number and looks at the stream only now and then, so that a fault upstream cannot leave it spinning.
// One block layout, one device-side store, one host-side wait, shared by both translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <time.h>

#include "icp_types.h"  // O3S_HOOK_ENV

namespace o3s {
namespace host_post {

// ---- layout: word 0 a lone count, word 1 the sequence number, values from word 2 (8-byte values stay 8-byte aligned) ----------
constexpr int kPostCount = 0, kPostSeq = 1, kPostVals = 2;

inline double now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}

// the hooks build can switch every post off (O3S_NO_MAILBOX): read per call, the tests run both sides in one process
inline bool posts_enabled() { return O3S_HOOK_ENV("O3S_NO_MAILBOX") == nullptr; }

// A mapped, host-coherent, zeroed block and the sequence numbers of its posts.  No destructor: who frees a block and who
// leaks it on purpose is the owner's business.
template <class T = uint32_t>
struct PostBlock {
  T* host = nullptr;
  T* dev = nullptr;  // the same block as the device addresses it
  uint32_t seq = 0;
  hipError_t alloc(size_t bytes = sizeof(T)) {
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), bytes, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return host = nullptr, e;
    memset(host, 0, bytes);
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0);
    if (e != hipSuccess) release();
    return e;
  }
  void release() {
    if (host) (void)hipHostFree(host);
    host = dev = nullptr;
  }
  uint32_t next() {  // never 0: a fresh block reads 0, and 0 is what a guarded post stores while its values change
    if (++seq == 0) ++seq;
    return seq;
  }
  explicit operator bool() const { return host && dev; }
};

// ---- device side ------------------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void post_store1(uint32_t* mb, int word, T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a post is made of 4- and 8-byte values");
  if constexpr (sizeof(T) == 4)
    __hip_atomic_store(mb + word, __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(mb + word), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// v[0..N) to the words from `word` on, not yet published
template <class T, int N>
__device__ __forceinline__ void post_store(uint32_t* mb, int word, const T (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) post_store1(mb, word + k * (int)(sizeof(T) / 4), v[k]);
}
__device__ __forceinline__ void post_publish(uint32_t* mb, uint32_t seq) {
  __hip_atomic_store(mb + kPostSeq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The whole tail, for one thread: the values, then the sequence number.
// kGuarded = false is for a slot with one outstanding post whose reader is its issuer: nobody reads while the values change.
// kGuarded = true is a seqlock, for a slot that is read LATER and possibly by another thread while the issuer posts again:
// 0 (which next() never hands out), a system-scope release fence, the values, the number with release.  A reader (read_guarded)
// that loads any value of this post B has, through its acquire fence, synchronised with that release fence, and the store of 0 is
// sequenced before the fence: the reader's second look at the sequence word sees 0 or B, never the A of the post before.  So the
// values of one post are never accepted under the number of another.  (Not a race to provoke in a test: the argument is the
// check.)  One fence, not a release on every value: a system-scope release store writes the L2 back and waits for the store
// before it to be acknowledged by the host — six of them in a row were six PCIe round trips at the tail of every pending insert.
template <bool kGuarded = false, class T, int N>
__device__ __forceinline__ void post(uint32_t* mb, uint32_t seq, int word, const T (&v)[N]) {
  if constexpr (kGuarded) {
    post_store1(mb, kPostSeq, 0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  }
  post_store(mb, word, v);
  post_publish(mb, seq);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
template <class T = uint32_t>
inline T post_get(const uint32_t* mb, int word) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a post is made of 4- and 8-byte values");
  if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, __atomic_load_n(mb + word, __ATOMIC_RELAXED));
  else return __builtin_bit_cast(T, __atomic_load_n(reinterpret_cast<const unsigned long long*>(mb + word), __ATOMIC_RELAXED));
}
inline bool post_landed(const uint32_t* mb, uint32_t seq) { return __atomic_load_n(mb + kPostSeq, __ATOMIC_ACQUIRE) == seq; }
// the reading side of a guarded post: the number, the values, the number again
inline bool read_guarded(const uint32_t* mb, uint32_t seq, int word, uint32_t* out, int n) {
  if (!post_landed(mb, seq)) return false;
  for (int k = 0; k < n; ++k) out[k] = post_get(mb, word + k);
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return post_landed(mb, seq);
}

// How often a waiting host leaves its spin.  hipStreamQuery / hipEventQuery are calls into the runtime (its locks, possibly a
// marker packet in the queue), never part of the polling itself; the values are measured ones.  (Round 5: with the stream polled
// every ~10 us the receiving thread's waits slowed the MAPPING thread's launches down whenever the two overlapped — the
// reference re-init took 0.34 ms instead of 0.11 with page-locked sweeps, where the receiving thread reaches its wait early.)
struct PollCadence {
  int spins;             // looks between two readings of the clock
  double event_us;       // the `drained` event, when there is one, is queried this often at most
  double guard_us;       // the stream itself: the guard against a fault upstream
  bool guard_at_once;    // the first look at the stream may come at once (the post is usually long there, or never will be)
};
constexpr double kPollGuardUs = 200.0;
constexpr PollCadence kMailboxCadence{4096, 0.0, kPollGuardUs, false};
constexpr PollCadence kLazyCadence{4096, 0.0, kPollGuardUs, true};
constexpr PollCadence kChainCadence{256, 4.0, 2000.0, false};

enum { kPollError = -1, kPollDrained = 0, kPollPosted = 1 };
enum { kTierSpin = 0, kTierEvent = 1, kTierGuard = 2 };
struct PollTrace {
  int queries = 0;       // calls into the runtime
  int tier = kTierSpin;  // what ended the wait
};
// Spins on look() until it holds: kPollPosted.  When `drained` (nullable: an event behind the last launch issued) or the stream
// reports that everything has run, one last look decides between kPollPosted and kPollDrained; any other answer of the runtime
// is kPollError.
template <class Look>
inline int poll_until(Look&& look, hipStream_t s, const PollCadence& c, hipEvent_t drained = nullptr, PollTrace* trace = nullptr) {
  PollTrace unused;
  PollTrace& tr = trace ? *trace : unused;
  double t_event = now_us(), t_guard = c.guard_at_once ? t_event - c.guard_us : t_event;
  for (;;) {
    for (int spin = 0; spin < c.spins; ++spin)
      if (look()) return kPollPosted;
    if (drained) {
      const double t = now_us();
      if (t - t_event >= c.event_us) {
        t_event = t;
        tr.queries += 1;
        const hipError_t q = hipEventQuery(drained);
        if (q == hipSuccess) return tr.tier = kTierEvent, look() ? kPollPosted : kPollDrained;
        if (q != hipErrorNotReady) return kPollError;
      }
    }
    const double t = now_us();  // (a reading of its own: behind an event tier the round's two readings are part of the measured cadence)
    if (t - t_guard < c.guard_us) continue;
    t_guard = t;
    tr.queries += 1;
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return tr.tier = kTierGuard, look() ? kPollPosted : kPollDrained;
    if (q != hipErrorNotReady) return kPollError;
  }
}
inline int mailbox_wait(const uint32_t* mb, uint32_t seq, hipStream_t s) {
  return poll_until([=] { return post_landed(mb, seq); }, s, kMailboxCadence);
}

// Waits for post `seq` (0: none was issued) and reads its n words from `word` on: kPollPosted.  Otherwise the words are copied
// from `dev_src` — through `landing`, a pinned area, when there is one — behind a synchronisation of the stream: kPollDrained.
// A caller whose device copy is not the posted words passes no dev_src and folds its own after kPollDrained.
inline int fetch_post(const PostBlock<>& mb, uint32_t seq, hipStream_t s, uint32_t* out, int n, int word, const void* dev_src,
                      uint32_t* landing = nullptr) {
  if (seq) {
    const int w = mailbox_wait(mb.host, seq, s);
    if (w == kPollError) return w;
    if (w == kPollPosted) {
      for (int k = 0; k < n; ++k) out[k] = post_get(mb.host, word + k);
      return w;
    }
  }
  if (!dev_src) return kPollDrained;
  uint32_t* dst = landing ? landing : out;
  if (hipMemcpyAsync(dst, dev_src, (size_t)n * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return kPollError;
  for (int k = 0; k < n; ++k) out[k] = dst[k];
  return kPollDrained;
}

}  // namespace host_post
}  // namespace o3s
