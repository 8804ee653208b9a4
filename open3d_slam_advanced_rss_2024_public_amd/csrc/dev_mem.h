// dev_mem.h — the one owner of a hipMalloc'd block, shared by both translation units (o3s_icp.hip, cloud_ops.hip).  Only the HIP
// runtime header and the standard library: tests/cpp/dev_mem_cases.cpp compiles it against a stub of the four calls it makes.
//
// DevMem frees what it holds when it dies, is overwritten by a move, or is told to release(); it cannot be copied.  WHEN a block
// grows and by how much is the caller's policy, spelled out by the members below and by the types built on them (Arena and DevBuf
// further down): the capacities are visible through *_device_bytes and decide when the device stalls in a
// hipFree / hipMalloc, so each policy is kept to the byte.
//
// HOW a block is carved up is said once per work area, by a layout (below, at Arena): the same description is measured on a
// counting arena and laid out on the real one, so no size formula stands apart from the takes it sizes, and a take that does
// not fit is refused instead of handing out an address past the block.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace o3s {

struct DevMem {
  void* p = nullptr;
  size_t cap = 0;

  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  DevMem(DevMem&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevMem& operator=(DevMem&& o) noexcept {  // what the target held is freed
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevMem() { release(); }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }

  // a block of exactly `bytes` in place of the one held: free first, then allocate (the contents are lost; empty on failure)
  hipError_t reset(size_t bytes) {
    release();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  // tight and grow-only: a request that fits re-uses the memory, one that does not gets exactly `bytes` (16 for none)
  hipError_t alloc(size_t bytes) {
    if (p && bytes <= cap) return hipSuccess;
    return reset(bytes ? bytes : 16);
  }
  // grow-only with head room: bytes + bytes / slack_div + pad, and at least twice what it had — a block that grows AGAIN belongs
  // to a cloud that grows (a map), and every move stalls the whole device for milliseconds
  hipError_t grow(size_t bytes, size_t slack_div, size_t pad) {
    if (bytes <= cap) return hipSuccess;
    const size_t had = cap;
    size_t want = bytes + bytes / slack_div + pad;
    if (had && want < 2 * had) want = 2 * had;
    return reset(want);
  }
  // grow-only with a fixed margin: bytes + pad when `bytes` do not fit (the contents are lost)
  hipError_t fit(size_t bytes, size_t pad) { return bytes > cap ? reset(bytes + pad) : hipSuccess; }
  // grow-only, half as much again + 4096 (at least twice what it had), keeping the first `keep` bytes: the new block is made
  // first, the prefix copied on `s` and `s` drained before the old block goes.  A failed allocation leaves everything as it was
  hipError_t ensure(size_t bytes, size_t keep, hipStream_t s) {
    if (bytes <= cap) return hipSuccess;
    size_t want = bytes + bytes / 2 + 4096;
    if (cap && want < 2 * cap) want = 2 * cap;
    DevMem q;
    hipError_t e = hipMalloc(&q.p, want);
    if (e != hipSuccess) {
      q.p = nullptr;
      return e;
    }
    q.cap = want;
    if (p && keep) {
      e = hipMemcpyAsync(q.p, p, keep, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    *this = static_cast<DevMem&&>(q);
    return e;
  }
};

// ---- grow-only device arena: one allocation per pipeline call at most, none once it has seen the largest input -----
// A work area is described ONCE, by a layout: a struct of the pointers with `template <class A> void lay(A& a, sizes...)`
// taking each array in turn, and `kSlack`, the bytes it reserves beyond them.  The same lay() runs on an ArenaCount, which
// only adds the padded sizes up, and on the Arena, which hands out the addresses: what is reserved is what is taken, by
// construction (layout_bytes, lay_out).  Sizes rocPRIM reports are arguments of a layout, so a layout is plain arithmetic.
struct Arena {
  DevMem mem;
  size_t used = 0;
  bool refused = false;               // a take did not fit: the layout is unusable (lay_out reports it before anything is launched)
  hipError_t reserve(size_t bytes) {  // (growing again: the cloud behind it grows (a map); hipFree / hipMalloc stall the device for milliseconds)
    used = 0;
    refused = false;
    return mem.grow(bytes, 4, 4096);
  }
  void release() {
    mem.release();
    used = 0;
  }
  static size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  template <typename T>
  T* take(size_t count) {
    const size_t bytes = pad(count * sizeof(T));
    if (bytes > mem.cap - used) {  // used <= cap always: nothing is handed out past the block
      refused = true;
      return nullptr;
    }
    T* p = reinterpret_cast<T*>(mem.as<char>() + used);
    used += bytes;
    return p;
  }
};
struct ArenaCount {  // the arena without memory: the same padding, no addresses
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    used += Arena::pad(count * sizeof(T));
    return nullptr;
  }
};
template <class A, typename T>
void take(A& a, T*& p, size_t count) {  // the element type is the pointer's
  p = a.template take<T>(count);
}
// what layout L takes for these sizes, padded; and what it reserves: that plus its slack
template <class L, class... S>
size_t measure(S... sizes) {
  L l{};
  ArenaCount c;
  l.lay(c, sizes...);
  return c.used;
}
template <class L, class... S>
size_t layout_bytes(S... sizes) {
  return measure<L>(sizes...) + L::kSlack;
}
// lay `l` out in a fresh reservation of `bytes` (a sibling's layout_bytes where the area is deliberately sized by it)
template <class L, class... S>
hipError_t lay_out_in(Arena& ar, size_t bytes, L& l, S... sizes) {
  const hipError_t e = ar.reserve(bytes);
  if (e != hipSuccess) return e;
  l.lay(ar, sizes...);
  return ar.refused ? hipErrorOutOfMemory : hipSuccess;
}
template <class L, class... S>
hipError_t lay_out(Arena& ar, L& l, S... sizes) {
  return lay_out_in(ar, layout_bytes<L>(sizes...), l, sizes...);
}

// A device buffer of an ICP handle (o3s_icp.hip): DevMem's block plus the owning handle's allocation generation, bumped whenever
// the buffer moves or a held block is released — which invalidates every captured graph that has the old address baked in.
// Members are wired where they are declared (`DevBuf d_ref{&alloc_gen};`), so no buffer can be left out; gen null: no captured
// kernel points into the buffer.  Not movable: a buffer stays with its handle.
struct DevBuf : private DevMem {
  using DevMem::as;
  using DevMem::cap;
  using DevMem::p;
  uint64_t* gen = nullptr;
  DevBuf() = default;
  explicit DevBuf(uint64_t* g) : gen(g) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // the first allocation is tight (a 20 M-point map is allocated once); a buffer that has to grow AGAIN belongs to a growing
  // map patch, and every move costs a device-wide synchronisation plus a re-capture of the chain's graph: double it
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (gen) ++*gen;
    return grow(bytes, 8, 256);
  }
  void release() {
    if (p && gen) ++*gen;
    DevMem::release();
  }
};

}  // namespace o3s
