// cloud_bounds.h — the min / max bound of a cloud on the device, read back once: the one encoding, the one replica layout, the one
// accumulate / flush, the one fold and the one fetch.  A section of cloud_dev.h, included there INSIDE namespace o3s_cloud behind the
// wave reductions and the pinned area it uses and in front of the hinted pipelines' kernels; nothing else includes it.
//
// Layout of a bounds block, kBoundsWords u64 words: [kExtSlots][min[3], ~max[3]] replicas, then the six folded bounds.  Every
// replica slot is a MINIMUM of order-preserving bit patterns — a maximum is kept as the minimum of the complemented pattern — so
// that one byte fill (0xFF) initialises them all.  Block b uses replica b % kExtSlots.
#pragma once

// order-preserving map of a double to u64 (so that integer min / max and their atomics order negatives too) and its inverse.  The
// double comes by reference (BoundsAcc::add's too): a value read from memory is then loaded as the integer it is used as, as the
// inline spellings this replaces were; by value the compiler forms fabs / fneg of the double instead (3 VGPRs more in k_bounds).
__host__ __device__ inline unsigned long long ordered_bits(const double& v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double from_ordered_bits(unsigned long long u) {
  u = (u & 0x8000000000000000ull) ? (u & 0x7fffffffffffffffull) : ~u;
  return __builtin_bit_cast(double, u);
}

constexpr int kBoundsReplicaWords = kExtSlots * 6, kBoundsWords = kBoundsReplicaWords + 6;

// what one thread has seen: a thread folds its points first, so that a wave reduces once per kernel and not once per point (the
// reduction's 72 lane permutes were the kernel: 35 us at 0.76 M points).  kMax = false keeps the minima only: at one point per lane
// (a sweep) the kernel is its six dependent look-and-atomic trips per wave, and a caller that wants the anchor alone pays three.
template <bool kMax = true>
struct BoundsAcc {
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  __device__ __forceinline__ void add(const double& x, const double& y, const double& z) {
    const unsigned long long u[3] = {ordered_bits(x), ordered_bits(y), ordered_bits(z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = u[a] < lo[a] ? u[a] : lo[a];
      if constexpr (kMax) hi[a] = u[a] > hi[a] ? u[a] : hi[a];
    }
  }
};
// wave reduction, then a (possibly stale) look before the atomic into this block's replica: extrema are monotone, so skipping is
// safe.  Reached by every lane of the wave; a wave that saw no point (lo = ~0 > hi = 0) writes nothing.  Without kMax the ~max
// slots keep their fill.
template <bool kMax>
__device__ __forceinline__ void bounds_flush(const BoundsAcc<kMax>& acc, unsigned long long* __restrict__ slots) {
  unsigned long long* mnmx = slots + 6 * (blockIdx.x & (kExtSlots - 1));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const unsigned long long l = wave_min_u64(acc.lo[a]), h = kMax ? wave_max_u64(acc.hi[a]) : ~0ull;
    if ((threadIdx.x & 63) == 0 && l <= h) {
      if (l < __atomic_load_n(&mnmx[a], __ATOMIC_RELAXED)) atomicMin(&mnmx[a], l);
      if constexpr (kMax)
        if (~h < __atomic_load_n(&mnmx[3 + a], __ATOMIC_RELAXED)) atomicMin(&mnmx[3 + a], ~h);
    }
  }
}

// A point source says where point i of a cloud comes from: open() is reached by EVERY thread of the block before any of them
// returns (a source may fill LDS behind a barrier there) and gives what at(i), the address of the point's three doubles, is asked of.
struct FlatPoints {  // one array, 3 x N doubles
  const double* __restrict__ pts;
  __device__ __forceinline__ FlatPoints open() const { return *this; }
  __device__ __forceinline__ const double* at(int64_t i) const { return pts + 3 * i; }
};

// blocks stride over the cloud: any grid is valid (cloud_bounds launches min(nblk(N), 1024) blocks)
template <class Src, bool kMax>
__global__ void __launch_bounds__(kB) k_bounds(Src src, int64_t N, unsigned long long* __restrict__ slots) {
  const auto cloud = src.open();
  BoundsAcc<kMax> acc;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < N; i += (int64_t)gridDim.x * kB) {
    const double* p = cloud.at(i);
    acc.add(p[0], p[1], p[2]);
  }
  bounds_flush(acc, slots);
}

// the six bounds of the kExtSlots replicas (one per lane; the maxima un-complemented), as lane 0 holds them
__device__ __forceinline__ void fold_bounds(const unsigned long long* __restrict__ slots, unsigned long long (&v)[6]) {
  static_assert(kExtSlots == 64, "one replica per lane");
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    v[a] = wave_min_u64(slots[threadIdx.x * 6 + a]);
    if (a >= 3) v[a] = ~v[a];
  }
}
// folds the replicas of a bounds block into its last six words (the copy a drained wait falls back to) and posts them (8-byte
// values from kPostVals, then the sequence number; mailbox nullable)
__global__ void __launch_bounds__(64) k_bounds_post(unsigned long long* __restrict__ block, uint32_t* __restrict__ mailbox, uint32_t seq) {
  if (blockIdx.x != 0) return;
  unsigned long long v[6];
  fold_bounds(block, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int a = 0; a < 6; ++a) block[kBoundsReplicaWords + a] = v[a];
  if (mailbox) post(mailbox, seq, kPostVals, v);
}

// host side: the fill before the accumulating kernel, and the one read-back behind it — out[0..2] the minima, out[3..5] the maxima,
// as ordered bit patterns.  The host never folds replicas.
inline int bounds_begin(unsigned long long* block, hipStream_t s) {
  CK(hipMemsetAsync(block, 0xFF, (size_t)kBoundsReplicaWords * 8, s));
  return O3S_OK;
}
inline int bounds_fetch(unsigned long long* block, hipStream_t s, unsigned long long out[6]) {
  PinnedArea& pa = pinned_area();
  const uint32_t seq = mailbox_open(pa);
  hipLaunchKernelGGL(k_bounds_post, dim3(1), dim3(64), 0, s, block, seq ? pa.mb.dev : (uint32_t*)nullptr, seq);
  CK(hipGetLastError());
  if (fetch_post(pa.mb, seq, s, reinterpret_cast<uint32_t*>(out), 12, kPostVals, block + kBoundsReplicaWords, pa.p) == kPollError) return O3S_ERR_HIP;
  return O3S_OK;
}
// the bounds of the N > 0 points of `src`; block: kBoundsWords words of device memory.  kMax = false: out[3..5] mean nothing
template <bool kMax = true, class Src>
inline int cloud_bounds(const Src& src, int64_t N, unsigned long long* block, hipStream_t s, unsigned long long out[6]) {
  const int rc = bounds_begin(block, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL((k_bounds<Src, kMax>), dim3(std::min(nblk(N), 1024u)), dim3(kB), 0, s, src, N, block);
  return bounds_fetch(block, s, out);
}
