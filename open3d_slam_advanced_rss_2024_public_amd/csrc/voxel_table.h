// voxel_table.h — the packed voxel key and the open-addressing table built on it, stated once for every module of
// cloud_ops.hip that uses them (dense map, overlap selection, occupancy snapshot, pose search, odometry constraints).  gfx950 only.
//
// Key: three 21-bit fields (x | y << 21 | z << 42), each the voxel index + 2^20; an index packs when it lies in the HALF-OPEN range
// [-2^20, 2^20).  kDmEmpty (all ones) is no voxel: a NaN coordinate, or an index beyond the range.
// Table: slot = key + 1 with 0 = empty (so a zeroed table is an empty one), home = low 32 bits of the splitmix64 finaliser of the
// slot value, linear probing, no deletion.  Two shapes: OvSlot (key + a count per layer) and a bare array of slot values.
// The dense map's own table (murmur-style dm_hash, tombstones, filter words) is a different one and lives in dense_map_impl.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace o3s {
namespace devfn {

// ---- key format ----
constexpr uint64_t kDmEmpty = ~0ull;
constexpr int32_t kDmBias = 1 << 20;
// the field of one axis (0 = x, 1 = y, 2 = z) of a packed key; idx must be in range
__device__ __forceinline__ uint64_t dm_field(int32_t idx, int axis) { return (uint64_t)(uint32_t)(idx + kDmBias) << (21 * axis); }
__device__ __forceinline__ int32_t dm_index(uint64_t key, int axis) { return (int32_t)((key >> (21 * axis)) & 0x1fffffull) - kDmBias; }  // ... and back
__device__ __forceinline__ uint64_t dm_pack(int32_t x, int32_t y, int32_t z) { return dm_field(z, 2) | dm_field(y, 1) | dm_field(x, 0); }
__device__ __forceinline__ bool dm_in_range(double f) { return f >= -(double)kDmBias && f < (double)kDmBias; }  // false for NaN
// getVoxelIdx(p, 1 / voxel) (VoxelHashMap.hpp:43-51, the reciprocal form) -> packed key; kDmEmpty: NaN or beyond the packable range
__device__ __forceinline__ uint64_t vm_key(double x, double y, double z, double inv) {
  const double fx = floor(x * inv), fy = floor(y * inv), fz = floor(z * inv);
  return (dm_in_range(fx) && dm_in_range(fy) && dm_in_range(fz)) ? dm_pack((int32_t)fx, (int32_t)fy, (int32_t)fz) : kDmEmpty;
}

// ---- hash ----
__device__ __forceinline__ uint64_t splitmix64(uint64_t k) {  // the finaliser
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return k;
}
__device__ __forceinline__ uint32_t ov_hash(uint64_t k) { return (uint32_t)splitmix64(k); }

// ---- table operations ----
struct __attribute__((aligned(16))) OvSlot {
  unsigned long long key1;  // packed voxel key + 1; 0 = empty
  uint32_t n[2];            // points of the source layer, of the target layer
};
// key's entry in the table, made if need be, with `add` more points of `layer`; 0xffffffff (and *full = 1) when the table is full
__device__ __forceinline__ uint32_t ov_count_key(uint64_t key, OvSlot* __restrict__ tab, uint32_t mask, int layer, uint32_t add, uint32_t* __restrict__ full) {
  const unsigned long long k1 = key + 1ull;
  uint32_t h = ov_hash(k1) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long prev = atomicCAS(&tab[h].key1, 0ull, k1);
    if (prev == 0ull || prev == k1) {
      atomicAdd(&tab[h].n[layer], add);
      return h;
    }
    h = (h + 1u) & mask;
  }
  *full = 1u;
  return 0xffffffffu;
}
// key-only table: claims key's slot or finds it within max_probe steps.  kVmMade: this lane made the entry (exactly one lane of a
// launch does, for every key); kVmFull: no slot within the limit
enum VmClaim { kVmFull = 0, kVmFound = 1, kVmMade = 2 };
__device__ __forceinline__ VmClaim vm_claim(uint64_t key, unsigned long long* __restrict__ tab, uint32_t mask, uint32_t max_probe) {
  const unsigned long long k1 = key + 1ull;
  uint32_t h = ov_hash(k1) & mask;
  for (uint32_t probe = 0; probe < max_probe; ++probe) {
    const unsigned long long prev = atomicCAS(&tab[h], 0ull, k1);
    if (prev == 0ull) return kVmMade;
    if (prev == k1) return kVmFound;
    h = (h + 1u) & mask;
  }
  return kVmFull;
}
// key-only table, read-only: is key there?  (The table is never full: an empty slot ends every miss.)
__device__ __forceinline__ bool vm_find(uint64_t key, const unsigned long long* __restrict__ tab, uint32_t mask) {
  const unsigned long long k1 = key + 1ull;
  uint32_t h = ov_hash(k1) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long v = tab[h];
    if (v == k1) return true;
    if (v == 0ull) break;
    h = (h + 1u) & mask;
  }
  return false;
}

// ---- sizing (the retry policies are their callers') ----
constexpr uint32_t kOvFirstSlots = 1u << 16;
inline uint32_t ov_slots_for(int64_t n_points) {  // room for one voxel per point at half load
  uint32_t c = 1u << 10;
  while ((int64_t)c < 2 * n_points && c < (1u << 31)) c <<= 1;
  return c;
}

}  // namespace devfn
}  // namespace o3s
