// wave_ops.h — the wave-level (wave64) device helpers of both translation units: o3s_icp.hip pulls them into o3s::kern,
// cloud_ops.hip into o3s_cloud (`using namespace o3s::devfn`).  gfx950 only.  Every fp64 helper here fixes an ORDER of additions
// that callers' results depend on bit for bit: a reduction with another tree is another function and does not belong here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace o3s {
namespace devfn {

// Wave-wide sums.  The in-row steps use DPP lane permutes (VALU speed, no LDS crossbar round trip: a ds_bpermute-based
// __shfl tree of a double costs ~12 dependent LDS operations, which dominated the small kernels); the four 16-lane row
// sums are then combined through v_readlane.  Every lane returns the total.
//   quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = dpp_i32<CTRL>(__double2loint(v)), hi = dpp_i32<CTRL>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);   // pairs
  v += dpp_f64<0x4E>(v);   // quads
  v += dpp_f64<0x141>(v);  // 8 lanes
  v += dpp_f64<0x140>(v);  // 16-lane rows
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  v += (uint32_t)dpp_i32<0xB1>((int)v);
  v += (uint32_t)dpp_i32<0x4E>((int)v);
  v += (uint32_t)dpp_i32<0x141>((int)v);
  v += (uint32_t)dpp_i32<0x140>((int)v);
  return ((uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16)) +
         ((uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {  // the total is lane 0's
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Wave-wide min / max before touching a global extremum: one atomic per wave instead of one per point (same-address
// atomics serialise at ~11 ns each — per-point atomics made the bound kernels the largest item of the mapping loop).
__device__ __forceinline__ int32_t wave_min_i32(int32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

// lane `leader`'s 64-bit value in every lane: two 32-bit shuffles
__device__ __forceinline__ uint64_t wave_bcast_u64(uint64_t v, int leader) {
  return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), leader) << 32) | (uint64_t)(uint32_t)__shfl((int)(v & 0xffffffffu), leader);
}

}  // namespace devfn
}  // namespace o3s
