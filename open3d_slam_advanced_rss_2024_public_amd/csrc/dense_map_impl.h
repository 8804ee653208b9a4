// dense_map_impl.h — device-resident dense map (C ABI: include/o3s_dense_map.h), gfx950 only.  Included at the end of
// cloud_ops.hip after submap_impl.h (one TU: shared kernels, one instantiation of the rocPRIM sort / scan).
//
// The reference's VoxelizedPointCloud is an unordered_map<Vector3i, AggregatedVoxel> filled point by point
// (O3S/src/Voxel.cpp:66-88).  Here it is an open-addressing table in HBM (linear probing, load <= 1/2, tombstones):
//   keys[cap] u64 | cnt[cap] i32 | sum[cap][6] f64 (position xyz, normal xyz) | csum[cap][3] f64 (colour; only once a
//   coloured cloud has been aggregated, include/dense_map/o3s_dense_map_color.h)
// An insert sorts the new points by packed voxel key (stable, so a voxel's points stay in input order), and ONE lane per
// distinct key claims / finds the slot (64-bit CAS) and adds its points one after the other — the same additions in the
// same order as the reference's loop, hence bit-identical sums, and no two lanes ever touch the same slot.
// Carving (O3S/src/helpers.cpp:360-390) is a lookup-only ray march: one lane per ray, existence tests against the table,
// hits flagged per slot, and a second kernel turns the flagged slots into tombstones.
#pragma once
#include "../../include/o3s_dense_map.h"
#include "../../include/dense_map/o3s_dense_map_color.h"

#include "cloud_dev.h"
#include "voxel_table.h"

namespace {

// the packed key (kDmEmpty, dm_pack, dm_field, dm_in_range, vm_key) is voxel_table.h's; the table here is this map's own
constexpr uint64_t kDmTomb = ~0ull - 1ull;
constexpr int kDmMaxOff = 16;  // neighbourhood offsets per axis: radius / voxel <= 7.5

__device__ __forceinline__ uint64_t dm_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
__device__ __forceinline__ uint64_t dm_home(uint64_t key, uint64_t mask) { return dm_hash(key) & mask; }
// Occupancy filter for the carving march, rebuilt from the table before every carve: one 64-bit word per 4 x 4 x 4 block
// of voxels (word = hash of the block, bit = position inside), so a stop's whole neighbourhood is answered by the few
// words its blocks hash to and the table is probed only where a bit is set.  Colliding blocks OR their bits: a set bit
// may be a false alarm (the table decides), a clear bit is always right.  A second array under an independent hash is
// consulted only when the first says "maybe": measured on the bench, one array alone sent 5 % of all free-space
// questions on to the table (65 M probes per carve for 0.1 M voxels actually found).
__device__ __forceinline__ uint64_t dm_block(uint64_t key) {
  return ((key >> 2) & 0x7ffffull) | (((key >> 23) & 0x7ffffull) << 19) | (((key >> 44) & 0x7ffffull) << 38);
}
__device__ __forceinline__ uint64_t dm_hash2(uint64_t b) { return dm_hash(b ^ 0x9e3779b97f4a7c15ull); }
__device__ __forceinline__ unsigned dm_bit(uint64_t key) {
  return (unsigned)((key & 3ull) | (((key >> 21) & 3ull) << 2) | (((key >> 42) & 3ull) << 4));
}
__device__ __forceinline__ uint64_t dm_load(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// slot of `key`, or -1; the table always holds an empty slot (load <= 1/2), so the probe ends
__device__ __forceinline__ int64_t dm_find(const uint64_t* __restrict__ keys, uint64_t mask, uint64_t key) {
  uint64_t h = dm_home(key, mask);
  for (;;) {
    const uint64_t k = dm_load(keys + h);
    if (k == key) return (int64_t)h;
    if (k == kDmEmpty) return -1;
    h = (h + 1) & mask;
  }
}

// one lane of a wave adds the wave's count to a global counter (same-address atomics serialise at ~11 ns each)
__device__ __forceinline__ void wave_count(bool flag, uint32_t* counter) {
  const uint64_t b = __ballot(flag);
  if (b && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(counter, (uint32_t)__builtin_popcountll(b));
}

// getVoxelIdx(p, InverseVoxelSize) (VoxelHashMap.hpp:48-51) -> packed key; out-of-range points raise err and sort last
__global__ void __launch_bounds__(kB) k_dm_keys(const double* __restrict__ pts, int64_t N, double inv, uint64_t* __restrict__ keys,
                                                uint32_t* __restrict__ vals, uint32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  const uint64_t k = vm_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], inv);
  vals[i] = (uint32_t)i;
  keys[i] = k;
  if (k == kDmEmpty) *err = 1u;
}

// VoxelizedPointCloud::insert (Voxel.cpp:66-88) on key-sorted points: one lane per distinct key.
// counters: [0] slots newly occupied, [1] of those, how many re-used a tombstone
// kCol: the map holds colour sums (csum).  A slot claimed here starts its colour sum at (1, 1, 1) — AggregatedVoxel's initialiser
// (Voxel.hpp:50), restated as it is — whether or not this cloud has colours (col nullable), so a re-used tombstone never shows the
// sum of the voxel that was carved away; aggregateColor (Voxel.cpp:34-36) then adds in input order like the other two sums.
// kCol == false is the kernel as it was before colours: no further load, store or register.
template <bool kCol>
__global__ void __launch_bounds__(kB) k_dm_insert(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ svals, int64_t N,
                                                  const double* __restrict__ pts, const double* __restrict__ nrm, const double* __restrict__ col,
                                                  uint64_t* __restrict__ keys, int32_t* __restrict__ cnt, double* __restrict__ sum,
                                                  double* __restrict__ csum, uint64_t mask, uint32_t* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  bool is_new = false, from_tomb = false;
  if (i < N) {
    const uint64_t key = skeys[i];
    if (key != kDmEmpty && (i == 0 || skeys[i - 1] != key)) {
      // find the key, else claim the first tombstone seen on the probe path, else the empty slot that ended the probe
      const uint64_t h0 = dm_home(key, mask);
      uint64_t h = h0;
      int64_t tomb = -1, slot = -1;
      for (;;) {
        const uint64_t k = dm_load(keys + h);
        if (k == key) {
          slot = (int64_t)h;
          break;
        }
        if (k == kDmTomb && tomb < 0) tomb = (int64_t)h;
        if (k == kDmEmpty) {
          const uint64_t target = tomb >= 0 ? (uint64_t)tomb : h;
          const uint64_t expect = tomb >= 0 ? kDmTomb : kDmEmpty;
          const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(keys + target), (unsigned long long)expect, (unsigned long long)key);
          if (old == expect) {
            slot = (int64_t)target;
            is_new = true;
            from_tomb = tomb >= 0;
            break;
          }
          h = h0;  // another key took that slot: probe again (this key is still ours alone to insert)
          tomb = -1;
          continue;
        }
        h = (h + 1) & mask;
      }
      double s[6] = {0, 0, 0, 0, 0, 0};
      [[maybe_unused]] double cs[3] = {1.0, 1.0, 1.0};
      int32_t c = 0;
      if (!is_new) {
        c = cnt[slot];
#pragma unroll
        for (int a = 0; a < 6; ++a) s[a] = sum[6 * slot + a];
        if constexpr (kCol) {
          if (col) {
#pragma unroll
            for (int a = 0; a < 3; ++a) cs[a] = csum[3 * slot + a];
          }
        }
      }
      for (int64_t j = i; j < N && skeys[j] == key; ++j) {  // aggregatePoint, aggregateNormal (Voxel.cpp:27-33), input order
        const int64_t p = svals[j];
        s[0] += pts[3 * p];
        s[1] += pts[3 * p + 1];
        s[2] += pts[3 * p + 2];
        ++c;
        if (nrm) {
          s[3] += nrm[3 * p];
          s[4] += nrm[3 * p + 1];
          s[5] += nrm[3 * p + 2];
        }
        if constexpr (kCol) {
          if (col) {
            cs[0] += col[3 * p];
            cs[1] += col[3 * p + 1];
            cs[2] += col[3 * p + 2];
          }
        }
      }
      cnt[slot] = c;
#pragma unroll
      for (int a = 0; a < 6; ++a) sum[6 * slot + a] = s[a];
      if constexpr (kCol) {
        if (is_new || col) {
#pragma unroll
          for (int a = 0; a < 3; ++a) csum[3 * slot + a] = cs[a];
        }
      }
    }
  }
  wave_count(is_new, counters);
  wave_count(from_tomb, counters + 1);
}

// moves every live slot into a fresh (all-empty) table; ocsum / csum: the colour sums, both null while the map has none
__global__ void __launch_bounds__(kB) k_dm_rehash(const uint64_t* __restrict__ okeys, const int32_t* __restrict__ ocnt, const double* __restrict__ osum,
                                                  const double* __restrict__ ocsum, int64_t ocap, uint64_t* __restrict__ keys,
                                                  int32_t* __restrict__ cnt, double* __restrict__ sum, double* __restrict__ csum, uint64_t mask) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= ocap) return;
  const uint64_t key = okeys[i];
  if (key == kDmEmpty || key == kDmTomb) return;
  uint64_t h = dm_home(key, mask);
  for (;;) {
    if (dm_load(keys + h) == kDmEmpty &&
        atomicCAS(reinterpret_cast<unsigned long long*>(keys + h), (unsigned long long)kDmEmpty, (unsigned long long)key) == kDmEmpty)
      break;
    h = (h + 1) & mask;
  }
  cnt[h] = ocnt[i];
#pragma unroll
  for (int a = 0; a < 6; ++a) sum[6 * h + a] = osum[6 * i + a];
  if (ocsum) {
#pragma unroll
    for (int a = 0; a < 3; ++a) csum[3 * h + a] = ocsum[3 * i + a];
  }
}

// the colour sums of a map that meets its first colour: every voxel, alive or yet to come, has held (1, 1, 1) all along
__global__ void __launch_bounds__(kB) k_dm_fill_ones(double* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i < n) v[i] = 1.0;
}

// toPointCloud (Voxel.cpp:90-114): voxels with numAggregatedPoints_ > 0
__global__ void __launch_bounds__(kB) k_dm_live(const uint64_t* __restrict__ keys, const int32_t* __restrict__ cnt, int64_t cap,
                                                uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= cap) return;
  const uint64_t k = keys[i];
  flag[i] = (k != kDmEmpty && k != kDmTomb && cnt[i] > 0) ? 1u : 0u;
}
__global__ void __launch_bounds__(kB) k_dm_collect(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off,
                                                   int64_t cap, uint64_t* __restrict__ okeys, uint32_t* __restrict__ oslots) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= cap || !flag[i]) return;
  okeys[off[i]] = keys[i];
  oslots[off[i]] = (uint32_t)i;
}
__global__ void __launch_bounds__(kB) k_dm_emit(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ sslots, int64_t V,
                                                const int32_t* __restrict__ cnt, const double* __restrict__ sum, const double* __restrict__ csum,
                                                double* __restrict__ out_p, double* __restrict__ out_n, double* __restrict__ out_col /*with csum*/,
                                                int32_t* __restrict__ out_k, int32_t* __restrict__ out_c) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= V) return;
  const uint64_t key = skeys[i];
  const int64_t s = sslots[i];
  const int32_t c = cnt[s];
  const double d = (double)c;  // aggregatedPosition_ / numAggregatedPoints_ (Voxel.cpp:18-23)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out_p[3 * i + a] = sum[6 * s + a] / d;
    out_n[3 * i + a] = sum[6 * s + 3 + a] / d;
  }
  if (csum) {  // getAggregatedColor (Voxel.cpp:24-26): the sum that began at (1, 1, 1), over ALL points of the voxel
#pragma unroll
    for (int a = 0; a < 3; ++a) out_col[3 * i + a] = csum[3 * s + a] / d;
  }
  out_k[3 * i] = dm_index(key, 0);
  out_k[3 * i + 1] = dm_index(key, 1);
  out_k[3 * i + 2] = dm_index(key, 2);
  out_c[i] = c;
}

// VoxelizedPointCloud::transform (Voxel.cpp:49-64): Isometry3d * Vector3d = translation + linear * v on both sums; the voxel is
// copied, so its colour sum stays.  t + ((T0 x + T1 y) + T2 z), no division: another order than o3d_transform_point's, so it stays
__global__ void __launch_bounds__(kB) k_dm_transform(const uint64_t* __restrict__ keys, const int32_t* __restrict__ cnt, double* __restrict__ sum,
                                                     int64_t cap, const double* __restrict__ Tm) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= cap) return;
  const uint64_t k = keys[i];
  if (k == kDmEmpty || k == kDmTomb || cnt[i] <= 0) return;
  double T[16];
#pragma unroll
  for (int a = 0; a < 16; ++a) T[a] = Tm[a];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const double x = sum[6 * i + 3 * g], y = sum[6 * i + 3 * g + 1], z = sum[6 * i + 3 * g + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) sum[6 * i + 3 * g + r] = T[12 + r] + ((T[r] * x + T[4 + r] * y) + T[8 + r] * z);
  }
}

// removeDuplicatePointsWithinSameVoxels (Voxel.cpp:162-192) on key-sorted points: the first point of every voxel
__global__ void __launch_bounds__(kB) k_dm_heads(const uint64_t* __restrict__ skeys, int64_t N, uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  const uint64_t k = skeys[i];
  head[i] = (k != kDmEmpty && (i == 0 || skeys[i - 1] != k)) ? 1u : 0u;
}
__global__ void __launch_bounds__(kB) k_dm_first(const uint32_t* __restrict__ svals, const uint32_t* __restrict__ head, const uint32_t* __restrict__ off,
                                                 int64_t N, uint32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i < N && head[i]) first[off[i]] = svals[i];
}

// ColorRangeCropper::isValidColor (croppers.cpp:178-180): min <= c && c <= max in every component, so a NaN fails
struct DmRgb {
  double lo[3], hi[3];
};
// flag[i] = 1 for a point with a valid colour that, with use_volume, also lies inside the cropping volume: denseMapCropper_->crop
// followed by colorCropper_.crop (Submap.cpp:100-101) are two order-preserving filters, hence one predicate
__global__ void __launch_bounds__(kB) k_dm_color_mask(o3s_cropper c, int use_volume, const double* __restrict__ pts, const double* __restrict__ col,
                                                      int64_t N, DmRgb b, uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = col[3 * i + a];
    ok = ok && b.lo[a] <= v && v <= b.hi[a];
  }
  if (ok && use_volume) ok = within(c, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
  flag[i] = ok ? 1u : 0u;
}
// the scatter of that crop: points, normals (nullable) and colours in one pass
__global__ void __launch_bounds__(kB) k_dm_compact_col(const double* __restrict__ pts, const double* __restrict__ nrm, const double* __restrict__ col,
                                                       int64_t N, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off,
                                                       double* __restrict__ out_p, double* __restrict__ out_n, double* __restrict__ out_c) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N || !flag[i]) return;
  const int64_t o = (int64_t)off[i];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out_p[3 * o + a] = pts[3 * i + a];
    if (nrm) out_n[3 * o + a] = nrm[3 * i + a];
    out_c[3 * o + a] = col[3 * i + a];
  }
}

__global__ void __launch_bounds__(kB) k_dm_build_filter(const uint64_t* __restrict__ keys, int64_t cap, unsigned long long* __restrict__ words,
                                                        uint64_t wmask) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= cap) return;
  const uint64_t k = keys[i];
  if (k == kDmEmpty || k == kDmTomb) return;
  const uint64_t b = dm_block(k);
  atomicOr(words + (dm_hash(b) & wmask), 1ull << dm_bit(k));
  atomicOr(words + (wmask + 1) + (dm_hash2(b) & wmask), 1ull << dm_bit(k));  // the second array follows the first
}

struct DmOffsets {
  int n;
  double d[kDmMaxOff];  // the values the reference's `for (dx = -r; dx <= r; dx += step)` loop takes (VoxelHashMap.cpp:24)
};

// getKeysOfCarvedPoints (helpers.cpp:360-390) with getVoxelsWithinPointNeighborhood (VoxelHashMap.cpp:13-46) inlined:
// one lane per ray, the reference's sequential march; every existing voxel it names gets rm[slot] = 1.
// A packed key is the OR of three per-axis parts, so each stop forms per axis (n values each): the shifted key part
// (bit 63 set when the index is out of range) and the squared offset from the voxel centre — 3 n divisions instead of
// n^3 — and the n^3 combinations cost an OR, an add and a compare each.  NX > 0: n == NX is known at compile time, the
// x tables stay in registers and the innermost loop is unrolled; NX == 0: any n <= kDmMaxOff.
// kDmRayLanes lanes share a ray: lane j takes stops j, j + kDmRayLanes, ... (every lane forms `distance` by the same
// repeated addition as the reference, so the stops are the same numbers).  120 k rays alone leave the chip at 2 waves per
// SIMD waiting on dependent look-ups; eight lanes per ray fill it.
constexpr int kDmRayLanes = 8;
constexpr uint64_t kDmBad = 1ull << 63;
#ifdef O3S_DM_STATS
__device__ unsigned long long g_dm_stats[4];  // stops, in-radius combinations, filter hits, voxels found
#endif
template <int NX>
__global__ void __launch_bounds__(kB) k_dm_carve_rays(const double* __restrict__ scan, const uint32_t* __restrict__ first, int64_t n_first, double sx,
                                                      double sy, double sz, double voxel, double radius, double r2lo, double r2hi, double step,
                                                      double max_len, double trunc, DmOffsets off, const uint64_t* __restrict__ keys, uint64_t mask,
                                                      const uint64_t* __restrict__ words, uint64_t wmask, uint8_t* __restrict__ rm) {
  constexpr int CAPX = NX > 0 ? NX : kDmMaxOff;
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= n_first * kDmRayLanes) return;
  const int sub = (int)(t % kDmRayLanes);
  const int64_t i = first[t / kDmRayLanes];
  const double dx = scan[3 * i] - sx, dy = scan[3 * i + 1] - sy, dz = scan[3 * i + 2] - sz;
  const double length = sqrt((dx * dx + dy * dy) + dz * dz);
  if (!(length > 0.0)) return;  // NaN direction (a return at the sensor, or a NaN point): no voxel can be addressed
  const double ux = dx / length, uy = dy / length, uz = dz / length;
  const double max_path = fmax(step, fmin(length - trunc, max_len));
  const double half = voxel * 0.5;
  const int n = NX > 0 ? NX : off.n;
  uint64_t blk[2] = {~0ull, ~0ull}, wrd[2] = {0, 0};  // the two filter words used last (x runs straddle two blocks)
  auto maybe_there = [&](uint64_t key) -> bool {
    const uint64_t b = dm_block(key);
    if (b != blk[0]) {
      if (b == blk[1]) {
        const uint64_t tb = blk[0], tw = wrd[0];
        blk[0] = blk[1];
        wrd[0] = wrd[1];
        blk[1] = tb;
        wrd[1] = tw;
      } else {
        blk[1] = blk[0];
        wrd[1] = wrd[0];
        blk[0] = b;
        wrd[0] = words[dm_hash(b) & wmask];
      }
    }
    return (wrd[0] >> dm_bit(key)) & 1ull;
  };
#ifdef O3S_DM_STATS
  unsigned long long st_stops = 0, st_in = 0, st_fhit = 0, st_found = 0;
#endif
  auto probe = [&](uint64_t key) {
#ifdef O3S_DM_STATS
    ++st_in;
#endif
    if (!maybe_there(key)) return;
    if (!((words[(wmask + 1) + (dm_hash2(dm_block(key)) & wmask)] >> dm_bit(key)) & 1ull)) return;
    const int64_t s = dm_find(keys, mask, key);
#ifdef O3S_DM_STATS
    ++st_fhit;
    if (s >= 0) ++st_found;
#endif
    if (s >= 0) rm[s] = 1;
  };
  // key part and squared centre offset of one test coordinate
  auto axis = [&](double tq, int ax, uint64_t& part, double& e2) {
    const double f = floor(tq / voxel);                          // getVoxelIdx(p, voxelSize): the dividing form
    const double e = tq - ((double)(int32_t)f * voxel + half);   // getVoxelCenter = key * voxel + voxel * 0.5
    e2 = e * e;
    part = dm_in_range(f) ? dm_field((int32_t)f, ax) : kDmBad;
  };
  double distance = 0.0;
  for (int k = 0; k < sub && distance < max_path; ++k) distance += step;  // this lane's first stop
  while (distance < max_path) {
    const double cx = distance * ux + sx, cy = distance * uy + sy, cz = distance * uz + sz;
    uint64_t px[CAPX], py[kDmMaxOff], pz[kDmMaxOff];
    double ex2[CAPX], ey2[kDmMaxOff], ez2[kDmMaxOff];
    if constexpr (NX > 0) {
#pragma unroll
      for (int q = 0; q < NX; ++q) axis(cx + off.d[q], 0, px[q], ex2[q]);
    } else {
      for (int q = 0; q < n; ++q) axis(cx + off.d[q], 0, px[q], ex2[q]);
    }
    for (int q = 0; q < n; ++q) {
      axis(cy + off.d[q], 1, py[q], ey2[q]);
      axis(cz + off.d[q], 2, pz[q], ez2[q]);
    }
    uint64_t ckey;
    {
      uint64_t a, b, c;
      double unused;
      axis(cx, 0, a, unused);
      axis(cy, 1, b, unused);
      axis(cz, 2, c, unused);
      ckey = a | b | c;
    }
    bool centre_added = false;
    for (int qz = 0; qz < n; ++qz)
      for (int qy = 0; qy < n; ++qy) {
        const uint64_t pyz = py[qy] | pz[qz];
        const double y2 = ey2[qy], z2 = ez2[qz];
        auto combo = [&](int qx) {
          // (testPoint - center).norm() <= radius: the square root is only taken inside a 1e-14 band around radius^2
          const double v = (ex2[qx] + y2) + z2;
          if (!(v <= r2lo || (v <= r2hi && sqrt(v) <= radius))) return;
          const uint64_t key = px[qx] | pyz;
          if (key == ckey) centre_added = true;
          if (key & kDmBad) return;  // a voxel outside the index range cannot be in the map
          probe(key);
        };
        if constexpr (NX > 0) {
#pragma unroll
          for (int qx = 0; qx < NX; ++qx) combo(qx);
        } else {
          for (int qx = 0; qx < n; ++qx) combo(qx);
        }
      }
    if (!centre_added && !(ckey & kDmBad)) probe(ckey);
    for (int k = 0; k < kDmRayLanes && distance < max_path; ++k) distance += step;  // the lane's next stop
#ifdef O3S_DM_STATS
    ++st_stops;
#endif
  }
#ifdef O3S_DM_STATS
  atomicAdd(g_dm_stats + 0, st_stops);
  atomicAdd(g_dm_stats + 1, st_in);
  atomicAdd(g_dm_stats + 2, st_fhit);
  atomicAdd(g_dm_stats + 3, st_found);
#endif
}

// removeKey for every flagged slot; one lane looks at eight flags at a time (cap is a power of two >= 2^16)
__global__ void __launch_bounds__(kB) k_dm_apply_remove(const uint8_t* __restrict__ rm, uint64_t* __restrict__ keys, int64_t cap,
                                                        uint32_t* __restrict__ counter /*16 replicas, summed by the host*/) {
  const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (g * 8 >= cap) return;
  const uint64_t w = reinterpret_cast<const uint64_t*>(rm)[g];
  if (!w) return;
  uint32_t n = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b)
    if ((w >> (8 * b)) & 0xffull) {
      keys[g * 8 + b] = kDmTomb;
      ++n;
    }
  atomicAdd(counter + (blockIdx.x & 15), n);
}

}  // namespace

struct o3s_dense_map {
  int device = 0;
  double voxel = 0.0, inv = 0.0;
  hipStream_t stream = nullptr;
  DevMem keys, cnt, sum;  // the table
  DevMem csum;            // its colour sums: empty until a coloured cloud is aggregated (dm_ensure_colors)
  int64_t cap = 0, live = 0, tomb = 0;
  int has_normals = 0, has_colors = 0;
  int64_t n_scans_inserted = 0;  // nScansInsertedDenseMap_
  mutable DevMem in_p, in_n, in_c, crop_p, crop_n, crop_c, tf_p, tf_n, d_T, d_ctr, out;
  mutable Arena arena;
  uint64_t* K() const { return keys.as<uint64_t>(); }
  int32_t* C() const { return cnt.as<int32_t>(); }
  double* S() const { return sum.as<double>(); }
  double* CS() const { return csum.as<double>(); }  // null while the map holds no colour sums
};

namespace {

// makes room for `add` more voxels at load <= 1/2, re-hashing into a larger (or tombstone-free) table when needed
int dm_reserve(o3s_dense_map* m, int64_t add) {
  hipStream_t s = m->stream;
  if (m->cap > 0 && 2 * (m->live + m->tomb + add) <= m->cap) return O3S_OK;
  int64_t ncap = 1 << 16;
  while (ncap < 4 * (m->live + add)) ncap <<= 1;
  DevMem nk, nc, ns, ncs;  // released on every early return; handed to the map at the end
  CK(nk.alloc((size_t)ncap * 8));
  CK(nc.alloc((size_t)ncap * 4));
  CK(ns.alloc((size_t)ncap * 48));
  const bool colors = m->csum.p != nullptr;  // slots nobody holds need no value: k_dm_insert<true> writes a colour sum as it claims
  if (colors) CK(ncs.alloc((size_t)ncap * 24));
  CK(hipMemsetAsync(nk.p, 0xff, (size_t)ncap * 8, s));
  if (m->cap > 0 && m->live > 0) {
    hipLaunchKernelGGL(k_dm_rehash, dim3(nblk(m->cap)), dim3(kB), 0, s, m->K(), m->C(), m->S(), m->CS(), m->cap, nk.as<uint64_t>(),
                       nc.as<int32_t>(), ns.as<double>(), ncs.as<double>(), (uint64_t)(ncap - 1));
    CK(hipGetLastError());
  }
  CK(hipStreamSynchronize(s));
  m->keys = std::move(nk);  // the old table is freed as the new one moves in
  m->cnt = std::move(nc);
  m->sum = std::move(ns);
  if (colors) m->csum = std::move(ncs);
  m->cap = ncap;
  m->tomb = 0;
  return O3S_OK;
}

// work area of an insert: the keys of n points and their stable sort (tb: room for the sort and for a scan of n flags)
struct DmSortArea {
  static constexpr size_t kSlack = 4096;
  uint64_t *keys, *skeys;  // s...: sorted
  uint32_t *vals, *svals;
  char* tmp;
  template <class A>
  void lay(A& a, size_t n, size_t tb) {
    take(a, keys, n);
    take(a, skeys, n);
    take(a, vals, n);
    take(a, svals, n);
    take(a, tmp, tb);
  }
};
// work area of carving: the sorted scan keys, then the first point of each scan voxel, the removal marks of a table of
// `cap` slots and the two arrays of the occupancy filter
struct DmCarveArea {
  static constexpr size_t kSlack = DmSortArea::kSlack;
  DmSortArea sort;
  uint32_t *head, *ord, *first;
  uint8_t* rm;
  unsigned long long* words;  // two arrays of nwords
  template <class A>
  void lay(A& a, size_t n, size_t tb, size_t cap, size_t nwords) {
    sort.lay(a, n, tb);
    take(a, head, n);
    take(a, ord, n + 1);
    take(a, first, n);
    take(a, rm, cap);
    take(a, words, nwords * 2);
  }
};
// work area of the export: the live slots of a table of `cap`, the sort of the v live voxels by key, and what is emitted
struct DmExportArea {
  static constexpr size_t kSlack = 4096;
  uint32_t *flag, *off;
  uint64_t *k1, *k2;
  uint32_t *s1, *s2;
  char* tmp;
  double *op, *on;
  int32_t *ok, *oc;
  double* ocol = nullptr;  // only when colours are asked for
  template <class A>
  void lay(A& a, size_t cap, size_t v, size_t tb, bool colors) {
    take(a, flag, cap);
    take(a, off, cap + 1);
    take(a, k1, v);
    take(a, k2, v);
    take(a, s1, v);
    take(a, s2, v);
    take(a, tmp, tb);
    take(a, op, v * 3);
    take(a, on, v * 3);
    take(a, ok, v * 3);
    take(a, oc, v);
    if (colors) take(a, ocol, v * 3);
  }
};
inline size_t dm_sort_temp_bytes(int64_t N) { return std::max(sort_temp_bytes(N), scan_temp_bytes(N)); }

// keys of a device cloud, stably sorted, in a work area laid out for N points and tb = dm_sort_temp_bytes(N)
int dm_sorted_keys(o3s_dense_map* m, const double* d_pts, int64_t N, const DmSortArea& w, size_t tb) {
  hipStream_t s = m->stream;
  CK(m->d_ctr.ensure(64, 0, s));
  CK(hipMemsetAsync(m->d_ctr.p, 0, 64, s));
  uint32_t* ctr = reinterpret_cast<uint32_t*>(m->d_ctr.p);
  hipLaunchKernelGGL(k_dm_keys, dim3(nblk(N)), dim3(kB), 0, s, d_pts, N, m->inv, w.keys, w.vals, ctr + 8);
  CK(rocprim::radix_sort_pairs(w.tmp, tb, w.keys, w.skeys, w.vals, w.svals, (size_t)N, 0, 64, s));
  return O3S_OK;
}

int dm_read_counters(o3s_dense_map* m, uint32_t out[16]) {
  CK(hipMemcpyAsync(out, m->d_ctr.p, 64, hipMemcpyDeviceToHost, m->stream));
  CK(hipStreamSynchronize(m->stream));
  return O3S_OK;
}

// The colour sums come into being with the first insert that needs them: a coloured cloud, or any cloud into a map whose
// isHasColors_ outlived a clear().  All of them 1.0: that is what every voxel of the reference has held since it was made.
int dm_ensure_colors(o3s_dense_map* m) {
  if (m->csum.p) return O3S_OK;
  DevMem cs;
  CK(cs.alloc((size_t)m->cap * 24));
  hipLaunchKernelGGL(k_dm_fill_ones, dim3(nblk(3 * m->cap)), dim3(kB), 0, m->stream, cs.as<double>(), 3 * m->cap);
  CK(hipGetLastError());
  m->csum = std::move(cs);
  return O3S_OK;
}

// VoxelizedPointCloud::insert on a device cloud; d_nrm, d_col: nullable
int dm_insert_dev(o3s_dense_map* m, const double* d_pts, const double* d_nrm, const double* d_col, int64_t N) {
  if (N == 0) return O3S_OK;
  if (N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  hipStream_t s = m->stream;
  int rc = dm_reserve(m, N);
  if (rc != O3S_OK) return rc;
  const size_t tb = dm_sort_temp_bytes(N);
  DmSortArea w;
  CK(lay_out(m->arena, w, (size_t)N, tb));
  rc = dm_sorted_keys(m, d_pts, N, w, tb);
  if (rc != O3S_OK) return rc;
  uint32_t ctr[16];
  rc = dm_read_counters(m, ctr);  // the range check has to be known before the table is touched
  if (rc != O3S_OK) return rc;
  if (ctr[8]) return O3S_ERR_BAD_ARGUMENT;
  if (d_col || m->has_colors) {
    rc = dm_ensure_colors(m);
    if (rc != O3S_OK) return rc;
  }
  if (m->csum.p) {
    hipLaunchKernelGGL(k_dm_insert<true>, dim3(nblk(N)), dim3(kB), 0, s, w.skeys, w.svals, N, d_pts, d_nrm, d_col, m->K(), m->C(), m->S(), m->CS(),
                       (uint64_t)(m->cap - 1), reinterpret_cast<uint32_t*>(m->d_ctr.p));
  } else {
    hipLaunchKernelGGL(k_dm_insert<false>, dim3(nblk(N)), dim3(kB), 0, s, w.skeys, w.svals, N, d_pts, d_nrm, (const double*)nullptr, m->K(), m->C(),
                       m->S(), (double*)nullptr, (uint64_t)(m->cap - 1), reinterpret_cast<uint32_t*>(m->d_ctr.p));
  }
  CK(hipGetLastError());
  rc = dm_read_counters(m, ctr);
  if (rc != O3S_OK) return rc;
  m->live += ctr[0];
  m->tomb -= ctr[1];
  if (d_nrm) m->has_normals = 1;  // isHasNormals_ (Voxel.cpp:80-82)
  if (d_col) m->has_colors = 1;   // isHasColors_ (Voxel.cpp:83-86)
  return O3S_OK;
}

int dm_upload_colors(o3s_dense_map* m, const double* colors, int64_t N) {
  hipStream_t s = m->stream;
  CK(m->in_c.ensure((size_t)N * 24, 0, s));
  CK(hipMemcpyAsync(m->in_c.p, colors, (size_t)N * 24, hipMemcpyHostToDevice, s));
  return O3S_OK;
}

int dm_upload(o3s_dense_map* m, const double* pts, const double* normals, int64_t N, const double* colors = nullptr) {
  hipStream_t s = m->stream;
  CK(m->in_p.ensure((size_t)N * 24, 0, s));
  CK(hipMemcpyAsync(m->in_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(m->in_n.ensure((size_t)N * 24, 0, s));
    CK(hipMemcpyAsync(m->in_n.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  return colors ? dm_upload_colors(m, colors, N) : O3S_OK;
}

// Submap::carve on the dense map, scan already on the device
int dm_carve_dev(o3s_dense_map* m, const o3s_dense_carving_params* p, const double* d_scan, int64_t N, const double sensor[3], int64_t* n_removed) {
  if (n_removed) *n_removed = 0;
  if (m->live == 0 || N == 0) return O3S_OK;  // "if (cloud->empty() ...) return" (Submap.cpp:148-150)
  if (N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  const double radius = p->neighborhood_radius_dense_map, step = 2.0 * radius;
  // the reference's march never ends for a zero step; refuse what would not terminate or not fit the offset table
  if (!(step > 0.0) || !std::isfinite(step) || !std::isfinite(p->max_raytracing_length) || !std::isfinite(p->truncation_distance) ||
      p->max_raytracing_length / step > 1.0e6)
    return O3S_ERR_BAD_ARGUMENT;
  DmOffsets off{};
  for (double d = -radius; d <= radius; d += m->voxel) {
    if (off.n == kDmMaxOff) return O3S_ERR_BAD_ARGUMENT;
    off.d[off.n++] = d;
  }
  hipStream_t s = m->stream;
  const size_t cap = (size_t)m->cap;
  int64_t nwords = 4096;  // about one word per four voxels: a few MB, L2 / Infinity-Cache resident
  while (nwords * 4 < m->live) nwords <<= 1;
  const size_t tb = dm_sort_temp_bytes(N);
  DmCarveArea w;
  CK(lay_out(m->arena, w, (size_t)N, tb, cap, (size_t)nwords));
  int rc = dm_sorted_keys(m, d_scan, N, w.sort, tb);
  if (rc != O3S_OK) return rc;
  CK(hipMemsetAsync(w.words, 0, (size_t)nwords * 16, s));
  hipLaunchKernelGGL(k_dm_build_filter, dim3(nblk(m->cap)), dim3(kB), 0, s, m->K(), m->cap, w.words, (uint64_t)(nwords - 1));
  hipLaunchKernelGGL(k_dm_heads, dim3(nblk(N)), dim3(kB), 0, s, w.sort.skeys, N, w.head);
  int64_t n_first = 0;
  rc = scan_flags(w.head, w.ord, N, w.sort.tmp, tb, &n_first, s);
  if (rc != O3S_OK) return rc;
  uint32_t ctr[16];
  rc = dm_read_counters(m, ctr);
  if (rc != O3S_OK) return rc;
  if (ctr[8]) return O3S_ERR_BAD_ARGUMENT;  // a NaN / out-of-range scan point has no voxel key
  if (n_first == 0) return O3S_OK;
  hipLaunchKernelGGL(k_dm_first, dim3(nblk(N)), dim3(kB), 0, s, w.sort.svals, w.head, w.ord, N, w.first);
  CK(hipMemsetAsync(w.rm, 0, cap, s));
  {
    // sqrt(v) <= radius is certain below r2lo and impossible above r2hi (sqrt is monotone and correctly rounded)
    const double r2 = radius * radius, r2lo = r2 * (1.0 - 1.0e-14), r2hi = r2 * (1.0 + 1.0e-14);
    const dim3 grid(nblk(n_first * kDmRayLanes)), block(kB);
#define O3S_DM_CARVE(NX)                                                                                                                     \
  hipLaunchKernelGGL(k_dm_carve_rays<NX>, grid, block, 0, s, d_scan, w.first, n_first, sensor[0], sensor[1], sensor[2], m->voxel, radius, r2lo, r2hi, \
                     step, p->max_raytracing_length, p->truncation_distance, off, m->K(), (uint64_t)(m->cap - 1),                            \
                     reinterpret_cast<const uint64_t*>(w.words), (uint64_t)(nwords - 1), w.rm)
    switch (off.n) {
      case 1: O3S_DM_CARVE(1); break;
      case 2: O3S_DM_CARVE(2); break;
      case 3: O3S_DM_CARVE(3); break;
      case 4: O3S_DM_CARVE(4); break;
      case 5: O3S_DM_CARVE(5); break;
      case 6: O3S_DM_CARVE(6); break;
      case 7: O3S_DM_CARVE(7); break;
      default: O3S_DM_CARVE(0); break;
    }
#undef O3S_DM_CARVE
#ifdef O3S_DM_STATS
    unsigned long long st[4];
    CK(hipStreamSynchronize(s));
    CK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_dm_stats), sizeof(st)));
    fprintf(stderr, "[dm stats, cumulative] rays %lld stops %llu in-radius %llu filter-hits %llu found %llu\n", (long long)n_first, st[0], st[1], st[2], st[3]);
#endif
  }
  CK(hipMemsetAsync(m->d_ctr.p, 0, 64, s));
  hipLaunchKernelGGL(k_dm_apply_remove, dim3(nblk(m->cap / 8)), dim3(kB), 0, s, w.rm, m->K(), m->cap, reinterpret_cast<uint32_t*>(m->d_ctr.p));
  CK(hipGetLastError());
  rc = dm_read_counters(m, ctr);
  if (rc != O3S_OK) return rc;
  int64_t removed = 0;
  for (int k = 0; k < 16; ++k) removed += ctr[k];
  m->live -= removed;
  m->tomb += removed;
  if (n_removed) *n_removed = removed;
  return O3S_OK;
}

int dm_set_dev(const o3s_dense_map* m) { return hipSetDevice(m->device) == hipSuccess ? O3S_OK : O3S_ERR_HIP; }

}  // namespace

extern "C" {

int o3s_dense_map_create(int device, double voxel_size, o3s_dense_map** out) {
  if (!out || !(voxel_size > 0.0) || !std::isfinite(voxel_size)) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  o3s_dense_map* m = new o3s_dense_map();
  m->device = device;
  m->voxel = voxel_size;
  m->inv = 1.0 / voxel_size;
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) {
    delete m;
    return O3S_ERR_HIP;
  }
  *out = m;
  return O3S_OK;
}

void o3s_dense_map_destroy(o3s_dense_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) {
    (void)hipStreamSynchronize(m->stream);
    (void)hipStreamDestroy(m->stream);
  }
  delete m;
}

int64_t o3s_dense_map_size(const o3s_dense_map* m) { return m ? m->live : 0; }
int o3s_dense_map_has_normals(const o3s_dense_map* m) { return m ? m->has_normals : 0; }
int o3s_dense_map_has_colors(const o3s_dense_map* m) { return m ? m->has_colors : 0; }
int64_t o3s_dense_map_capacity(const o3s_dense_map* m) { return m ? m->cap : 0; }

void o3s_dense_map_clear(o3s_dense_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->stream);
  m->keys.release();
  m->cnt.release();
  m->sum.release();
  m->csum.release();  // (has_colors stays, like has_normals: VoxelHashMap::clear empties voxels_ alone, VoxelHashMap.hpp:125)
  m->cap = m->live = m->tomb = 0;
}

int o3s_dense_map_insert_colored(o3s_dense_map* m, const double* pts, const double* normals, const double* colors, int64_t N) {
  if (!m || N < 0 || (N > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  int rc = dm_set_dev(m);
  if (rc != O3S_OK) return rc;
  rc = dm_upload(m, pts, normals, N, colors);
  if (rc != O3S_OK) return rc;
  return dm_insert_dev(m, m->in_p.as<double>(), normals ? m->in_n.as<double>() : nullptr, colors ? m->in_c.as<double>() : nullptr, N);
}

int o3s_dense_map_insert(o3s_dense_map* m, const double* pts, const double* normals, int64_t N) {
  return o3s_dense_map_insert_colored(m, pts, normals, nullptr, N);
}

int o3s_dense_map_carve(o3s_dense_map* m, const o3s_dense_carving_params* p, const double* scan_pts, int64_t N, const double sensor_position[3],
                        int64_t* n_removed) {
  if (n_removed) *n_removed = 0;
  if (!m || !p || !sensor_position || N < 0 || (N > 0 && !scan_pts)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0 || m->live == 0) return O3S_OK;
  int rc = dm_set_dev(m);
  if (rc != O3S_OK) return rc;
  rc = dm_upload(m, scan_pts, nullptr, N);
  if (rc != O3S_OK) return rc;
  return dm_carve_dev(m, p, m->in_p.as<double>(), N, sensor_position, n_removed);
}

}  // extern "C"

namespace {
// Submap::insertScanDenseMap (Submap.cpp:97-113) on a raw scan that is already in HBM
// d_raw_c: the scan's colours (nullable); rgb: the bounds of colorCropper_
int dm_insert_scan_dev(o3s_dense_map* m, const o3s_cropper* dense_map_cropper, const double* d_raw_p, const double* d_raw_n, const double* d_raw_c,
                       const DmRgb& rgb, int64_t N, const double T[16], const o3s_dense_carving_params* carving, int64_t* n_removed) {
  hipStream_t s = m->stream;
  const bool hn = d_raw_n != nullptr;
  int rc = O3S_OK;
  if (N > 0) {
    // denseMapCropper_->setPose(Identity); crop(rawScan) (Submap.cpp:99-100)
    o3s_cropper c = *dense_map_cropper;
    c.centre[0] = c.centre[1] = c.centre[2] = 0.0;
    CK(m->crop_p.ensure((size_t)N * 24, 0, s));
    CK(m->crop_n.ensure((size_t)N * 24, 0, s));
    int64_t kept = 0;
    if (!d_raw_c) {  // a cloud without colours passes colorCropper_.crop whole (croppers.cpp:209-214)
      rc = crop_dev(m->arena, c, d_raw_p, d_raw_n, N, m->crop_p.as<double>(), m->crop_n.as<double>(), &kept, s);
      if (rc != O3S_OK) return rc;
    } else {  // the volume crop and colorCropper_.crop (Submap.cpp:101) as one flag pass, one scan, one scatter
      CK(m->crop_c.ensure((size_t)N * 24, 0, s));
      const size_t tb = scan_temp_bytes(N);
      CropArea w;
      CK(lay_out(m->arena, w, (size_t)N, tb));
      hipLaunchKernelGGL(k_dm_color_mask, dim3(nblk(N)), dim3(kB), 0, s, c, 1, d_raw_p, d_raw_c, N, rgb, w.flag);
      rc = scan_flags(w.flag, w.off, N, w.tmp, tb, &kept, s);
      if (rc != O3S_OK) return rc;
      hipLaunchKernelGGL(k_dm_compact_col, dim3(nblk(N)), dim3(kB), 0, s, d_raw_p, d_raw_n, d_raw_c, N, w.flag, w.off, m->crop_p.as<double>(),
                         m->crop_n.as<double>(), m->crop_c.as<double>());
      CK(hipGetLastError());
    }
    if (kept > 0) {
      // o3d_slam::transform (helpers.cpp:283-318): a near-identity pose emits the cloud twice (copy + transformed)
      double dev = 0.0;
      for (int cc = 0; cc < 4; ++cc)
        for (int r = 0; r < 4; ++r) dev = std::max(dev, std::fabs(T[cc * 4 + r] - (r == cc ? 1.0 : 0.0)));
      const bool doubled = dev < 1e-4;
      const int64_t n_tf = doubled ? 2 * kept : kept;
      CK(m->tf_p.ensure((size_t)n_tf * 24, 0, s));
      CK(m->tf_n.ensure((size_t)n_tf * 24, 0, s));
      CK(m->d_T.ensure(128, 0, s));
      CK(hipMemcpyAsync(m->d_T.p, T, 128, hipMemcpyHostToDevice, s));
      double* dp = m->tf_p.as<double>();
      double* dn = m->tf_n.as<double>();
      if (doubled) {
        CK(hipMemcpyAsync(dp, m->crop_p.p, (size_t)kept * 24, hipMemcpyDeviceToDevice, s));
        if (hn) CK(hipMemcpyAsync(dn, m->crop_n.p, (size_t)kept * 24, hipMemcpyDeviceToDevice, s));
        dp += 3 * kept;
        dn += 3 * kept;
      }
      hipLaunchKernelGGL(k_transform_append, dim3(nblk(kept)), dim3(kB), 0, s, m->crop_p.as<double>(), hn ? m->crop_n.as<double>() : nullptr, kept, m->d_T.as<double>(), dp,
                         hn ? dn : nullptr);
      CK(hipGetLastError());
      // out->colors_ = cloud.colors_ (helpers.cpp:291): the colours ride along as they are — `kept` of them also beside the 2 * kept
      // points of the doubled cloud, which therefore no longer HasColors(): that scan adds no colour and does not set isHasColors_
      const double* d_col = (d_raw_c && !doubled) ? m->crop_c.as<double>() : nullptr;
      rc = dm_insert_dev(m, m->tf_p.as<double>(), hn ? m->tf_n.as<double>() : nullptr, d_col, n_tf);
      if (rc != O3S_OK) return rc;
    }
  }
  // carve(rawScan, mapToRangeSensor.translation(), carving_, &denseMap_) (Submap.cpp:108-110, 146-157)
  if (carving && N > 0 && m->live > 0 && (m->n_scans_inserted % carving->carve_space_every_n_scans) == 1) {
    const double sensor[3] = {T[12], T[13], T[14]};
    rc = dm_carve_dev(m, carving, d_raw_p, N, sensor, n_removed);
    if (rc != O3S_OK) return rc;
  }
  ++m->n_scans_inserted;
  return O3S_OK;
}

// ColorRangeCropper's bounds: rgbMin_ = 0, rgbMax_ = 1 unless given (croppers.hpp; nothing in the reference sets them)
DmRgb dm_rgb(const double rgb_min[3], const double rgb_max[3]) {
  DmRgb b;
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = rgb_min ? rgb_min[a] : 0.0;
    b.hi[a] = rgb_max ? rgb_max[a] : 1.0;
  }
  return b;
}
}  // namespace

extern "C" {

int o3s_dense_map_insert_scan_colored(o3s_dense_map* m, const o3s_cropper* dense_map_cropper, const double rgb_min[3], const double rgb_max[3],
                                      const double* raw_pts, const double* raw_normals, const double* raw_colors, int64_t N, const double T[16],
                                      const o3s_dense_carving_params* carving, int64_t* n_removed) {
  if (n_removed) *n_removed = 0;
  if (!m || !dense_map_cropper || !T || N < 0 || (N > 0 && !raw_pts)) return O3S_ERR_BAD_ARGUMENT;
  if (carving && carving->carve_space_every_n_scans <= 0) return O3S_ERR_BAD_ARGUMENT;  // the reference divides by it
  int rc = dm_set_dev(m);
  if (rc != O3S_OK) return rc;
  if (N > 0) {
    rc = dm_upload(m, raw_pts, raw_normals, N, raw_colors);
    if (rc != O3S_OK) return rc;
  }
  return dm_insert_scan_dev(m, dense_map_cropper, m->in_p.as<double>(), raw_normals ? m->in_n.as<double>() : nullptr,
                            raw_colors ? m->in_c.as<double>() : nullptr, dm_rgb(rgb_min, rgb_max), N, T, carving, n_removed);
}

int o3s_dense_map_insert_scan(o3s_dense_map* m, const o3s_cropper* dense_map_cropper, const double* raw_pts, const double* raw_normals, int64_t N,
                              const double T[16], const o3s_dense_carving_params* carving, int64_t* n_removed) {
  return o3s_dense_map_insert_scan_colored(m, dense_map_cropper, nullptr, nullptr, raw_pts, raw_normals, nullptr, N, T, carving, n_removed);
}

int o3s_dense_map_insert_resident_scan_colored(o3s_dense_map* m, const o3s_cropper* dense_map_cropper, const double rgb_min[3],
                                               const double rgb_max[3], const o3s_scan* sc, const double* raw_colors, int64_t n_colors,
                                               const double T[16], const o3s_dense_carving_params* carving, int64_t* n_removed) {
  if (n_removed) *n_removed = 0;
  if (!m || !dense_map_cropper || !sc || !T || (raw_colors && n_colors < 0)) return O3S_ERR_BAD_ARGUMENT;
  if (carving && carving->carve_space_every_n_scans <= 0) return O3S_ERR_BAD_ARGUMENT;
  if (sc->device != m->device) return O3S_ERR_BAD_ARGUMENT;
  if (raw_colors && n_colors != sc->n_raw) return O3S_ERR_BAD_SHAPE;  // one colour per raw point
  int rc = dm_set_dev(m);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(sc->stream));  // the scan's own work is complete (its calls end synchronised); this map's stream takes over
  const bool hc = raw_colors && sc->n_raw > 0;
  if (hc) {
    rc = dm_upload_colors(m, raw_colors, sc->n_raw);
    if (rc != O3S_OK) return rc;
  }
  return dm_insert_scan_dev(m, dense_map_cropper, sc->raw_p.as<double>(), sc->raw_has_normals ? sc->raw_n.as<double>() : nullptr,
                            hc ? m->in_c.as<double>() : nullptr, dm_rgb(rgb_min, rgb_max), sc->n_raw, T, carving, n_removed);
}

int o3s_dense_map_insert_resident_scan(o3s_dense_map* m, const o3s_cropper* dense_map_cropper, const o3s_scan* sc, const double T[16],
                                       const o3s_dense_carving_params* carving, int64_t* n_removed) {
  return o3s_dense_map_insert_resident_scan_colored(m, dense_map_cropper, nullptr, nullptr, sc, nullptr, 0, T, carving, n_removed);
}

int o3s_dense_map_to_point_cloud_colored(const o3s_dense_map* m, double* pts, double* normals, double* colors, int32_t* keys, int32_t* counts,
                                         int64_t* n_out) {
  if (n_out) *n_out = 0;
  if (!m) return O3S_ERR_BAD_ARGUMENT;
  if (colors && !m->has_colors) return O3S_ERR_BAD_SHAPE;  // as o3s_submap_download_colors refuses a map without colours
  if (m->live == 0) return O3S_OK;
  if (colors && !m->csum.p) return O3S_ERR_HIP;  // cannot happen: has_colors is set by, and a live voxel after it made by, an insert that holds them
  if (!pts) return O3S_ERR_BAD_ARGUMENT;
  int rc = dm_set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const size_t cap = (size_t)m->cap, v = (size_t)m->live;
  const size_t tb = std::max(scan_temp_bytes(m->cap), sort_temp_bytes(m->live));
  DmExportArea w;
  CK(lay_out(m->arena, w, cap, v, tb, colors != nullptr));
  hipLaunchKernelGGL(k_dm_live, dim3(nblk(m->cap)), dim3(kB), 0, s, m->K(), m->C(), m->cap, w.flag);
  int64_t V = 0;
  rc = scan_flags(w.flag, w.off, m->cap, w.tmp, tb, &V, s);
  if (rc != O3S_OK) return rc;
  if (V > m->live) return O3S_ERR_HIP;  // cannot happen: the host count tracks every claim and removal
  if (V == 0) return O3S_OK;
  hipLaunchKernelGGL(k_dm_collect, dim3(nblk(m->cap)), dim3(kB), 0, s, m->K(), w.flag, w.off, m->cap, w.k1, w.s1);
  size_t stb = tb;
  CK(rocprim::radix_sort_pairs(w.tmp, stb, w.k1, w.k2, w.s1, w.s2, (size_t)V, 0, 64, s));
  hipLaunchKernelGGL(k_dm_emit, dim3(nblk(V)), dim3(kB), 0, s, w.k2, w.s2, V, m->C(), m->S(), colors ? m->CS() : (const double*)nullptr, w.op, w.on, w.ocol, w.ok,
                     w.oc);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(pts, w.op, (size_t)V * 24, hipMemcpyDeviceToHost, s));
  if (normals) CK(hipMemcpyAsync(normals, w.on, (size_t)V * 24, hipMemcpyDeviceToHost, s));
  if (colors) CK(hipMemcpyAsync(colors, w.ocol, (size_t)V * 24, hipMemcpyDeviceToHost, s));
  if (keys) CK(hipMemcpyAsync(keys, w.ok, (size_t)V * 12, hipMemcpyDeviceToHost, s));
  if (counts) CK(hipMemcpyAsync(counts, w.oc, (size_t)V * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (n_out) *n_out = V;
  return O3S_OK;
}

int o3s_dense_map_to_point_cloud(const o3s_dense_map* m, double* pts, double* normals, int32_t* keys, int32_t* counts, int64_t* n_out) {
  return o3s_dense_map_to_point_cloud_colored(m, pts, normals, nullptr, keys, counts, n_out);
}

// ColorRangeCropper::crop (croppers.cpp:205-239) on host buffers
int o3s_color_range_crop(int device, const double rgb_min[3], const double rgb_max[3], const double* pts, const double* normals, const double* colors,
                         const double* covariances, int64_t N, double* out_pts, double* out_normals, double* out_colors, double* out_covariances,
                         int64_t* n_out) {
  if (!pts || !out_pts || !n_out || N < 0 || (normals && !out_normals) || (colors && !out_colors) || (covariances && !out_covariances))
    return O3S_ERR_BAD_ARGUMENT;
  *n_out = 0;
  if (N == 0) return O3S_OK;
  if (N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  if (!colors) {  // "*cropped = cloud" (croppers.cpp:211-214): nothing to decide, nothing for the device to do
    std::memcpy(out_pts, pts, (size_t)N * 24);
    if (normals) std::memcpy(out_normals, normals, (size_t)N * 24);
    if (covariances) std::memcpy(out_covariances, covariances, (size_t)N * 72);
    *n_out = N;
    return O3S_OK;
  }
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_pts, d_nrm, d_col, d_cov, d_opts, d_on, d_ocol, d_ocov;
  Arena ar;
  CK(d_pts.alloc((size_t)N * 24));
  CK(d_col.alloc((size_t)N * 24));
  CK(d_opts.alloc((size_t)N * 24));
  CK(d_ocol.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d_pts.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(d_col.p, colors, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(d_nrm.alloc((size_t)N * 24));
    CK(d_on.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(d_nrm.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  if (covariances) {
    CK(d_cov.alloc((size_t)N * 72));
    CK(d_ocov.alloc((size_t)N * 72));
    CK(hipMemcpyAsync(d_cov.p, covariances, (size_t)N * 72, hipMemcpyHostToDevice, s));
  }
  const size_t tb = scan_temp_bytes(N);
  CropArea w;
  CK(lay_out(ar, w, (size_t)N, tb));
  hipLaunchKernelGGL(k_dm_color_mask, dim3(nblk(N)), dim3(kB), 0, s, o3s_cropper{}, 0, d_pts.as<double>(), d_col.as<double>(), N,
                     dm_rgb(rgb_min, rgb_max), w.flag);
  int64_t kept = 0;
  rc = scan_flags(w.flag, w.off, N, w.tmp, tb, &kept, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_dm_compact_col, dim3(nblk(N)), dim3(kB), 0, s, d_pts.as<double>(), normals ? d_nrm.as<double>() : nullptr, d_col.as<double>(), N,
                     w.flag, w.off, d_opts.as<double>(), d_on.as<double>(), d_ocol.as<double>());
  if (covariances)
    hipLaunchKernelGGL(k_compact_attr, dim3(nblk(N)), dim3(kB), 0, s, (const double*)nullptr, d_cov.as<double>(), N, w.flag, w.off, (double*)nullptr,
                       d_ocov.as<double>());
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s));
  CK(hipMemcpy(out_pts, d_opts.p, (size_t)kept * 24, hipMemcpyDeviceToHost));
  if (normals) CK(hipMemcpy(out_normals, d_on.p, (size_t)kept * 24, hipMemcpyDeviceToHost));
  CK(hipMemcpy(out_colors, d_ocol.p, (size_t)kept * 24, hipMemcpyDeviceToHost));
  if (covariances) CK(hipMemcpy(out_covariances, d_ocov.p, (size_t)kept * 72, hipMemcpyDeviceToHost));
  *n_out = kept;
  return O3S_OK;
}

int o3s_dense_map_transform(o3s_dense_map* m, const double T[16]) {
  if (!m || !T) return O3S_ERR_BAD_ARGUMENT;
  if (m->live == 0) return O3S_OK;  // "if (empty()) return" (Voxel.cpp:51-53)
  const int rc = dm_set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  CK(m->d_T.ensure(128, 0, s));
  CK(hipMemcpyAsync(m->d_T.p, T, 128, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_dm_transform, dim3(nblk(m->cap)), dim3(kB), 0, s, m->K(), m->C(), m->S(), m->cap, m->d_T.as<double>());
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s));
  return O3S_OK;
}

}  // extern "C"
