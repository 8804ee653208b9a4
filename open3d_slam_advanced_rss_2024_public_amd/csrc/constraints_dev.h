// constraints_dev.h — kernels of o3s_submaps_odometry_constraints (include/constraints/o3s_constraints.h): the overlap selection and
// Open3D's information matrix for MANY pairs of resident submaps in one sequence of launches; gfx950 only.  Included from
// constraints_impl.h at the end of cloud_ops.hip (one TU: the key and the OvSlot table of voxel_table.h, wave_sum of wave_ops.h,
// o3d_transform_point and the sort of cloud_dev.h; nothing of overlap_impl.h).
//
// Every launch covers all pairs.  A pair table on the device (OcPair) says which blocks belong to which pair: a block never straddles
// two clouds, so the wave-wide step of the selection and the per-block partial sums see one pair only, and a pair's
// partials are the same whatever else is in the call.
//
//  k_oc_count   voxel key of every point (the source placed by T_k) and the per-voxel counts, in the pair's own slice of one table
//  k_oc_flag    the selection flags and their count per block; every selected TARGET point gets the bucket of its search cell as sort key
//  (rocPRIM)    one stable sort of all target points by bucket (not selected: behind the last bucket)
//  k_oc_heads   the range of every bucket in the sorted order, and the sorted records (x, y, z, pair | index)
//  k_oc_search  per selected source point the nearest selected target point of its pair among the buckets of the cells around it,
//               the 21 + 1 sums of its rows of G^T G, block partials
//  k_oc_fold    per pair and component: the block partials in block order; the two selection sizes from the blocks' counts
//  k_oc_post    everything the host reads, into its pinned block, then one sequence number (host_post.h)
//
// The search structure is a cell grid of edge max_dist that is never laid out: a cell is hashed together with its pair into one of B
// buckets, and a bucket may hold points of several cells and pairs.  That costs nothing in correctness — a candidate counts only when
// it belongs to the pair and lies within the radius, and a point seen twice changes no minimum — and spares the grid its bounds (a
// reduction and a wait of its own) and its memory (the cells of a 60 m submap at 0.2 m).  Cells are numbered by floor(x / max_dist)
// in 64 bits; the cells probed for a point are those of [x - r', x + r'] per axis with r' a hair above max_dist, so a neighbour whose
// quotient rounds across a cell border is still met (three cells per axis, four when the interval straddles one more border).
#pragma once
#include "cloud_dev.h"
#include "voxel_table.h"

namespace {
namespace o3s_cloud {

constexpr int kOcComps = 22;  // [0..20] the upper triangle of G^T G, [21] the number of correspondences
constexpr int kOcRes = 24;    // 8-byte words per pair in the host block: the sums, then (n_source | n_target << 32), then the error word

struct OcPair {
  const double* sp;
  const double* tp;
  double T[16];
  int64_t ns, nt;
  uint32_t blk_s, blk_t;  // first block of the source / of the target in the launches over all points (blk_t = blk_s + nblk(ns))
  uint32_t sblk;          // first block of the source in the search launch: where its partials start
  uint32_t g_s, g_t;      // where the source's / the target's flags and slots start
  uint32_t t_base;        // where the target starts among all targets (the sort's index space)
  uint32_t tab_off, tab_mask;  // the pair's slice of the voxel table
  int32_t has_T;          // T is given: the selection places the source by it (o3s_overlap_indices multiplies by an identity too)
  int32_t apply_search;   // ... and so does the search, unless T is an identity (PointCloud::Transform is skipped for one)
};

// the pair whose range [first(k), first(k + 1)) holds v; first is ascending, first(0) <= v
template <uint32_t OcPair::*kFirst>
__device__ __forceinline__ int oc_find(const OcPair* __restrict__ pairs, int m, uint32_t v) {
  int lo = 0, hi = m - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid].*kFirst <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// cell number along one axis; clamped where a 64-bit integer ends (coordinates are bounded by the selection's voxel range and
// max_dist >= voxel 2^-20, so the clamp is never reached: it keeps the conversion defined)
__device__ __forceinline__ long long oc_cell(double x, double h) {
  const double big = 4611686018427387904.0;  // 2^62
  return (long long)fmin(fmax(floor(x / h), -big), big);
}
// the bounds of the cells that can hold a point within max_dist of x: r' = max_dist (1 + 2^-20) + |x| 2^-50 covers the rounding of
// the difference the distance is formed from, of x -+ r' and of the quotients (floor and a correctly rounded division are monotone)
__device__ __forceinline__ void oc_cell_range(double x, double h, long long* lo, long long* hi) {
  const double r = h * (1.0 + 0x1p-20) + fabs(x) * 0x1p-50;
  *lo = oc_cell(x - r, h);
  *hi = oc_cell(x + r, h);
}

// err[k] = 1: pair k has a coordinate that is not finite or a voxel index beyond +-2^20; err[m] = 1: a pair's table slice is full.
// The counts are those of k_ov_count.  The lanes that share the voxel of the wave's first lane are served by that lane with one
// compare-and-swap and one add (a map in voxel order: whole waves fall into one voxel); every other lane then counts itself, all of
// them at once — serving one distinct voxel after the other, as k_ov_count does, is up to 64 dependent round trips per wave on a
// map in any other order (the lesson of k_vm_insert).  Integer adds only: the counts do not depend on the order.
__global__ void __launch_bounds__(kB) k_oc_count(const OcPair* __restrict__ pairs, int m, double inv, OvSlot* __restrict__ tab, uint32_t* __restrict__ slot_of,
                                                 uint32_t* __restrict__ err) {
  const int k = oc_find<&OcPair::blk_s>(pairs, m, blockIdx.x);
  const OcPair& P = pairs[k];
  const int layer = blockIdx.x >= P.blk_t ? 1 : 0;
  const int64_t N = layer ? P.nt : P.ns;
  const int64_t i = (int64_t)(blockIdx.x - (layer ? P.blk_t : P.blk_s)) * kB + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  uint64_t key = kDmEmpty;
  if (i < N) {
    const double* __restrict__ pts = layer ? P.tp : P.sp;
    double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!layer && P.has_T) o3d_transform_point(P.T, x, y, z);
    key = vm_key(x, y, z, inv);
    if (key == kDmEmpty) err[k] = 1u;
  }
  OvSlot* __restrict__ slice = tab + P.tab_off;
  bool pending = key != kDmEmpty;
  uint32_t my_slot = 0xffffffffu;
  const unsigned long long open = __ballot(pending);
  if (open) {  // (uniform)
    const int leader = __ffsll((long long)open) - 1;
    const uint64_t lk = wave_bcast_u64(key, leader);
    const bool same = pending && key == lk;
    const unsigned long long grp = __ballot(same);
    uint32_t h = 0xffffffffu;
    if (lane == leader) h = ov_count_key(lk, slice, P.tab_mask, layer, (uint32_t)__popcll(grp), err + m);
    h = (uint32_t)__shfl((int)h, leader);
    if (same) my_slot = h;
    else if (pending) my_slot = ov_count_key(key, slice, P.tab_mask, layer, 1u, err + m);
  }
  if (i < N) slot_of[(size_t)(layer ? P.g_t : P.g_s) + (size_t)i] = my_slot;
}

// flag[g] as k_ov_flag makes it; blk_cnt[block] = the flags the block set (no atomic: 130 k waves adding to a dozen words serialise).
// A target point also gets its sort key: the bucket of (pair, search cell) when it is selected, n_buckets when it is not.
__global__ void __launch_bounds__(kB) k_oc_flag(const OcPair* __restrict__ pairs, int m, const OvSlot* __restrict__ tab, const uint32_t* __restrict__ slot_of,
                                                int64_t min_pts, double cell, uint32_t n_buckets, uint32_t* __restrict__ flag, uint32_t* __restrict__ blk_cnt,
                                                uint64_t* __restrict__ bkey, uint32_t* __restrict__ bval) {
  __shared__ uint32_t shc[kB / 64];
  const int k = oc_find<&OcPair::blk_s>(pairs, m, blockIdx.x);
  const OcPair& P = pairs[k];
  const int layer = blockIdx.x >= P.blk_t ? 1 : 0;
  const int64_t N = layer ? P.nt : P.ns;
  const int64_t i = (int64_t)(blockIdx.x - (layer ? P.blk_t : P.blk_s)) * kB + threadIdx.x;
  bool in = false;
  if (i < N) {
    const size_t g = (size_t)(layer ? P.g_t : P.g_s) + (size_t)i;
    const uint32_t h = slot_of[g];
    if (h != 0xffffffffu) {
      const OvSlot sl = tab[(size_t)P.tab_off + h];
      in = (int64_t)sl.n[1 - layer] >= min_pts && (min_pts <= 1 || (int64_t)sl.n[layer] >= min_pts);
    }
    flag[g] = in ? 1u : 0u;
    if (layer) {
      uint64_t b = n_buckets;
      if (in) {
        const double* __restrict__ tp = P.tp;
        const long long cx = oc_cell(tp[3 * i], cell), cy = oc_cell(tp[3 * i + 1], cell), cz = oc_cell(tp[3 * i + 2], cell);
        b = splitmix64((uint64_t)cx + splitmix64((uint64_t)cy + splitmix64((uint64_t)cz + (uint64_t)k))) & (uint64_t)(n_buckets - 1u);
      }
      bkey[(size_t)P.t_base + (size_t)i] = b;
      bval[(size_t)P.t_base + (size_t)i] = P.t_base + (uint32_t)i;
    }
  }
  const unsigned long long b = __ballot(in);
  if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (shc[0] + shc[1]) + (shc[2] + shc[3]);
}

struct __attribute__((aligned(16))) OcRec {  // a selected target point in sorted order
  double x, y, z;
  uint32_t idx, pair;  // its index in its own cloud, its pair
};
// ks / vs: the sorted keys and values.  range[b] = [first, last + 1) of bucket b in the sorted order (zeroed before: empty)
__global__ void __launch_bounds__(kB) k_oc_heads(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ vs, int64_t Mt, uint32_t n_buckets,
                                                 const OcPair* __restrict__ pairs, int m, uint2* __restrict__ range, OcRec* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= Mt) return;
  const uint64_t b = ks[i];
  if (b >= (uint64_t)n_buckets) return;
  const uint32_t v = vs[i];
  const int k = oc_find<&OcPair::t_base>(pairs, m, v);
  const uint32_t j = v - pairs[k].t_base;
  const double* __restrict__ tp = pairs[k].tp;
  OcRec r;
  r.x = tp[3 * (size_t)j];
  r.y = tp[3 * (size_t)j + 1];
  r.z = tp[3 * (size_t)j + 2];
  r.idx = j;
  r.pair = (uint32_t)k;
  rec[i] = r;
  if (i == 0 || ks[i - 1] != b) range[b].x = (uint32_t)i;
  if (i + 1 == Mt || ks[i + 1] != b) range[b].y = (uint32_t)(i + 1);
}

// One lane per source point.  part[c * n_blocks + block]: the block's sum of component c — every lane holds one point's terms (or
// zeros), the wave's fixed tree, then the four waves in order: the same bits wherever the pair stands in the call.
__global__ void __launch_bounds__(kB) k_oc_search(const OcPair* __restrict__ pairs, int m, const uint32_t* __restrict__ flag, const uint2* __restrict__ range,
                                                  const OcRec* __restrict__ rec, uint32_t bucket_mask, double cell, double r2, double* __restrict__ part) {
  __shared__ double sh[kB / 64][kOcComps];
  const int k = oc_find<&OcPair::sblk>(pairs, m, blockIdx.x);
  const OcPair& P = pairs[k];
  const int64_t i = (int64_t)(blockIdx.x - P.sblk) * kB + threadIdx.x;
  double acc[kOcComps];
#pragma unroll
  for (int c = 0; c < kOcComps; ++c) acc[c] = 0.0;
  if (i < P.ns && flag[(size_t)P.g_s + (size_t)i]) {
    double qx = P.sp[3 * i], qy = P.sp[3 * i + 1], qz = P.sp[3 * i + 2];
    if (P.apply_search) o3d_transform_point(P.T, qx, qy, qz);
    long long x0, x1, y0, y1, z0, z1;
    oc_cell_range(qx, cell, &x0, &x1);
    oc_cell_range(qy, cell, &y0, &y1);
    oc_cell_range(qz, cell, &z0, &z1);
    double best = __builtin_huge_val(), tx = 0.0, ty = 0.0, tz = 0.0;
    uint32_t bj = 0xffffffffu;
    for (long long cz = z0; cz <= z1; ++cz) {
      const uint64_t hz = splitmix64((uint64_t)cz + (uint64_t)k);
      for (long long cy = y0; cy <= y1; ++cy) {
        const uint64_t hy = splitmix64((uint64_t)cy + hz);
        for (long long cx = x0; cx <= x1; ++cx) {
          const uint2 rg = range[(uint32_t)splitmix64((uint64_t)cx + hy) & bucket_mask];
          for (uint32_t a = rg.x; a < rg.y; ++a) {
            const OcRec c = rec[a];
            if (c.pair != (uint32_t)k) continue;
            const double ddx = qx - c.x, ddy = qy - c.y, ddz = qz - c.z;  // the squared distance as the registration's search forms it
            double d = ddx * ddx;
            d = d + ddy * ddy;
            d = d + ddz * ddz;
            if (d < best || (d == best && c.idx < bj)) {
              best = d;
              bj = c.idx;
              tx = c.x;
              ty = c.y;
              tz = c.z;
            }
          }
        }
      }
    }
    if (best < r2) {  // GetInformationMatrixFromPointClouds: three rows per correspondence, built from the TARGET point
      const double rows[3][6] = {{0.0, tz, -ty, 1.0, 0.0, 0.0}, {-tz, 0.0, tx, 0.0, 1.0, 0.0}, {ty, -tx, 0.0, 0.0, 0.0, 1.0}};
      int t = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
          double s = rows[0][a] * rows[0][b];
          s = s + rows[1][a] * rows[1][b];
          s = s + rows[2][a] * rows[2][b];
          acc[t++] = s;
        }
      acc[21] = 1.0;
    }
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < kOcComps; ++c) {
    const double v = wave_sum(acc[c]);
    if (l == 0) sh[w][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < kOcComps)
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// block (k, c), c < kOcComps: lane l adds the partials l, l + 64, ... of pair k's blocks in that order, then the wave's fixed tree;
// c = kOcComps + layer: the selection size of the layer, the sum of its blocks' counts
constexpr int kOcFolds = kOcComps + 2;
__global__ void __launch_bounds__(64) k_oc_fold(const OcPair* __restrict__ pairs, const double* __restrict__ part, uint32_t n_blocks,
                                                const uint32_t* __restrict__ blk_cnt, double* __restrict__ sums, uint32_t* __restrict__ cnt) {
  const int k = blockIdx.x / kOcFolds, c = blockIdx.x % kOcFolds, l = threadIdx.x;
  const OcPair& P = pairs[k];
  if (c >= kOcComps) {
    const int layer = c - kOcComps;
    const uint32_t* p = blk_cnt + (layer ? P.blk_t : P.blk_s);
    const int nb = (int)(((layer ? P.nt : P.ns) + kB - 1) / kB);
    uint32_t s = 0;
    for (int b = l; b < nb; b += 64) s += p[b];
    s = wave_sum_u32(s);
    if (l == 0) cnt[2 * k + layer] = s;
    return;
  }
  const double* p = part + (size_t)c * n_blocks + P.sblk;
  const int nb = (int)((P.ns + kB - 1) / kB);
  double s = 0;
  for (int b = l; b < nb; b += 64) s += p[b];
  s = wave_sum(s);
  if (l == 0) sums[(size_t)k * kOcComps + c] = s;
}

// The hand-over: pair k's sums, counts and error word into the host's block `res` (kOcRes words a pair), the table-full word into
// the mailbox, then the sequence number.  One wave.  (mailbox NULL: posts are off, the host synchronises the stream instead.)
__global__ void __launch_bounds__(64) k_oc_post(int m, const double* __restrict__ sums, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ err,
                                                unsigned long long* __restrict__ res, uint32_t* __restrict__ mailbox, uint32_t seq) {
  if (blockIdx.x != 0) return;
  uint32_t* r32 = reinterpret_cast<uint32_t*>(res);
  for (int w = threadIdx.x; w < m * kOcRes; w += 64) {
    const int k = w / kOcRes, c = w % kOcRes;
    unsigned long long v;
    if (c < kOcComps) v = __builtin_bit_cast(unsigned long long, sums[(size_t)k * kOcComps + c]);
    else if (c == kOcComps) v = (unsigned long long)cnt[2 * k] | ((unsigned long long)cnt[2 * k + 1] << 32);
    else v = (unsigned long long)err[k] | ((unsigned long long)err[m] << 32);
    post_store1(r32, 2 * w, v);
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0 && mailbox) {
    const uint32_t v[1] = {err[m]};
    post(mailbox, seq, kPostVals, v);
  }
}

}  // namespace o3s_cloud
}  // namespace
