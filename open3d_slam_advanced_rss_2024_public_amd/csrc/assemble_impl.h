// assemble_impl.h — the assembled map (C ABI: include/assembled_map/o3s_assembled_map.h): the map clouds of K resident submaps read
// as one cloud, gfx950 only.  Included at the end of cloud_ops.hip behind submap_impl.h (it reads o3s_submap's arrays) so that it
// shares the one instantiation of the rocPRIM sort / scan and of k_heads / the flag scan in cloud_dev.h.
//
// The K arrays are addressed through a segment table on the device: per non-empty submap its point / normal / colour arrays and the
// ordinal of its first point in the concatenation (start[K] = the total).  The global ordinal g in [0, total) is what the voxel sort
// carries as its value; a lane finds the segment of an ordinal by binary search over the <= K + 1 starts, which a block keeps in LDS.
//
//   voxel_size <= 0   k_asm_concat                                                      1 launch
//   voxel_size  > 0   k_bounds<AsmPoints> -> k_bounds_post (cloud_bounds: the one         2 + 1 + sort + 1 + scan + 1 launches
//                     read-back before the keys: exact min / max bound, from which the
//                     host derives the anchor AND the index extents) ->
//                     k_grid_keys<AsmPoints> -> sort_pairs (stable) -> k_heads ->
//                     flag scan -> k_asm_reduce
// The bound and key kernels are the flat clouds' own (cloud_bounds.h, normals_dev.h) over the segmented point source below.
// The existing voxelisers (voxel_pipeline_dev, k_vox_reduce*) are untouched; k_asm_reduce restates their mode-1 arithmetic over
// segments: sums in ascending ordinal = input order of the concatenation, mean = sum / count, normals not renormalised.
#pragma once
#include "../../include/assembled_map/o3s_assembled_map.h"

#include "submap_impl.h"

namespace {

constexpr int kAsmLds = 1024;  // segment starts a block keeps in LDS (8 KB); a table with more is searched in global memory

struct AsmTable {  // device addresses, all inside one buffer; a kernel argument
  const int64_t* start = nullptr;        // [K + 1], strictly increasing (empty submaps are not listed), start[K] = total
  const double* const* pts = nullptr;    // [K]
  const double* const* nrm = nullptr;    // [K]; read only when the result carries normals
  const double* const* col = nullptr;    // [K]; read only when the result carries colours
  int K = 0;
};

// the starts as this block reads them: LDS when they fit.  Reached by every thread of the block, before any of them returns.
__device__ __forceinline__ const int64_t* asm_starts(const AsmTable& t, int64_t* sh) {
  if (t.K + 1 > kAsmLds) return t.start;  // (uniform)
  for (int k = threadIdx.x; k <= t.K; k += kB) sh[k] = t.start[k];
  __syncthreads();
  return sh;
}
// the segment of ordinal g: the largest s with start[s] <= g (0 <= g < start[K])
__device__ __forceinline__ int asm_find(const int64_t* st, int K, int64_t g) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (st[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// The concatenation as a point source (cloud_bounds.h): point g of [0, total).  open() is asm_starts — the block-wide LDS prologue
// that every thread reaches before any returns.
struct AsmPoints {
  AsmTable t;
  struct Opened {
    const int64_t* st;
    const double* const* pts;
    int K;
    __device__ __forceinline__ const double* at(int64_t g) const {
      const int s = asm_find(st, K, g);
      return pts[s] + 3 * (g - st[s]);
    }
  };
  __device__ __forceinline__ Opened open() const {
    __shared__ int64_t sh[kAsmLds];
    return {asm_starts(t, sh), t.pts, t.K};
  }
};

// Mapper::getAssembledMapPointCloud (Mapper.cpp:524-535): one lane per DOUBLE of the output, so that a wave reads and writes 512
// contiguous bytes wherever a segment does not end inside it.  out_n / out_c nullable.
__global__ void __launch_bounds__(kB) k_asm_concat(AsmTable t, int64_t total, double* __restrict__ out_p, double* __restrict__ out_n,
                                                   double* __restrict__ out_c) {
  __shared__ int64_t sh[kAsmLds];
  const int64_t* st = asm_starts(t, sh);
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= 3 * total) return;
  const int s = asm_find(st, t.K, i / 3);
  const int64_t r = i - 3 * st[s];
  out_p[i] = t.pts[s][r];
  if (out_n) out_n[i] = t.nrm[s][r];
  if (out_c) out_c[i] = t.col[s][r];
}

// One lane per voxel, the run structure of k_vox_reduce: the voxel's members follow its head in ascending ordinal (stable sort), which
// is the order of the sequential accumulation over the concatenated cloud (Open3D VoxelDownSample: AccumulatedPoint::AddPoint), so
// the fp64 means are bit-identical to it.  Ordinals ascend inside a run, so the segment index only ever moves forward.
__global__ void __launch_bounds__(kB) k_asm_reduce(AsmTable t, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   const uint32_t* __restrict__ head, const uint32_t* __restrict__ ord, int64_t N,
                                                   double* __restrict__ out_p, double* __restrict__ out_n, double* __restrict__ out_c) {
  __shared__ int64_t sh[kAsmLds];
  const int64_t* st = asm_starts(t, sh);
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N || !head[i]) return;
  const uint64_t k = keys[i];
  double sp[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, sc[3] = {0, 0, 0};
  int cnt = 0;
  int s = asm_find(st, t.K, (int64_t)vals[i]);
  for (int64_t j = i; j < N && keys[j] == k; ++j) {
    const int64_t g = (int64_t)vals[j];
    while (g >= st[s + 1]) ++s;  // (st[K] = total > g)
    const int64_t r = 3 * (g - st[s]);
    const double* p = t.pts[s] + r;
    sp[0] += p[0];
    sp[1] += p[1];
    sp[2] += p[2];
    if (out_n) {
      const double* q = t.nrm[s] + r;
      sn[0] += q[0];
      sn[1] += q[1];
      sn[2] += q[2];
    }
    if (out_c) {
      const double* q = t.col[s] + r;
      sc[0] += q[0];
      sc[1] += q[1];
      sc[2] += q[2];
    }
    ++cnt;
  }
  const int64_t o = (int64_t)ord[i];
  const double dn = (double)cnt;
  for (int a = 0; a < 3; ++a) {
    out_p[3 * o + a] = sp[a] / dn;
    if (out_n) out_n[3 * o + a] = sn[a] / dn;
    if (out_c) out_c[3 * o + a] = sc[a] / dn;
  }
}

// work area of the voxelising build over n points in all
struct AssembleArea {
  static constexpr size_t kSlack = 4096;
  unsigned long long* d_bb;  // bounds block
  uint64_t *keys, *keys2;
  uint32_t *vals, *vals2, *head, *ord;
  char* tmp;  // also k_heads' per-block counts `blk` (room: scan_temp_bytes), consumed by the scan right behind
  template <class A>
  void lay(A& a, size_t n, size_t tb_scan, size_t tb_sort) {
    take(a, d_bb, kBoundsWords);
    take(a, keys, n);
    take(a, keys2, n);
    take(a, vals, n);
    take(a, vals2, n);
    take(a, head, n);
    take(a, ord, n + 1);
    take(a, tmp, std::max(tb_scan, tb_sort));
  }
};

}  // namespace

struct o3s_assembled_map {
  int device = 0;
  DevMem pts, nrm, col;  // the result
  int64_t n = 0;
  int has_normals = 0, has_colors = 0;
  Arena arena;         // work area of the voxelising build
  DevMem table;          // the segment table
};

extern "C" {

int o3s_assembled_map_create(int device, o3s_assembled_map** out) {
  if (!out) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  o3s_assembled_map* a = new o3s_assembled_map();
  a->device = device;
  *out = a;
  return O3S_OK;
}

void o3s_assembled_map_destroy(o3s_assembled_map* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);  // (every build has returned complete: nothing is in flight on the arrays)
  delete a;
}

int64_t o3s_assembled_map_size(const o3s_assembled_map* a) { return a ? a->n : 0; }
int o3s_assembled_map_has_normals(const o3s_assembled_map* a) { return a && a->n > 0 && a->has_normals ? 1 : 0; }
int o3s_assembled_map_has_colors(const o3s_assembled_map* a) { return a && a->n > 0 && a->has_colors ? 1 : 0; }
int64_t o3s_assembled_map_device_bytes(const o3s_assembled_map* a) {
  return a ? (int64_t)(a->pts.cap + a->nrm.cap + a->col.cap + a->arena.mem.cap + a->table.cap) : 0;
}

int o3s_assembled_map_build(o3s_assembled_map* a, int32_t n, o3s_submap* const* maps, double voxel_size, int32_t attrs, int64_t* n_out) {
  // everything is checked before the first launch: a bad argument leaves the previous result
  if (!a || n < 0 || (n > 0 && !maps)) return O3S_ERR_BAD_ARGUMENT;
  for (int32_t i = 0; i < n; ++i) {
    if (!maps[i] || maps[i]->device != a->device) return O3S_ERR_BAD_ARGUMENT;
    for (int32_t j = 0; j < i; ++j)
      if (maps[j] == maps[i]) return O3S_ERR_BAD_ARGUMENT;
  }
  for (int32_t i = 0; i < n; ++i)
    if (const int rs_ = submap_settle(maps[i]); rs_ != O3S_OK) return rs_;  // pending inserts are completed first
  int64_t total = 0;
  int K = 0;
  bool hn = (attrs & O3S_ASSEMBLE_NORMALS) != 0, hc = (attrs & O3S_ASSEMBLE_COLORS) != 0;
  for (int32_t i = 0; i < n; ++i) {
    const o3s_submap* m = maps[i];
    if (m->n <= 0) continue;
    total += m->n;
    if (total > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
    ++K;
    hn = hn && m->has_normals == 1;  // an attribute only some submaps carry is dropped (Open3D's HasNormals() of the mixed cloud)
    hc = hc && m->has_colors == 1;
  }
  if (total == 0) {  // "no submaps" / all empty: an empty cloud (Mapper.cpp:509-512)
    a->n = 0;
    a->has_normals = a->has_colors = 0;
    if (n_out) *n_out = 0;
    return O3S_OK;
  }
  if (hipSetDevice(a->device) != hipSuccess) return O3S_ERR_HIP;
  // what the submaps' own streams still have in flight (an insert's tail, a transform) is waited for: each distinct stream once
  for (int32_t i = 0; i < n; ++i) {
    bool seen = false;
    for (int32_t j = 0; j < i && !seen; ++j) seen = maps[j]->stream == maps[i]->stream;
    if (!seen) CK(hipStreamSynchronize(maps[i]->stream));
  }
  hipStream_t s = maps[0]->stream;

  // ---- the segment table: [start (K + 1) | pts (K) | nrm (K) | col (K)], staged in the thread's pinned area when it fits
  const size_t tbytes = (size_t)(4 * K + 1) * 8;
  CK(a->table.ensure(tbytes, 0, s));
  std::vector<uint64_t> pageable;
  uint64_t* h = nullptr;
  if (tbytes <= 4096 && pinned_words()) h = reinterpret_cast<uint64_t*>(pinned_words());
  else {
    pageable.resize((size_t)4 * K + 1);
    h = pageable.data();
  }
  {
    int k = 0;
    int64_t at = 0;
    for (int32_t i = 0; i < n; ++i) {
      const o3s_submap* m = maps[i];
      if (m->n <= 0) continue;
      const int c = m->cur;
      h[k] = (uint64_t)at;
      h[(size_t)K + 1 + k] = (uint64_t)(uintptr_t)m->pts[c].p;
      h[(size_t)2 * K + 1 + k] = (uint64_t)(uintptr_t)(hn ? m->nrm[c].p : nullptr);
      h[(size_t)3 * K + 1 + k] = (uint64_t)(uintptr_t)(hc ? m->col[c].p : nullptr);
      at += m->n;
      ++k;
    }
    h[K] = (uint64_t)total;
  }
  CK(hipMemcpyAsync(a->table.p, h, tbytes, hipMemcpyHostToDevice, s));
  AsmTable t;
  {
    const char* b = reinterpret_cast<const char*>(a->table.p);
    t.start = reinterpret_cast<const int64_t*>(b);
    t.pts = reinterpret_cast<const double* const*>(b + (size_t)(K + 1) * 8);
    t.nrm = reinterpret_cast<const double* const*>(b + (size_t)(2 * K + 1) * 8);
    t.col = reinterpret_cast<const double* const*>(b + (size_t)(3 * K + 1) * 8);
    t.K = K;
  }

  if (!(voxel_size > 0.0)) {  // ---- the plain concatenation
    a->n = 0;                 // the arrays are about to be rewritten: a failure below leaves an empty result
    const size_t bytes = (size_t)total * 24;
    CK(a->pts.ensure(bytes, 0, s));
    if (hn) CK(a->nrm.ensure(bytes, 0, s));
    if (hc) CK(a->col.ensure(bytes, 0, s));
    hipLaunchKernelGGL(k_asm_concat, dim3(nblk(3 * total)), dim3(kB), 0, s, t, total, a->pts.as<double>(), hn ? a->nrm.as<double>() : nullptr, hc ? a->col.as<double>() : nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(s));
    a->n = total;
    a->has_normals = hn ? 1 : 0;
    a->has_colors = hc ? 1 : 0;
    if (n_out) *n_out = total;
    return O3S_OK;
  }

  // ---- Open3D VoxelDownSample of the concatenation
  const int64_t N = total;
  const size_t tb_scan = scan_temp_bytes(N), tb_sort = sort_temp_bytes(N);
  AssembleArea ar;
  CK(lay_out(a->arena, ar, (size_t)N, tb_scan, tb_sort));
  uint32_t* blk = reinterpret_cast<uint32_t*>(ar.tmp);  // k_heads' per-block counts (room: scan_temp_bytes), consumed by the scan right behind
  const unsigned nb = nblk(N);
  // 1. exact min and max bound over all segments, read back once
  const AsmPoints cloud{t};
  unsigned long long bnd[6];
  if (const int rc = cloud_bounds(cloud, N, ar.d_bb, s, bnd); rc != O3S_OK) return rc;
  // anchor = min_bound - voxel / 2; extents from the max bound with the kernel's own expression (IEEE fp64 on both sides)
  double anchor[3];
  uint64_t ext[3];
  for (int k = 0; k < 3; ++k) {
    anchor[k] = from_ordered_bits(bnd[k]) - voxel_size * 0.5;
    const double top = std::floor((from_ordered_bits(bnd[3 + k]) - anchor[k]) / voxel_size);
    if (!std::isfinite(top) || top < 0.0 || top > 2147483646.0) return O3S_ERR_BAD_ARGUMENT;  // (the previous result is untouched)
    ext[k] = (uint64_t)top + 1;
  }
  const long double prod = (long double)ext[0] * (long double)ext[1] * (long double)ext[2];
  if (prod >= 9.0e18L) return O3S_ERR_BAD_ARGUMENT;  // voxel index range does not pack into 63 bits
  const int bits = key_bits((uint64_t)prod);
  // 2. - 4. keys from the segments (Open3D's voxel index floor((p - anchor) / voxel), packed (z, y, x); the value is the global
  // ordinal; floor((x - a) / v) is monotone in x, so every index is inside the extents), stable sort, heads, flag scan
  hipLaunchKernelGGL(k_grid_keys<AsmPoints>, dim3(nb), dim3(kB), 0, s, cloud, N, voxel_size, anchor[0], anchor[1], anchor[2], ext[0], ext[1], ar.keys, ar.vals);
  size_t tb = tb_sort;
  CK(sort_pairs(ar.tmp, tb, ar.keys, ar.keys2, ar.vals, ar.vals2, (size_t)N, bits, s));
  hipLaunchKernelGGL(k_heads, dim3(nb), dim3(kB), 0, s, ar.keys2, N, ~0ull /*no key is excluded*/, ar.head, 0, blk);
  int64_t n_vox = 0;
  {
    const int rc = scan_flags(ar.head, ar.ord, N, ar.tmp, tb_scan, &n_vox, s, blk);
    if (rc != O3S_OK) return rc;
  }
  if (n_vox <= 0 || n_vox > N) return O3S_ERR_HIP;
  // 5. the per-voxel means, gathered from the segments by ordinal
  a->n = 0;  // the arrays are about to be rewritten: a failure below leaves an empty result
  const size_t bytes = (size_t)n_vox * 24;
  CK(a->pts.ensure(bytes, 0, s));
  if (hn) CK(a->nrm.ensure(bytes, 0, s));
  if (hc) CK(a->col.ensure(bytes, 0, s));
  hipLaunchKernelGGL(k_asm_reduce, dim3(nb), dim3(kB), 0, s, t, ar.keys2, ar.vals2, ar.head, ar.ord, N, a->pts.as<double>(), hn ? a->nrm.as<double>() : nullptr,
                     hc ? a->col.as<double>() : nullptr);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s));
  a->n = n_vox;
  a->has_normals = hn ? 1 : 0;
  a->has_colors = hc ? 1 : 0;
  if (n_out) *n_out = n_vox;
  return O3S_OK;
}

int o3s_assembled_map_download(const o3s_assembled_map* a, double* pts, double* normals, double* colors) {
  if (!a || (a->n > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  if ((normals && !o3s_assembled_map_has_normals(a)) || (colors && !o3s_assembled_map_has_colors(a))) return O3S_ERR_BAD_SHAPE;
  if (a->n == 0) return O3S_OK;
  if (hipSetDevice(a->device) != hipSuccess) return O3S_ERR_HIP;
  const size_t bytes = (size_t)a->n * 24;
  CK(hipMemcpy(pts, a->pts.p, bytes, hipMemcpyDeviceToHost));
  if (normals) CK(hipMemcpy(normals, a->nrm.p, bytes, hipMemcpyDeviceToHost));
  if (colors) CK(hipMemcpy(colors, a->col.p, bytes, hipMemcpyDeviceToHost));
  return O3S_OK;
}

int o3s_assembled_map_to_submap(const o3s_assembled_map* a, o3s_submap* dst) {
  if (const int rs_ = submap_settle(dst); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!a || !dst || dst->device != a->device) return O3S_ERR_BAD_ARGUMENT;
  const int rc = set_dev(dst);
  if (rc != O3S_OK) return rc;
  hipStream_t s = dst->stream;
  const int c = dst->cur;
  const size_t bytes = (size_t)a->n * 24;
  const bool hn = o3s_assembled_map_has_normals(a) != 0, hc = o3s_assembled_map_has_colors(a) != 0;
  CK(dst->pts[c].ensure(bytes, 0, s));
  if (hn) CK(dst->nrm[c].ensure(bytes, 0, s));
  if (hc) CK(dst->col[c].ensure(bytes, 0, s));
  if (a->n > 0) {
    CK(hipMemcpyAsync(dst->pts[c].p, a->pts.p, bytes, hipMemcpyDeviceToDevice, s));
    if (hn) CK(hipMemcpyAsync(dst->nrm[c].p, a->nrm.p, bytes, hipMemcpyDeviceToDevice, s));
    if (hc) CK(hipMemcpyAsync(dst->col[c].p, a->col.p, bytes, hipMemcpyDeviceToDevice, s));
  }
  CK(hipStreamSynchronize(s));
  dst->n = a->n;
  dst->layout_valid = false;
  dst->has_normals = a->n == 0 ? -1 : (hn ? 1 : 0);
  dst->has_colors = hc ? 1 : 0;
  dst->n_feat = -1;  // the features described the map that is gone
  return O3S_OK;
}

}  // extern "C"
