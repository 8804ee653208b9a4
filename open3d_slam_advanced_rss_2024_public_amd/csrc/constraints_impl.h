// constraints_impl.h — host side of o3s_submaps_odometry_constraints (include/constraints/o3s_constraints.h); the kernels are in
// constraints_dev.h.  Included at the end of cloud_ops.hip after o3d_icp_impl.h (its work area lives in RegArea) and submap_impl.h.
//
// One call = one sequence of launches over ALL its pairs on one stream and one wait: the pair table goes up, six kernels and a
// sort run, k_oc_post writes every pair's sums, counts and error word into the work area's pinned block and publishes through the
// calling thread's mailbox.  Only a voxel-table slice that filled up (more than 2^16 overlap voxels in one pair) makes a second
// pass, with room for one voxel per point, as overlap_dev does.  Calls whose pairs hold more than kOcChunkPoints points together
// are cut into chunks of whole pairs, one such sequence each.
#pragma once
#include <algorithm>

#include "../../include/constraints/o3s_constraints.h"
#include "constraints_dev.h"
#include "o3d_icp_impl.h"
#include "submap_impl.h"

namespace {
namespace o3s_cloud {

constexpr int64_t kOcChunkPoints = (int64_t)1 << 29;  // points of one sequence of launches: 32-bit bases, table offsets and block numbers

struct OcSizes {  // sizes of one chunk, from the host's view of its pairs
  uint32_t slots = 0, n_buckets = 0, blocks_all = 0, blocks_src = 0;
  int64_t G = 0, Mt = 0;
  size_t tb_sort = 0;
};
// work area of one chunk of m pairs
struct OcArea {
  static constexpr size_t kSlack = 4096;
  OcPair* d_pairs;
  OvSlot* tab;
  uint32_t *slot_of, *flag;
  uint32_t* err;  // a bad coordinate per pair [m], a table slice is full [1], the selection sizes [2 m]
  uint32_t* cnt(int m) const { return err + (m + 1); }  // ... the selection sizes
  uint32_t* blk_cnt;
  uint64_t *k1, *k2;
  uint32_t *v1, *v2;
  char* tmp;
  uint2* range;
  OcRec* rec;
  double *part, *sums;
  template <class A>
  void lay(A& a, int m, const OcSizes& L) {
    take(a, d_pairs, (size_t)m);
    take(a, tab, (size_t)L.slots);
    take(a, slot_of, (size_t)L.G);
    take(a, flag, (size_t)L.G);
    take(a, err, (size_t)(3 * m + 1));
    take(a, blk_cnt, (size_t)L.blocks_all);
    take(a, k1, (size_t)L.Mt);
    take(a, k2, (size_t)L.Mt);
    take(a, v1, (size_t)L.Mt);
    take(a, v2, (size_t)L.Mt);
    take(a, tmp, L.tb_sort);
    take(a, range, (size_t)L.n_buckets);
    take(a, rec, (size_t)L.Mt);
    take(a, part, (size_t)kOcComps * L.blocks_src);
    take(a, sums, (size_t)m * kOcComps);
  }
};

// the pairs idx[0..m) of the call, enqueued and waited for once per attempt.  status / info / counts are written for every pair.
int oc_run_chunk(RegArea& area, const std::vector<int32_t>& idx, const o3s_submap* const* sources, const o3s_submap* const* targets, const double* Ts,
                 double voxel, int64_t min_pts, double max_dist, double* infos, int64_t* n_overlaps, int64_t* n_corr, int32_t* statuses, hipStream_t s) {
  const int m = (int)idx.size();
  std::vector<OcPair> pairs((size_t)m);
  for (int attempt = 0;; ++attempt) {
    OcSizes L;
    bool all_full_size = true;
    for (int k = 0; k < m; ++k) {
      const o3s_submap *src = sources[idx[(size_t)k]], *tgt = targets[idx[(size_t)k]];
      OcPair& P = pairs[(size_t)k];
      P.sp = src->pts[src->cur].as<double>();
      P.tp = tgt->pts[tgt->cur].as<double>();
      P.ns = src->n;
      P.nt = tgt->n;
      P.has_T = Ts ? 1 : 0;
      P.apply_search = 0;
      for (int e = 0; e < 16; ++e) P.T[e] = Ts ? Ts[16 * (size_t)idx[(size_t)k] + e] : (e % 5 == 0 ? 1.0 : 0.0);
      if (Ts) P.apply_search = h_is_identity(P.T) ? 0 : 1;
      const uint32_t full = ov_slots_for(P.ns + P.nt), slots = attempt == 0 ? std::min(kOvFirstSlots, full) : full;
      all_full_size = all_full_size && slots == full;
      P.tab_off = L.slots;
      P.tab_mask = slots - 1u;
      L.slots += slots;
      P.blk_s = L.blocks_all;
      P.blk_t = P.blk_s + nblk(P.ns);
      L.blocks_all = P.blk_t + nblk(P.nt);
      P.sblk = L.blocks_src;
      L.blocks_src += nblk(P.ns);
      P.g_s = (uint32_t)L.G;
      P.g_t = (uint32_t)(L.G + P.ns);
      L.G += P.ns + P.nt;
      P.t_base = (uint32_t)L.Mt;
      L.Mt += P.nt;
    }
    L.n_buckets = 1u << 10;
    while ((int64_t)L.n_buckets < L.Mt && L.n_buckets < (1u << 31)) L.n_buckets <<= 1;
    L.tb_sort = sort_temp_bytes(L.Mt);

    OcArea w;
    CK(lay_out(area.ov.arena, w, m, L));
    // the host's block: pinned, mapped, grow-only (a pinned allocation takes milliseconds: once per size)
    const size_t res_bytes = (size_t)m * kOcRes * 8;
    if (!area.oc_res || area.oc_res_bytes < res_bytes) {
      area.oc_res.release();
      area.oc_res_bytes = 0;
      CK(area.oc_res.alloc(res_bytes + res_bytes / 2));
      area.oc_res_bytes = res_bytes + res_bytes / 2;
    }

    CK(hipMemcpyAsync(w.d_pairs, pairs.data(), (size_t)m * sizeof(OcPair), hipMemcpyHostToDevice, s));  // pageable source: staged before the call returns
    CK(hipMemsetAsync(w.tab, 0, (size_t)L.slots * sizeof(OvSlot), s));
    CK(hipMemsetAsync(w.err, 0, (size_t)(3 * m + 1) * 4, s));
    CK(hipMemsetAsync(w.range, 0, (size_t)L.n_buckets * 8, s));
    hipLaunchKernelGGL(k_oc_count, dim3(L.blocks_all), dim3(kB), 0, s, (const OcPair*)w.d_pairs, m, 1.0 / voxel, w.tab, w.slot_of, w.err);
    hipLaunchKernelGGL(k_oc_flag, dim3(L.blocks_all), dim3(kB), 0, s, (const OcPair*)w.d_pairs, m, (const OvSlot*)w.tab, (const uint32_t*)w.slot_of, min_pts, max_dist,
                       L.n_buckets, w.flag, w.blk_cnt, w.k1, w.v1);
    CK(hipGetLastError());
    size_t stb = L.tb_sort;
    CK(sort_pairs(w.tmp, stb, w.k1, w.k2, w.v1, w.v2, (size_t)L.Mt, key_bits((uint64_t)L.n_buckets + 1u), s));
    hipLaunchKernelGGL(k_oc_heads, dim3(nblk(L.Mt)), dim3(kB), 0, s, (const uint64_t*)w.k2, (const uint32_t*)w.v2, L.Mt, L.n_buckets, (const OcPair*)w.d_pairs, m, w.range,
                       w.rec);
    hipLaunchKernelGGL(k_oc_search, dim3(L.blocks_src), dim3(kB), 0, s, (const OcPair*)w.d_pairs, m, (const uint32_t*)w.flag, (const uint2*)w.range, (const OcRec*)w.rec,
                       L.n_buckets - 1u, max_dist, max_dist * max_dist, w.part);
    hipLaunchKernelGGL(k_oc_fold, dim3((unsigned)(m * kOcFolds)), dim3(64), 0, s, (const OcPair*)w.d_pairs, (const double*)w.part, L.blocks_src, (const uint32_t*)w.blk_cnt, w.sums,
                       w.cnt(m));
    PinnedArea& pa = pinned_area();
    const uint32_t seq = mailbox_open(pa);
    hipLaunchKernelGGL(k_oc_post, dim3(1), dim3(64), 0, s, m, (const double*)w.sums, (const uint32_t*)w.cnt(m), (const uint32_t*)w.err,
                       reinterpret_cast<unsigned long long*>(area.oc_res.dev), seq ? pa.mb.dev : (uint32_t*)nullptr, seq);
    CK(hipGetLastError());
    uint32_t full_word = 0;
    const int posted = fetch_post(pa.mb, seq, s, &full_word, 1, kPostVals, nullptr);
    if (posted == kPollError) return O3S_ERR_HIP;
    if (posted != kPollPosted) CK(hipStreamSynchronize(s));  // posts are off: the block is complete behind the stream
    const uint32_t* res = area.oc_res.host;
    bool full = false;
    for (int k = 0; k < m; ++k) full = full || post_get<uint64_t>(res, 2 * (k * kOcRes + kOcComps + 1)) >> 32 != 0;
    if (full) {  // a pair's first table slice filled up: once more with room for one voxel per point
      if (all_full_size) return O3S_ERR_HIP;
      CK(hipStreamSynchronize(s));  // the arena is laid out afresh
      continue;
    }
    for (int k = 0; k < m; ++k) {
      const size_t o = (size_t)idx[(size_t)k];
      const uint64_t c = post_get<uint64_t>(res, 2 * (k * kOcRes + kOcComps)), e = post_get<uint64_t>(res, 2 * (k * kOcRes + kOcComps + 1));
      const int64_t n_s = (int64_t)(c & 0xffffffffu), n_t = (int64_t)(c >> 32);
      if (e & 0xffffffffu) {  // NaN / voxel index beyond +-2^20: int(floor(.)) is undefined behaviour in the reference
        statuses[o] = O3S_ERR_BAD_ARGUMENT;
        continue;
      }
      if (n_overlaps) {
        n_overlaps[2 * o] = n_s;
        n_overlaps[2 * o + 1] = n_t;
      }
      if (n_s == 0 || n_t == 0) {
        statuses[o] = O3S_ERR_EMPTY_REFERENCE;
        continue;
      }
      double v[kOcComps];
      for (int t = 0; t < kOcComps; ++t) v[t] = post_get<double>(res, 2 * (k * kOcRes + t));
      int t = 0;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
          infos[36 * o + (size_t)(b * 6 + a)] = v[t];
          infos[36 * o + (size_t)(a * 6 + b)] = v[t];
          ++t;
        }
      if (n_corr) n_corr[o] = (int64_t)v[21];
      statuses[o] = O3S_OK;
    }
    return O3S_OK;
  }
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_submaps_odometry_constraints(int32_t n, const o3s_submap* const* sources, const o3s_submap* const* targets, const double* Ts,
                                     double overlap_voxel_size, int64_t min_points_per_voxel, double max_correspondence_distance, double* infos,
                                     int64_t* n_overlaps, int64_t* n_correspondences, int32_t* statuses) {
  using namespace o3s_cloud;
  if (n < 0 || (n > 0 && (!sources || !targets || !infos || !statuses)) || !(overlap_voxel_size > 0.0) || !std::isfinite(overlap_voxel_size) ||
      !(max_correspondence_distance > 0.0) || !std::isfinite(max_correspondence_distance) ||
      max_correspondence_distance < overlap_voxel_size * 0x1p-20 || min_points_per_voxel < 1)
    return O3S_ERR_BAD_ARGUMENT;
  if (n == 0) return O3S_OK;
  const int device = sources[0] ? sources[0]->device : -1;
  for (int32_t k = 0; k < n; ++k)
    if (!sources[k] || !targets[k] || sources[k]->device != device || targets[k]->device != device) return O3S_ERR_BAD_ARGUMENT;
  if (Ts)
    for (size_t e = 0; e < 16 * (size_t)n; ++e)
      if (!std::isfinite(Ts[e])) return O3S_ERR_BAD_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return O3S_ERR_HIP;
  // every submap involved is complete, and its own stream idle, before the call's stream reads it (each distinct stream once)
  std::vector<hipStream_t> drained;
  for (int32_t k = 0; k < n; ++k)
    for (const o3s_submap* sm : {sources[k], targets[k]}) {
      if (const int rs_ = submap_settle(sm); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
      if (std::find(drained.begin(), drained.end(), sm->stream) != drained.end()) continue;
      CK(hipStreamSynchronize(sm->stream));
      drained.push_back(sm->stream);
    }
  hipStream_t s = targets[0]->stream;
  RegLease area(device, s);
  std::vector<int32_t> chunk;
  int64_t chunk_points = 0;
  auto flush = [&]() -> int {
    if (chunk.empty()) return O3S_OK;
    const int rc = oc_run_chunk(*area, chunk, sources, targets, Ts, overlap_voxel_size, min_points_per_voxel, max_correspondence_distance, infos, n_overlaps,
                                n_correspondences, statuses, s);
    chunk.clear();
    chunk_points = 0;
    return rc;
  };
  for (int32_t k = 0; k < n; ++k) {
    std::memset(infos + 36 * (size_t)k, 0, 36 * sizeof(double));
    if (n_overlaps) n_overlaps[2 * k] = n_overlaps[2 * k + 1] = 0;
    if (n_correspondences) n_correspondences[k] = 0;
    const int64_t np = sources[k]->n + targets[k]->n;
    if (sources[k]->n <= 0 || targets[k]->n <= 0) {
      statuses[k] = O3S_ERR_EMPTY_REFERENCE;
      continue;
    }
    if (np > (int64_t)0x7fffffff) {
      statuses[k] = O3S_ERR_BAD_ARGUMENT;
      continue;
    }
    if (chunk_points + np > kOcChunkPoints)
      if (const int rc = flush(); rc != O3S_OK) return rc;
    chunk.push_back(k);
    chunk_points += np;
  }
  if (const int rc = flush(); rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(s));  // a post is read a moment before its kernel retires: the call ends on a drained stream
  return area.end(O3S_OK);
}

}  // extern "C"
