// overlap_impl.h — computeIndicesOfOverlappingPoints (O3S/src/helpers.cpp:319-345) and the loop-closure refinement that
// uses it (O3S/src/PlaceRecognition.cpp:97-150) on the device; gfx950 only.  Included at the end of cloud_ops.hip after
// submap_impl.h (one TU: the voxel key and table of voxel_table.h, the rocPRIM sort / scan instantiations and the
// Open3D-semantics ICP of o3d_icp_impl.h).
//
// The reference fills a VoxelMap (unordered_map voxel key -> per-layer index lists) with the target cloud and with the
// source cloud moved by sourceToTarget, then walks the map and keeps the indices of every voxel that holds at least
// minNumPointsPerVoxel points of BOTH layers.  Here: one packed voxel key per point (getVoxelIdx, reciprocal form,
// VoxelHashMap.hpp:43-51) and ONE open-addressing table keyed by it with a count per layer: the lanes of a wave that fall
// into the same voxel (clouds arrive scan by scan, so most do) add their count with one atomic; a second pass looks every
// point's voxel up.  The overlap voxels are large (2 m: a few thousand of them under 0.5 M points), so the table starts at
// 2^16 slots; a table that fills up is reported and the pass repeated with room for one voxel per point.  (Round 3 sorted both
// 64-bit key arrays — rocPRIM takes its merge sort for them — and searched them per point: 0.46 ms of a 3.1 ms refinement.)
// The reference's output order is its hash map's iteration order (unspecified); ascending index order is used here, on the
// device and in the oracle.
#pragma once
#include "o3d_icp_impl.h"
#include "submap_impl.h"
#include "voxel_table.h"

namespace {
namespace o3s_cloud {

// Open3D PointCloud::Transform on points only: p' = (T [p 1]).head<3>() / w (same arithmetic as k_transform_append)
__global__ void __launch_bounds__(kB) k_ov_keys(const double* __restrict__ pts, int64_t N, const double* __restrict__ Tm /*nullable: identity*/,
                                                double inv, uint64_t* __restrict__ keys, uint32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  if (Tm) o3d_transform_point(Tm, x, y, z);
  const uint64_t k = vm_key(x, y, z, inv);
  keys[i] = k;
  if (k == kDmEmpty) *err = 1u;
}

// counts the points of `layer` per voxel and notes every point's slot.  keys[i] must hold the voxel key of point i (k_ov_keys);
// err[1] = the table is full.
__global__ void __launch_bounds__(kB) k_ov_count(const uint64_t* __restrict__ keys, int64_t N, OvSlot* __restrict__ tab, uint32_t mask, int layer,
                                                 uint32_t* __restrict__ slot_of, uint32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const uint64_t k = i < N ? keys[i] : kDmEmpty;
  bool pending = k != kDmEmpty;  // out-of-range points carry kDmEmpty (and have raised err[0])
  uint32_t my_slot = 0xffffffffu;
  for (;;) {
    const unsigned long long open = __ballot(pending);
    if (!open) break;
    const int leader = __ffsll((long long)open) - 1;
    const uint64_t lk = wave_bcast_u64(k, leader);
    const bool same = pending && k == lk;
    const unsigned long long grp = __ballot(same);
    uint32_t h = 0xffffffffu;
    if (lane == leader) h = ov_count_key(lk, tab, mask, layer, (uint32_t)__popcll(grp), err + 1);
    h = (uint32_t)__shfl((int)h, leader);
    my_slot = same ? h : my_slot;
    pending = pending && !same;
  }
  if (i < N) slot_of[i] = my_slot;
}

// flag[i] = 1 iff the voxel of point i holds >= min_pts points of its own layer and of the other layer (slot_of: where k_ov_count
// found or made the voxel's entry; 0xffffffff: no entry — a point beyond the index range, or a table that overflowed: the pass is repeated)
__global__ void __launch_bounds__(kB) k_ov_flag(const uint32_t* __restrict__ slot_of, int64_t N, const OvSlot* __restrict__ tab, int layer, int64_t min_pts,
                                                uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  const uint32_t h = slot_of[i];
  bool in = false;
  if (h != 0xffffffffu) {
    const OvSlot sl = tab[h];
    in = (int64_t)sl.n[1 - layer] >= min_pts && (min_pts <= 1 || (int64_t)sl.n[layer] >= min_pts);
  }
  flag[i] = in ? 1u : 0u;
}

// SelectByIndex of the target with its normals (k_compact) that also keeps the bounds of what it writes, in the replicas of a bounds
// block (cloud_bounds.h; bounds_begin before): the index over the selection is built next, and the pass over it that would find its
// bounds again, with a wait of its own, is saved.
__global__ void __launch_bounds__(kB) k_compact_bounds(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t N,
                                                       const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off, double* __restrict__ out_pts,
                                                       double* __restrict__ out_n, unsigned long long* __restrict__ slots) {
  BoundsAcc<> acc;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < N; i += (int64_t)gridDim.x * kB) {
    if (!flag[i]) continue;
    const int64_t o = (int64_t)off[i];
    double v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = pts[3 * i + a];
      out_pts[3 * o + a] = v[a];
      out_n[3 * o + a] = nrm[3 * i + a];
    }
    acc.add(v[0], v[1], v[2]);
  }
  bounds_flush(acc, slots);
}

// the selection's one hand-over to the host: both counts (off[n] = the number of set flags) and the two error words (kOvCounts),
// with `slots` also the folded bounds of the selected target (kOvBounds: 8-byte values, maxima un-complemented), then the
// sequence number.  One wave: a replica per lane.
constexpr int kOvCounts = kPostVals, kOvBounds = kOvCounts + 4;
static_assert(kOvBounds + 12 <= kLazySlot, "the eager posts stay clear of the slot that is read later");
__global__ void __launch_bounds__(64) k_ov_post(const uint32_t* __restrict__ fs, uint32_t* __restrict__ os, int64_t Ns, const uint32_t* __restrict__ ft,
                                                uint32_t* __restrict__ ot, int64_t Nt, const uint32_t* __restrict__ err,
                                                const unsigned long long* __restrict__ slots /*nullable*/, uint32_t* __restrict__ mailbox, uint32_t seq) {
  if (blockIdx.x != 0) return;
  if (slots && mailbox) {
    unsigned long long v[6];
    fold_bounds(slots, v);
    if (threadIdx.x == 0) post_store(mailbox, kOvBounds, v);
  }
  if (threadIdx.x != 0) return;
  const uint32_t ns = os[Ns - 1] + fs[Ns - 1], nt = ot[Nt - 1] + ft[Nt - 1];
  os[Ns] = ns;
  ot[Nt] = nt;
  if (mailbox) {
    const uint32_t v[4] = {ns, nt, err[0], err[1]};
    post(mailbox, seq, kOvCounts, v);
  }
}

// What o3s_o3d_registration_icp_submaps_overlap lets the selection do on the way, when its output buffers can hold either cloud
// whole (o3s_o3d_registration_reserve): the two SelectByIndex copies are enqueued BEFORE the counts are known and the bounds of the
// selected target travel with the counts.
struct OvSelect {
  const double* tgt_normals = nullptr;
  const double* src_normals = nullptr;  // nullable: the source's normals are selected too (Generalized ICP builds its covariances from them)
  double *out_src = nullptr, *out_tgt = nullptr, *out_tgt_n = nullptr, *out_src_n = nullptr;
  unsigned long long bounds[6] = {0, 0, 0, 0, 0, 0};  // of the selected target: minima, maxima (ordered bit patterns)
  bool have_bounds = false;  // ... and the two copies have been made
};

__global__ void __launch_bounds__(kB) k_ov_indices(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off, int64_t N,
                                                   int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i < N && flag[i]) out[off[i]] = i;
}

// work area of the overlap selection of a source of ns and a target of nt points (tb_scan: a scan of max(ns, nt) flags)
struct OverlapArea {
  static constexpr size_t kSlack = 4096;
  uint64_t *ks, *kt;
  uint32_t *fs, *ft;
  uint32_t *os, *ot;  // first each point's slot (k_ov_count), then the offsets: the scans overwrite the slots once the flags are made
  char* tmp;
  OvSlot* tab;
  uint32_t* err;
  double* d_T;
  unsigned long long* bb;  // folded by k_ov_post, with the counts
  template <class A>
  void lay(A& a, size_t ns, size_t nt, size_t slots, size_t tb_scan) {
    take(a, ks, ns);
    take(a, kt, nt);
    take(a, fs, ns);
    take(a, ft, nt);
    take(a, os, ns + 1);
    take(a, ot, nt + 1);
    take(a, tmp, tb_scan);
    take(a, tab, slots);
    take(a, err, 16);
    take(a, d_T, 16);
    take(a, bb, kBoundsReplicaWords);
  }
};

size_t reg_overlap_arena_bytes(int64_t Ns, int64_t Nt) {  // with the table at its largest
  return layout_bytes<OverlapArea>((size_t)Ns, (size_t)Nt, (size_t)ov_slots_for(Ns + Nt), scan_temp_bytes(std::max(Ns, Nt)));
}

// flags + exclusive offsets of both layers on the device; counts on the host.  d_T: 16 doubles on the device.
inline int overlap_dev(OverlapWork& w, const double* d_src, int64_t Ns, const double* d_tgt, int64_t Nt, const double T[16], double voxel,
                       int64_t min_pts, uint32_t** flag_s, uint32_t** off_s, int64_t* n_s, uint32_t** flag_t, uint32_t** off_t, int64_t* n_t,
                       hipStream_t s, OvSelect* sel = nullptr) {
  *n_s = *n_t = 0;
  if (sel) sel->have_bounds = false;
  if (Ns > (int64_t)0x7fffffff || Nt > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  uint32_t slots = std::min(kOvFirstSlots, ov_slots_for(Ns + Nt));
  OverlapArea a;
  const size_t tb_scan = scan_temp_bytes(std::max(Ns, Nt));
  for (int attempt = 0;; ++attempt) {
    if (sel) sel->have_bounds = false;  // an attempt whose table filled up has posted the bounds of an INCOMPLETE selection: never carried over
    CK(lay_out(w.arena, a, (size_t)Ns, (size_t)Nt, (size_t)slots, tb_scan));
    CK(hipMemsetAsync(a.err, 0, 8, s));
    CK(hipMemsetAsync(a.tab, 0, (size_t)slots * sizeof(OvSlot), s));
    CK(hipMemcpyAsync(a.d_T, T, 16 * sizeof(double), hipMemcpyHostToDevice, s));  // pageable source: staged before the call returns
    const double inv = 1.0 / voxel;
    hipLaunchKernelGGL(k_ov_keys, dim3(nblk(Ns)), dim3(kB), 0, s, d_src, Ns, (const double*)a.d_T, inv, a.ks, a.err);
    hipLaunchKernelGGL(k_ov_keys, dim3(nblk(Nt)), dim3(kB), 0, s, d_tgt, Nt, (const double*)nullptr, inv, a.kt, a.err);
    // the slots land in the offset arrays, which the scans below overwrite once the flags are made
    hipLaunchKernelGGL(k_ov_count, dim3(nblk(Ns)), dim3(kB), 0, s, a.ks, Ns, a.tab, slots - 1u, 0, a.os, a.err);
    hipLaunchKernelGGL(k_ov_count, dim3(nblk(Nt)), dim3(kB), 0, s, a.kt, Nt, a.tab, slots - 1u, 1, a.ot, a.err);
    hipLaunchKernelGGL(k_ov_flag, dim3(nblk(Ns)), dim3(kB), 0, s, (const uint32_t*)a.os, Ns, a.tab, 0, min_pts, a.fs);
    hipLaunchKernelGGL(k_ov_flag, dim3(nblk(Nt)), dim3(kB), 0, s, (const uint32_t*)a.ot, Nt, a.tab, 1, min_pts, a.ft);
    CK(hipGetLastError());
    // both scans, then ONE hand-over of the two counts and the error words (three separate waits — two counts and a copied-back error
    // word — were 40-50 us of a refinement)
    int rc = scan_flags_dev(a.fs, a.os, Ns, a.tmp, tb_scan, s);
    if (rc != O3S_OK) return rc;
    rc = scan_flags_dev(a.ft, a.ot, Nt, a.tmp, tb_scan, s);
    if (rc != O3S_OK) return rc;
    uint32_t herr[2] = {0, 0};
    {
      PinnedArea& pa = pinned_area();
      const uint32_t seq = mailbox_open(pa);
      const bool with_sel = sel && seq;
      if (with_sel) {  // the two selections, enqueued before their sizes are known (the buffers hold either cloud whole)
        if (const int rb = bounds_begin(a.bb, s); rb != O3S_OK) return rb;
        hipLaunchKernelGGL(k_compact, dim3(nblk(Ns)), dim3(kB), 0, s, d_src, sel->src_normals, Ns, (const uint32_t*)a.fs, (const uint32_t*)a.os, sel->out_src,
                           sel->out_src_n, (int32_t*)nullptr);
        hipLaunchKernelGGL(k_compact_bounds, dim3(std::min(nblk(Nt), 1024u)), dim3(kB), 0, s, d_tgt, sel->tgt_normals, Nt, (const uint32_t*)a.ft,
                           (const uint32_t*)a.ot, sel->out_tgt, sel->out_tgt_n, a.bb);
      }
      hipLaunchKernelGGL(k_ov_post, dim3(1), dim3(64), 0, s, (const uint32_t*)a.fs, a.os, Ns, (const uint32_t*)a.ft, a.ot, Nt, (const uint32_t*)a.err,
                         with_sel ? (const unsigned long long*)a.bb : (const unsigned long long*)nullptr, seq ? pa.mb.dev : (uint32_t*)nullptr, seq);
      CK(hipGetLastError());
      uint32_t r[4 + 12];
      const int posted = fetch_post(pa.mb, seq, s, r, with_sel ? 16 : 4, kOvCounts, nullptr);
      if (posted == kPollError) return O3S_ERR_HIP;
      if (posted == kPollPosted) {
        *n_s = (int64_t)r[0];
        *n_t = (int64_t)r[1];
        herr[0] = r[2];
        herr[1] = r[3];
        if (with_sel) {
          std::memcpy(sel->bounds, r + 4, sizeof(sel->bounds));
          sel->have_bounds = *n_t > 0;
        }
      } else {
        if (sel) sel->have_bounds = false;  // the caller falls back to its own compaction and bounds pass
        uint32_t cnt[2] = {0, 0};
        CK(hipMemcpyAsync(&cnt[0], a.os + Ns, 4, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(&cnt[1], a.ot + Nt, 4, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(herr, a.err, 8, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        *n_s = (int64_t)cnt[0];
        *n_t = (int64_t)cnt[1];
      }
    }
    if (herr[0]) return O3S_ERR_BAD_ARGUMENT;  // NaN / voxel index beyond +-2^20: int(floor(.)) is undefined behaviour in the reference
    if (!herr[1]) break;
    // the first table filled up (more than 2^16 overlap voxels: rare): once more with room for one voxel per point
    if (attempt > 0 || slots >= ov_slots_for(Ns + Nt)) return O3S_ERR_HIP;
    slots = ov_slots_for(Ns + Nt);
    *n_s = *n_t = 0;
  }
  *flag_s = a.fs;
  *off_s = a.os;
  *flag_t = a.ft;
  *off_t = a.ot;
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_overlap_indices(int device, const double* source, int64_t Ns, const double* target, int64_t Nt, const double source_to_target[16],
                        double voxel_size, int64_t min_points_per_voxel, int64_t* idx_source, int64_t* n_source, int64_t* idx_target,
                        int64_t* n_target) {
  using namespace o3s_cloud;
  if (!n_source || !n_target || !source_to_target || Ns < 0 || Nt < 0 || !(voxel_size > 0.0) || min_points_per_voxel < 1)
    return O3S_ERR_BAD_ARGUMENT;
  *n_source = *n_target = 0;
  if (Ns == 0 || Nt == 0) return O3S_OK;
  if (!source || !target || !idx_source || !idx_target) return O3S_ERR_BAD_ARGUMENT;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_s, d_t, d_is, d_it;
  CK(d_s.alloc((size_t)Ns * 24));
  CK(d_t.alloc((size_t)Nt * 24));
  CK(hipMemcpyAsync(d_s.p, source, (size_t)Ns * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(d_t.p, target, (size_t)Nt * 24, hipMemcpyHostToDevice, s));
  RegLease area(device, s);
  OverlapWork& w = area->ov;
  uint32_t *fs, *os, *ft, *ot;
  int64_t ns = 0, nt = 0;
  rc = overlap_dev(w, d_s.as<double>(), Ns, d_t.as<double>(), Nt, source_to_target, voxel_size, min_points_per_voxel, &fs, &os, &ns, &ft, &ot, &nt, s);
  if (rc != O3S_OK) return rc;
  CK(d_is.alloc((size_t)std::max<int64_t>(ns, 1) * 8));
  CK(d_it.alloc((size_t)std::max<int64_t>(nt, 1) * 8));
  hipLaunchKernelGGL(k_ov_indices, dim3(nblk(Ns)), dim3(kB), 0, s, fs, os, Ns, d_is.as<int64_t>());
  hipLaunchKernelGGL(k_ov_indices, dim3(nblk(Nt)), dim3(kB), 0, s, ft, ot, Nt, d_it.as<int64_t>());
  CK(hipGetLastError());
  if (ns) CK(hipMemcpyAsync(idx_source, d_is.p, (size_t)ns * 8, hipMemcpyDeviceToHost, s));
  if (nt) CK(hipMemcpyAsync(idx_target, d_it.p, (size_t)nt * 8, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *n_source = ns;
  *n_target = nt;
  return area.end(O3S_OK);
}

}  // extern "C"

namespace {
// the refinement of ONE pair on stream s (both submaps' own streams drained by the caller, the device current)
// est_type: o3s_o3d_estimation_type (point-to-plane: the refinement as it always was); the source's normals are selected for GICP
int refine_overlap_on(const o3s_submap* source, const o3s_submap* target, double max_dist, const double init[16], const o3s_o3d_icp_criteria* criteria,
                      double overlap_voxel_size, int64_t min_points_per_voxel, o3s_o3d_icp_result* result, double* info36, int64_t* n_overlap,
                      hipStream_t s, int est_type = o3s_cloud::kEstPlane, double gicp_epsilon = 1e-3) {
  using namespace o3s_cloud;
  int rc = O3S_OK;
  const bool gicp = est_type == kEstGicp;
  const double* sp = source->pts[source->cur].as<double>();
  const double* tp = target->pts[target->cur].as<double>();
  const double* tn = target->has_normals == 1 ? target->nrm[target->cur].as<double>() : nullptr;
  const double* sn = gicp ? source->nrm[source->cur].as<double>() : nullptr;
  uint32_t *fs, *os, *ft, *ot;
  int64_t ns = 0, nt = 0;
  RegLease area(target->device, s);
  if (gicp) CK(area->ov_srcn.alloc((size_t)source->n * 24));  // grows on the first GICP refinement of an area, then stays
  // with room for either cloud whole (o3s_o3d_registration_reserve) the two SelectByIndex copies and the bounds of the selected target
  // ride on the selection's own hand-over: no wait for the counts in front of the copies, none for the bounds in front of the index
  // (a target without normals — point-to-point — takes the plain copies)
  OvSelect sel;
  const bool roomy = tn && area->ov_src.cap >= (size_t)source->n * 24 && area->ov_tgt.cap >= (size_t)target->n * 24 &&
                     area->ov_tgtn.cap >= (size_t)target->n * 24;
  if (roomy) {
    sel.tgt_normals = tn;
    sel.src_normals = sn;
    sel.out_src = area->ov_src.as<double>();
    sel.out_tgt = area->ov_tgt.as<double>();
    sel.out_tgt_n = area->ov_tgtn.as<double>();
    sel.out_src_n = gicp ? area->ov_srcn.as<double>() : nullptr;
  }
  rc = overlap_dev(area->ov, sp, source->n, tp, target->n, init, overlap_voxel_size, min_points_per_voxel, &fs, &os, &ns, &ft, &ot, &nt, s, roomy ? &sel : nullptr);
  if (rc != O3S_OK) return rc;
  if (n_overlap) {
    n_overlap[0] = ns;
    n_overlap[1] = nt;
  }
  if (ns == 0 || nt == 0) return O3S_ERR_EMPTY_REFERENCE;
  if (!sel.have_bounds) {
    // source.SelectByIndex(sourceIdxs) / target.SelectByIndex(targetIdxs) in HBM (ascending index order)
    CK(area->ov_src.alloc((size_t)ns * 24));
    CK(area->ov_tgt.alloc((size_t)nt * 24));
    CK(area->ov_tgtn.alloc((size_t)nt * 24));
    hipLaunchKernelGGL(k_compact, dim3(nblk(source->n)), dim3(kB), 0, s, sp, sn, source->n, fs, os, area->ov_src.as<double>(),
                       gicp ? area->ov_srcn.as<double>() : (double*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_compact, dim3(nblk(target->n)), dim3(kB), 0, s, tp, tn, target->n, ft, ot, area->ov_tgt.as<double>(), area->ov_tgtn.as<double>(),
                       (int32_t*)nullptr);
    CK(hipGetLastError());
  }
  O3dEstIn e;
  e.type = est_type;
  e.eps = gicp_epsilon;
  e.src_n = gicp ? area->ov_srcn.as<double>() : nullptr;
  rc = o3d_icp_run(area->reg, area->ov_src.as<double>(), ns, area->ov_tgt.as<double>(), tn ? area->ov_tgtn.as<double>() : nullptr, nt, max_dist, init,
                   criteria, result, s, /*on_device=*/true, sel.have_bounds ? sel.bounds : nullptr, &e);
  if (rc == O3S_OK && info36) rc = o3d_info_after_icp(area->reg, max_dist, result->transformation, info36, s);
  return area.end(rc);
}

// streams of the batch entry's lanes: made once per device, kept for the life of the process (a stream costs ~3 ms to create)
constexpr int kLanes = 4;
inline o3s_cloud::DeviceStreams<kLanes>& lane_streams() {
  static auto* p = new o3s_cloud::DeviceStreams<kLanes>;  // never destroyed (see DeviceStreams)
  return *p;
}
inline hipStream_t lane_stream(int device, int lane) {  // the device is current; a device that could not make every lane's stream has none
  const auto set = lane_streams().get(device);
  return set.n == kLanes ? set.s[lane % kLanes] : nullptr;
}
namespace o3s_cloud {
void reg_warm_lane_streams(int device) { (void)lane_streams().get(device); }  // o3s_o3d_registration_reserve_n with count > 1
}  // namespace o3s_cloud
}  // namespace

namespace {
// o3s_o3d_registration_icp_submaps_overlap[_ex]
int refine_overlap_entry(const o3s_submap* source, const o3s_submap* target, double max_dist, const double init[16], const o3s_o3d_icp_criteria* criteria,
                         double overlap_voxel_size, int64_t min_points_per_voxel, o3s_o3d_icp_result* result, double* info36, int64_t* n_overlap, int est_type,
                         double gicp_epsilon) {
  using namespace o3s_cloud;
  if (!source || !target || !init || !result || !(max_dist > 0.0) || !(overlap_voxel_size > 0.0) || min_points_per_voxel < 1)
    return O3S_ERR_BAD_ARGUMENT;
  if (source->device != target->device) return O3S_ERR_BAD_ARGUMENT;
  if (n_overlap) n_overlap[0] = n_overlap[1] = 0;
  if (const int rs_ = submap_settle(source); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (const int rt_ = submap_settle(target); rt_ != O3S_OK) return rt_;
  if (source->n == 0 || target->n == 0) return O3S_ERR_EMPTY_REFERENCE;
  if (est_type != kEstPoint && target->has_normals != 1) return O3S_ERR_BAD_SHAPE;  // "requires target pointcloud to have normals"
  if (est_type == kEstGicp && source->has_normals != 1) return O3S_ERR_BAD_SHAPE;   // GICP's covariances come from the normals
  int rc = set_dev(target);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(source->stream));
  CK(hipStreamSynchronize(target->stream));
  return refine_overlap_on(source, target, max_dist, init, criteria, overlap_voxel_size, min_points_per_voxel, result, info36, n_overlap, target->stream,
                           est_type, gicp_epsilon);
}

// o3s_o3d_registration_icp_submaps_overlap_batch[_ex]
int refine_overlap_batch(int32_t n, const o3s_submap* const* sources, const o3s_submap* const* targets, double max_dist, const double* inits,
                         const o3s_o3d_icp_criteria* criteria, double overlap_voxel_size, int64_t min_points_per_voxel, o3s_o3d_icp_result* results,
                         double* infos, int64_t* n_overlaps, int32_t* statuses, int est_type, double gicp_epsilon) {
  using namespace o3s_cloud;
  if (n < 0 || (n > 0 && (!sources || !targets || !inits || !results || !statuses)) || !(max_dist > 0.0) || !(overlap_voxel_size > 0.0) ||
      min_points_per_voxel < 1)
    return O3S_ERR_BAD_ARGUMENT;
  if (n == 0) return O3S_OK;
  int device = -1;
  for (int32_t k = 0; k < n; ++k) {
    if (!sources[k] || !targets[k] || sources[k]->device != targets[k]->device) return O3S_ERR_BAD_ARGUMENT;
    if (device < 0) device = targets[k]->device;
    if (targets[k]->device != device) return O3S_ERR_BAD_ARGUMENT;  // one device per call (the work areas and the lanes' streams are per device)
  }
  if (hipSetDevice(device) != hipSuccess) return O3S_ERR_HIP;
  for (int32_t k = 0; k < n; ++k) {  // every submap involved is complete before any lane reads it
    if (const int rs_ = submap_settle(sources[k]); rs_ != O3S_OK) return rs_;
    if (const int rt_ = submap_settle(targets[k]); rt_ != O3S_OK) return rt_;
    CK(hipStreamSynchronize(sources[k]->stream));
    CK(hipStreamSynchronize(targets[k]->stream));
  }
  const int lanes = std::min<int>(kLanes, n);
  std::vector<hipStream_t> streams((size_t)lanes);
  for (int l = 0; l < lanes; ++l) {
    // one pair: the target's own stream, like the single call (no lane stream is needed — or made: the first use of the lanes'
    // streams creates them, ~3 ms each, unless o3s_o3d_registration_reserve_n has done so ahead of time)
    streams[(size_t)l] = lanes == 1 ? targets[0]->stream : lane_stream(device, l);
    if (!streams[(size_t)l]) return O3S_ERR_HIP;
  }
  auto one = [&](int32_t k, hipStream_t s) {
    if (n_overlaps) n_overlaps[2 * k] = n_overlaps[2 * k + 1] = 0;
    if (sources[k]->n == 0 || targets[k]->n == 0) return (int)O3S_ERR_EMPTY_REFERENCE;
    if (est_type != kEstPoint && targets[k]->has_normals != 1) return (int)O3S_ERR_BAD_SHAPE;
    if (est_type == kEstGicp && sources[k]->has_normals != 1) return (int)O3S_ERR_BAD_SHAPE;
    return refine_overlap_on(sources[k], targets[k], max_dist, inits + 16 * (size_t)k, criteria, overlap_voxel_size, min_points_per_voxel, &results[k],
                             infos ? infos + 36 * (size_t)k : nullptr, n_overlaps ? n_overlaps + 2 * (size_t)k : nullptr, s, est_type, gicp_epsilon);
  };
  auto lane = [&](int l) {
    (void)hipSetDevice(device);
    for (int32_t k = l; k < n; k += lanes) statuses[k] = one(k, streams[(size_t)l]);
    (void)hipStreamSynchronize(streams[(size_t)l]);
  };
  std::vector<std::thread> pool;
  for (int l = 1; l < lanes; ++l) pool.emplace_back(lane, l);
  lane(0);
  for (auto& th : pool) th.join();
  for (int32_t k = 0; k < n; ++k)
    if (statuses[k] != O3S_OK && statuses[k] != O3S_ERR_EMPTY_REFERENCE) return statuses[k];
  return O3S_OK;
}
}  // namespace

extern "C" {

int o3s_o3d_registration_icp_submaps_overlap(const o3s_submap* source, const o3s_submap* target, double max_dist, const double init[16],
                                             const o3s_o3d_icp_criteria* criteria, double overlap_voxel_size, int64_t min_points_per_voxel,
                                             o3s_o3d_icp_result* result, double* info36, int64_t* n_overlap) {
  return refine_overlap_entry(source, target, max_dist, init, criteria, overlap_voxel_size, min_points_per_voxel, result, info36, n_overlap,
                              o3s_cloud::kEstPlane, 1e-3);
}

int o3s_o3d_registration_icp_submaps_overlap_ex(const o3s_submap* source, const o3s_submap* target, double max_dist, const double init[16],
                                                const o3s_o3d_estimation* est, const o3s_o3d_icp_criteria* criteria, double overlap_voxel_size,
                                                int64_t min_points_per_voxel, o3s_o3d_icp_result* result, double* info36, int64_t* n_overlap) {
  if (!o3d_est_valid(est)) return O3S_ERR_BAD_ARGUMENT;
  return refine_overlap_entry(source, target, max_dist, init, criteria, overlap_voxel_size, min_points_per_voxel, result, info36, n_overlap, est->type,
                              est->gicp_epsilon);
}

int o3s_o3d_registration_icp_submaps_overlap_batch(int32_t n, const o3s_submap* const* sources, const o3s_submap* const* targets, double max_dist,
                                                   const double* inits, const o3s_o3d_icp_criteria* criteria, double overlap_voxel_size,
                                                   int64_t min_points_per_voxel, o3s_o3d_icp_result* results, double* infos, int64_t* n_overlaps,
                                                   int32_t* statuses) {
  return refine_overlap_batch(n, sources, targets, max_dist, inits, criteria, overlap_voxel_size, min_points_per_voxel, results, infos, n_overlaps,
                              statuses, o3s_cloud::kEstPlane, 1e-3);
}

int o3s_o3d_registration_icp_submaps_overlap_batch_ex(int32_t n, const o3s_submap* const* sources, const o3s_submap* const* targets, double max_dist,
                                                      const double* inits, const o3s_o3d_estimation* est, const o3s_o3d_icp_criteria* criteria,
                                                      double overlap_voxel_size, int64_t min_points_per_voxel, o3s_o3d_icp_result* results,
                                                      double* infos, int64_t* n_overlaps, int32_t* statuses) {
  if (!o3d_est_valid(est)) return O3S_ERR_BAD_ARGUMENT;
  return refine_overlap_batch(n, sources, targets, max_dist, inits, criteria, overlap_voxel_size, min_points_per_voxel, results, infos, n_overlaps,
                              statuses, est->type, est->gicp_epsilon);
}

}  // extern "C"

// ---- occupancy snapshot of a resident submap and the overlap fitness (include/o3s_submap.h) ---------------------------------------
// Submap::voxelMap_ as the revisit check reads it (Submap.cpp:260-264, SubmapCollection.cpp:392-407): only WHETHER a voxel holds a
// map point matters, so the snapshot is a key-only open-addressing table (voxel_table.h: vm_claim, vm_find) that stays in
// HBM with the submap.  Keys are vm_key's, the arithmetic of k_ov_keys.
namespace {
namespace o3s_cloud {

// Inserts the voxel of every point.  The lanes of a wave that share the voxel of its first lane are served by that lane (a map in
// voxel order: whole waves fall into one voxel and make one compare-and-swap); every other lane inserts its own key, all of them at
// once (serving one distinct key after the other, as k_ov_count does for its per-voxel counts, was 64 dependent round trips per wave
// on a map in any other order: 2 ms for 0.4 M points).  cnt[0] += voxels this launch made, cnt[1] = 1 when a key found no slot
// within max_probe steps (the table is too small: the host repeats the build with room for one voxel per point at half load).
__global__ void __launch_bounds__(kB) k_vm_insert(const double* __restrict__ pts, int64_t N, double inv, unsigned long long* __restrict__ tab,
                                                  uint32_t mask, uint32_t max_probe, uint32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const uint64_t k = i < N ? vm_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], inv) : kDmEmpty;
  bool pending = k != kDmEmpty;
  const unsigned long long open = __ballot(pending);
  if (!open) return;  // (uniform)
  const int leader = __ffsll((long long)open) - 1;
  const uint64_t lk = wave_bcast_u64(k, leader);
  if (lane != leader && k == lk) pending = false;
  if (!pending) return;
  const VmClaim c = vm_claim(k, tab, mask, max_probe);
  if (c == kVmMade) atomicAdd(&cnt[0], 1u);  // exactly one lane of the whole launch makes a voxel's entry
  if (c == kVmFull) cnt[1] = 1u;
}

// p' = R p + t as an isometry product — fp64, no FMA (the TU is compiled with -ffp-contract=off), ((R0 x + R1 y) + R2 z) + t — then
// key, then lookup.  One ballot per wave, one integer add per wave: the total does not depend on any order.
struct Iso3d {
  double r[9];  // row-major
  double t[3];
};
__global__ void __launch_bounds__(kB) k_vm_count(const double* __restrict__ pts, int64_t N, Iso3d T, double inv,
                                                 const unsigned long long* __restrict__ tab, uint32_t mask, uint32_t* __restrict__ total) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  bool hit = false;
  if (i < N) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    double q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double s = T.r[3 * a] * x;
      s = s + T.r[3 * a + 1] * y;
      s = s + T.r[3 * a + 2] * z;
      q[a] = s + T.t[a];
    }
    const uint64_t k = vm_key(q[0], q[1], q[2], inv);
    hit = k != kDmEmpty && vm_find(k, tab, mask);
  }
  const unsigned long long b = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(total, (uint32_t)__popcll(b));
}
// hands `n` counter words to the host (host_post.h)
__global__ void __launch_bounds__(64) k_vm_post(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ mailbox, uint32_t seq) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t v[2] = {cnt[0], cnt[1]};
  post(mailbox, seq, kPostVals, v);
}
inline int vm_fetch(const uint32_t* d_cnt, uint32_t out[2], hipStream_t s) {
  PinnedArea& pa = pinned_area();
  const uint32_t seq = mailbox_open(pa);
  if (seq) {
    hipLaunchKernelGGL(k_vm_post, dim3(1), dim3(64), 0, s, d_cnt, pa.mb.dev, seq);
    CK(hipGetLastError());
  }
  return fetch_post(pa.mb, seq, s, out, 2, kPostVals, d_cnt, pinned_words()) == kPollError ? O3S_ERR_HIP : O3S_OK;
}
// The count's total lives in a word of the CALLING THREAD's own (per device; 16 bytes, made on first use and never freed: a
// thread_local destructor could run behind the runtime's own exit): the submap is const here, and two threads that count against
// one snapshot at the same time — the mapping thread's revisit check, a worker's — must not share a counter.
inline uint32_t* vm_thread_counter(int device) {
  static thread_local std::vector<uint32_t*> per_device;
  if ((size_t)device >= per_device.size()) per_device.resize((size_t)device + 1, nullptr);
  if (!per_device[(size_t)device] && hipMalloc(reinterpret_cast<void**>(&per_device[(size_t)device]), 16) != hipSuccess) per_device[(size_t)device] = nullptr;
  return per_device[(size_t)device];
}
constexpr uint32_t kVmMaxProbe = 256;  // a first-size table that makes a key walk further is given up for the full-size one

// counts the points of a device cloud that fall into an occupied voxel of m's snapshot; everything is enqueued on m's stream
int vm_count_dev(const o3s_submap* m, const double* d_pts, int64_t N, const double* T, int64_t* n_overlapping) {
  hipStream_t s = m->stream;
  Iso3d iso;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) iso.r[3 * r + c] = T[4 * c + r];
    iso.t[r] = T[12 + r];
  }
  uint32_t* d_total = vm_thread_counter(m->device);  // (the device is current: set_dev)
  if (!d_total) return O3S_ERR_HIP;
  CK(hipMemsetAsync(d_total, 0, 8, s));
  hipLaunchKernelGGL(k_vm_count, dim3(nblk(N)), dim3(kB), 0, s, d_pts, N, iso, 1.0 / m->vox_size,
                     reinterpret_cast<const unsigned long long*>(m->vox_tab.p), m->vox_slots - 1u, d_total);
  CK(hipGetLastError());
  uint32_t r[2] = {0, 0};
  const int rc = vm_fetch(d_total, r, s);
  if (rc != O3S_OK) return rc;
  *n_overlapping = (int64_t)r[0];
  return O3S_OK;
}
// the shared front of the two entry points: 1 = answered without the device (no points, or no snapshot), 0 = count, else an error
int vm_count_front(const o3s_submap* m, int64_t N, const double* T, int64_t* n_overlapping, double* fitness) {
  if (!m || !T || !n_overlapping || !fitness || N < 0 || N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(T[k])) return O3S_ERR_BAD_ARGUMENT;
  *n_overlapping = 0;
  // static_cast<double>(numOverlappingPoints) / scan.points_.size(): 0 / 0 for an empty scan, 0 / N over an empty voxel map
  *fitness = N == 0 ? std::numeric_limits<double>::quiet_NaN() : 0.0;
  return (N == 0 || m->n_vox <= 0) ? 1 : 0;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_submap_build_voxel_map(o3s_submap* m, double voxel_size) {
  using namespace o3s_cloud;
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !(voxel_size > 0.0) || !std::isfinite(voxel_size)) return O3S_ERR_BAD_ARGUMENT;
  if (m->n > (int64_t)0x3fffffff) return O3S_ERR_BAD_ARGUMENT;
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const uint32_t full = ov_slots_for(m->n);
  // the first table: 2^16 slots, or room for one voxel per four points at half load when that is more (a 0.4 M-point map at
  // 2.5 x its voxel size holds 77 k voxels: a first table they do not fit is filled to its probe limit and thrown away — 0.9 ms)
  uint32_t slots = std::min(std::max(kOvFirstSlots, ov_slots_for(m->n / 4)), full);
  m->n_vox = -1;  // (a failed build leaves no snapshot)
  for (;;) {
    CK(m->vox_tab.ensure(((size_t)slots + 1) * 8, 0, s));
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(m->vox_tab.p);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(tab + slots);
    CK(hipMemsetAsync(tab, 0, ((size_t)slots + 1) * 8, s));
    uint32_t r[2] = {0, 0};
    if (m->n > 0) {
      // the full-size table holds at most one voxel per point at half load: every key finds a slot
      hipLaunchKernelGGL(k_vm_insert, dim3(nblk(m->n)), dim3(kB), 0, s, (const double*)m->pts[m->cur].as<double>(), m->n, 1.0 / voxel_size, tab, slots - 1u,
                         slots == full ? slots : std::min(slots, kVmMaxProbe), cnt);
      CK(hipGetLastError());
      if (const int rf = vm_fetch(cnt, r, s); rf != O3S_OK) return rf;
    }
    // the first table filled up, or past half load (lookups of absent keys would walk long runs): once more at full size
    if ((r[1] || 2 * (uint64_t)r[0] > slots) && slots < full) {
      slots = full;
      continue;
    }
    if (r[1]) return O3S_ERR_HIP;
    m->vox_slots = slots;
    m->vox_size = voxel_size;
    m->n_vox = (int64_t)r[0];
    return O3S_OK;
  }
}

int64_t o3s_submap_voxel_map_size(const o3s_submap* m) { return m ? m->n_vox : -1; }

int o3s_submap_overlap_fitness(const o3s_submap* m, const double* pts, int64_t N, const double T_map_sensor[16], int64_t* n_overlapping,
                               double* fitness) {
  using namespace o3s_cloud;
  const int f = vm_count_front(m, N, T_map_sensor, n_overlapping, fitness);
  if (f != 0) return f == 1 ? O3S_OK : f;
  if (!pts) return O3S_ERR_BAD_ARGUMENT;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  DevMem d_p;
  CK(d_p.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, m->stream));
  rc = vm_count_dev(m, d_p.as<double>(), N, T_map_sensor, n_overlapping);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(m->stream));  // (the post may be ahead of the kernel's retirement: the buffer goes now)
  *fitness = (double)*n_overlapping / (double)N;
  return O3S_OK;
}

int o3s_submap_overlap_fitness_scan(const o3s_submap* m, const o3s_scan* scan, int which, const double T_map_sensor[16], int64_t* n_overlapping,
                                    double* fitness) {
  using namespace o3s_cloud;
  if (!scan || (which != 0 && which != 1)) return O3S_ERR_BAD_ARGUMENT;
  const int64_t N = which == 0 ? scan->n_wide : scan->n_narrow;
  const int f = vm_count_front(m, N, T_map_sensor, n_overlapping, fitness);
  if (f != 0) return f == 1 ? O3S_OK : f;
  if (m->device != scan->device) return O3S_ERR_BAD_ARGUMENT;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  if (scan->stream != m->stream) {  // the scan's clouds are complete before the count reads them
    CK(hipEventRecord(scan->handover, scan->stream));
    CK(hipStreamWaitEvent(m->stream, scan->handover, 0));
  }
  rc = vm_count_dev(m, (which == 0 ? scan->wide_p : scan->narrow_p).as<double>(), N, T_map_sensor, n_overlapping);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(m->stream));  // the scan may be refilled when this returns
  *fitness = (double)*n_overlapping / (double)N;
  return O3S_OK;
}

}  // extern "C"
