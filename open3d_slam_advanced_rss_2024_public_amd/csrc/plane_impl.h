// plane_impl.h — host side and C entry points of the RANSAC plane segmentation (include/plane_segmentation/o3s_plane_segmentation.h).
// Included at the end of cloud_ops.hip behind cluster_impl.h, whose resident removal paths it shares; the kernels are in plane_dev.h.
#pragma once
#include "plane_dev.h"
#include "cluster_impl.h"

#include <atomic>

namespace {
namespace o3s_cloud {

// work area of one call over a cloud of n points with `batch` hypotheses in flight; n_peel = n when planes are peeled, else 0
struct PlaneArea {
  static constexpr size_t kSlack = 4096;
  PlaneHeader* hdr;
  int32_t* outcome;
  double *planes, *part_e, *sv_e, *lpts, *rpart, *cloud[2];
  uint32_t *part_n, *sv_n, *iflag, *ioff, *orig[2], *keep, *koff;
  int32_t* labels;
  char* tmp;
  template <class A>
  void lay(A& a, size_t n, size_t batch, size_t chunks, size_t n_peel, size_t tb_scan) {
    take(a, hdr, 1);
    take(a, outcome, batch);
    take(a, planes, batch * 4);
    take(a, part_n, batch * chunks);
    take(a, part_e, batch * chunks);
    take(a, sv_n, batch);
    take(a, sv_e, batch);
    take(a, iflag, n);
    take(a, ioff, n + 1);
    take(a, lpts, n * 3);
    take(a, rpart, chunks * 6);
    take(a, cloud[0], n_peel * 3);
    take(a, cloud[1], n_peel * 3);
    take(a, orig[0], n_peel);
    take(a, orig[1], n_peel);
    take(a, labels, n);
    take(a, keep, n);
    take(a, koff, n + 1);
    take(a, tmp, tb_scan);
  }
};

struct PlaneWork {  // grow-only, leased per call from the device's pool
  Arena arena;
  DevMem in_p, table, out_i;  // staging of the host-array entries
  size_t bytes() const { return arena.mem.cap + in_p.cap + table.cap + out_i.cap; }
};
constexpr int kPlDevices = 64;
inline std::atomic<long long>& plane_bytes_of(int device) {  // what the area that served the last call on `device` holds
  static std::atomic<long long> held[kPlDevices];
  return held[device >= 0 && device < kPlDevices ? device : 0];
}
struct PlaneLease : AreaLease<PlaneWork, /*kAlwaysDrain=*/true> {  // every exit hands the area back behind a drained stream
  using AreaLease::AreaLease;
  ~PlaneLease() { plane_bytes_of(device).store((long long)a->bytes()); }
};

inline int plane_batch() {  // a constant in the product; the hooks build reads it per call (one test, several batch sizes)
  if (const char* e = O3S_HOOK_ENV("O3S_PLANE_BATCH")) {
    const long v = atol(e);
    if (v >= 1 && v <= (1 << 20)) return (int)v;
  }
  return kPlBatch;
}
inline int plane_eval_block(int count) {
  if (const char* e = O3S_HOOK_ENV("O3S_PLANE_EVAL_BLOCK")) {
    const long v = atol(e);
    if (v == 64 || v == 128 || v == 256) return (int)v;
  }
  return count >= kPlEvalBlockMax ? kPlEvalBlockMax : kPlEvalBlock;  // a full block of four waves shares one staged chunk
}
inline int plane_chunks(int64_t M) { return (int)((std::max<int64_t>(M, 1) + kPlChunk - 1) / kPlChunk); }
// the batch a call runs with: never more than the iterations asked for, and batch x chunks partial sums bounded (2^24 of each, 192 MB)
inline int plane_eff_batch(int batch, int64_t n_iter, int64_t N) {
  const int64_t cap = std::max<int64_t>(64, ((int64_t)1 << 24) / plane_chunks(N));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(batch, n_iter), cap));
}

inline bool plane_params_valid(const o3s_plane_params* p) {  // (num_iterations 0 is the caller's: it returns before this)
  return p && p->distance_threshold > 0.0 && std::isfinite(p->distance_threshold) && p->confidence > 0.0 && p->confidence <= 1.0 && p->num_iterations > 0 &&
         p->ransac_n >= 3 && p->ransac_n <= kPlNMax && p->max_planes >= 1 && p->max_planes <= 16 && p->min_inliers >= 0;
}
inline bool plane_table_in_range(const int32_t* t, int64_t words, int64_t N) {
  for (int64_t k = 0; k < words; ++k)
    if (t[k] < 0 || t[k] >= N) return false;
  return true;
}
inline PlaneArgs plane_args(const o3s_plane_params* p, uint32_t k, int64_t M) {
  PlaneArgs a;
  a.n = p->ransac_n;
  a.k = k;
  a.thr = p->distance_threshold;
  a.confidence = p->confidence;
  a.seed = p->seed;
  a.M = M;
  return a;
}
inline int plane_lay_out(PlaneWork& w, PlaneArea& a, int64_t N, int batch, bool peel, size_t* tb) {
  *tb = scan_temp_bytes(std::max<int64_t>(N, 1));
  CK(lay_out(w.arena, a, (size_t)N, (size_t)batch, (size_t)plane_chunks(N), peel ? (size_t)N : (size_t)0, *tb));
  return O3S_OK;
}

// hypotheses [itr0, itr0 + count) up to the folded sums per slot; `hdr` nullable (o3s_plane_evaluate_samples: no early end)
inline int plane_issue_batch(PlaneArea& a, const PlaneArgs& g, const double* d_pts, const int32_t* d_table, int64_t itr0, int count, const PlaneHeader* hdr,
                             hipStream_t s) {
  const int chunks = plane_chunks(g.M), eb = plane_eval_block(count);
  hipLaunchKernelGGL(k_pl_hyp, dim3(nblk(count)), dim3(kB), 0, s, g, d_pts, d_table, (long long)itr0, count, hdr, a.outcome, a.planes);
  hipLaunchKernelGGL(k_pl_eval, dim3((unsigned)chunks, (unsigned)((count + eb - 1) / eb)), dim3(eb), 0, s, d_pts, (long long)g.M, g.thr, (long long)itr0, hdr, count,
                     (const double*)a.planes, a.part_n, a.part_e);
  hipLaunchKernelGGL(k_pl_fold, dim3((unsigned)((count + kPlFoldBlock - 1) / kPlFoldBlock)), dim3(kPlFoldBlock), 0, s, (long long)itr0, hdr, count, chunks, (const int32_t*)a.outcome, (const uint32_t*)a.part_n,
                     (const double*)a.part_e, a.sv_n, a.sv_e);
  CK(hipGetLastError());
  return O3S_OK;
}

// One segmentation of d_pts (M points on the device): the batches, the winner's inlier list (a.iflag / a.ioff / a.lpts) and its refit;
// *h: the header, on a drained stream.  With confidence 1 nothing is read back before that; below 1 the host looks at est_k every
// kPlLook batches — what it has not seen yet costs launches that return at once, never a different result.
inline int plane_one_dev(PlaneArea& a, size_t tb, const o3s_plane_params* p, uint32_t k, const double* d_pts, int64_t M, const int32_t* d_table, int64_t n_iter,
                         int batch, PlaneHeader* h, hipStream_t s) {
  *h = PlaneHeader{};
  h->est_k = n_iter;
  h->best_itr = -1;
  if (M < p->ransac_n || n_iter <= 0) return O3S_OK;
  const PlaneArgs g = plane_args(p, k, M);
  hipLaunchKernelGGL(k_pl_init, dim3(1), dim3(64), 0, s, a.hdr, (long long)n_iter);
  int64_t b = 0;
  for (int64_t itr0 = 0; itr0 < n_iter; itr0 += batch, ++b) {
    if (p->confidence < 1.0 && b > 0 && b % kPlLook == 0) {
      long long est_k = 0;
      CK(hipMemcpyAsync(&est_k, &a.hdr->est_k, 8, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      if (itr0 >= est_k) break;
    }
    const int count = (int)std::min<int64_t>(batch, n_iter - itr0);
    const int rc = plane_issue_batch(a, g, d_pts, d_table, itr0, count, a.hdr, s);
    if (rc != O3S_OK) return rc;
    hipLaunchKernelGGL(k_pl_select, dim3(1), dim3(64), 0, s, g, a.hdr, (long long)itr0, count, (const int32_t*)a.outcome, (const uint32_t*)a.sv_n,
                       (const double*)a.sv_e, (const double*)a.planes);
  }
  uint32_t* blk = reinterpret_cast<uint32_t*>(a.tmp);
  hipLaunchKernelGGL(k_pl_inlier_flags, dim3(nblk(M)), dim3(kB), 0, s, d_pts, (long long)M, g.thr, (const PlaneHeader*)a.hdr, a.iflag, blk);
  CK(hipGetLastError());
  const int rc = scan_flags_dev(a.iflag, a.ioff, M, a.tmp, tb, s, blk);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_pl_list_total, dim3(1), dim3(64), 0, s, (const uint32_t*)a.iflag, a.ioff, (long long)M, a.hdr);
  hipLaunchKernelGGL(k_compact, dim3(nblk(M)), dim3(kB), 0, s, d_pts, (const double*)nullptr, M, (const uint32_t*)a.iflag, (const uint32_t*)a.ioff, a.lpts,
                     (double*)nullptr, (int32_t*)nullptr);
  const dim3 gp((unsigned)plane_chunks(M));  // a block per chunk of the list, which is no longer than the cloud
  hipLaunchKernelGGL(k_pl_refit_part<false>, gp, dim3(64), 0, s, (const double*)a.lpts, (const PlaneHeader*)a.hdr, a.rpart);
  hipLaunchKernelGGL(k_pl_refit_fold<false>, dim3(1), dim3(64), 0, s, (const double*)a.rpart, a.hdr);
  hipLaunchKernelGGL(k_pl_refit_part<true>, gp, dim3(64), 0, s, (const double*)a.lpts, (const PlaneHeader*)a.hdr, a.rpart);
  hipLaunchKernelGGL(k_pl_refit_fold<true>, dim3(1), dim3(64), 0, s, (const double*)a.rpart, a.hdr);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(h, a.hdr, sizeof(PlaneHeader), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (h->best_itr >= 0 && h->n_list != h->n_in) return O3S_ERR_HIP;  // the list and the count come from the same arithmetic
  return O3S_OK;
}

struct PlanePeel {
  int n_planes = 0;
  double models[16 * 4];
  int64_t counts[16];
  PlaneHeader first;  // the header of plane 0 (o3s_segment_plane reports it)
};

// The peel on d_pts (N > 0 points on the device): up to max_planes segmentations, each of what the planes before left, compacted on
// the device.  label: a.labels gets the plane of every point (-1: none).  The area keeps the last plane's inlier list.
inline int plane_peel_dev(PlaneWork& w, PlaneArea& a, const o3s_plane_params* p, const double* d_pts, int64_t N, const int32_t* d_table, int64_t n_table,
                          int max_planes, int min_inliers, bool label, PlanePeel* out, hipStream_t s) {
  const int64_t n_iter = d_table ? std::min<int64_t>(p->num_iterations, n_table) : (int64_t)p->num_iterations;
  const int batch = plane_eff_batch(plane_batch(), n_iter, N);
  size_t tb = 0;
  int rc = plane_lay_out(w, a, N, batch, max_planes > 1, &tb);
  if (rc != O3S_OK) return rc;
  if (label) CK(hipMemsetAsync(a.labels, 0xff, (size_t)N * 4, s));  // -1
  const double* cur = d_pts;
  const uint32_t* orig = nullptr;
  int64_t M = N;
  out->n_planes = 0;
  for (int k = 0; k < max_planes; ++k) {
    PlaneHeader h;
    rc = plane_one_dev(a, tb, p, (uint32_t)k, cur, M, d_table, n_iter, batch, &h, s);
    if (rc != O3S_OK) return rc;
    if (k == 0) out->first = h;
    if (h.best_itr < 0 || h.n_list < (long long)min_inliers) break;
    for (int c = 0; c < 4; ++c) out->models[4 * k + c] = h.model[c];
    out->counts[k] = h.n_list;
    out->n_planes = k + 1;
    const bool last = k + 1 == max_planes;
    if (label || !last) {
      hipLaunchKernelGGL(k_pl_peel, dim3(nblk(M)), dim3(kB), 0, s, cur, orig, (long long)M, (const uint32_t*)a.iflag, (const uint32_t*)a.ioff, (int32_t)k,
                         label ? a.labels : (int32_t*)nullptr, last ? (double*)nullptr : a.cloud[k & 1], last ? (uint32_t*)nullptr : a.orig[k & 1]);
      CK(hipGetLastError());
    }
    cur = a.cloud[k & 1];
    orig = a.orig[k & 1];
    M -= h.n_list;
  }
  return O3S_OK;
}

// the peel, then keep = "no plane took the point" with its scan: what the three removal entries compact by
inline int plane_keep_dev(PlaneWork& w, PlaneArea& a, const o3s_plane_params* p, const double* d_pts, int64_t N, PlanePeel* out, int64_t* n_keep, hipStream_t s) {
  int rc = plane_peel_dev(w, a, p, d_pts, N, nullptr, 0, p->max_planes, p->min_inliers, /*label=*/true, out, s);
  if (rc != O3S_OK) return rc;
  uint32_t* blk = reinterpret_cast<uint32_t*>(a.tmp);
  hipLaunchKernelGGL(k_pl_keep, dim3(nblk(N)), dim3(kB), 0, s, (const int32_t*)a.labels, (long long)N, a.keep, blk);
  CK(hipGetLastError());
  return scan_flags(a.keep, a.koff, N, a.tmp, scan_temp_bytes(N), n_keep, s, blk);
}
inline void plane_models_out(const PlanePeel& r, int32_t* n_planes, double* models, int64_t* counts) {
  if (n_planes) *n_planes = r.n_planes;
  for (int k = 0; k < r.n_planes; ++k) {
    if (models)
      for (int c = 0; c < 4; ++c) models[4 * k + c] = r.models[4 * k + c];
    if (counts) counts[k] = r.counts[k];
  }
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

void o3s_plane_default_params(o3s_plane_params* p) {
  if (!p) return;
  p->distance_threshold = 0.0;
  p->confidence = 1.0;
  p->seed = 0;
  p->num_iterations = 100;
  p->ransac_n = 3;
  p->max_planes = 1;
  p->min_inliers = 3;
}

int o3s_plane_reserve(int device, int64_t max_points, int32_t num_iterations) {
  if (max_points < 0 || max_points > (int64_t)0x7fffffff || num_iterations < 0) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  PlaneLease w(device);
  PlaneArea a;
  size_t tb = 0;
  CK(w->in_p.alloc((size_t)max_points * 24));
  CK(w->out_i.alloc((size_t)max_points * 8));
  return plane_lay_out(*w, a, max_points, plane_eff_batch(plane_batch(), std::max<int64_t>(num_iterations, 1), max_points), /*peel=*/true, &tb);
}

int o3s_plane_release(int device) {
  const int rc = release_idle_areas<PlaneWork>(device);
  if (rc == O3S_OK) plane_bytes_of(device).store(0);
  return rc;
}

int64_t o3s_plane_device_bytes(int device) { return device >= 0 && device < kPlDevices ? (int64_t)plane_bytes_of(device).load() : 0; }

int o3s_segment_plane(int device, const o3s_plane_params* p, const double* pts, int64_t N, const int32_t* samples, int64_t n_samples, double model[4],
                      int64_t* inlier_indices, int64_t* n_inliers, int64_t* best_iteration, int64_t* est_k, int64_t* evaluated) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->num_iterations == 0) return O3S_OK;
  if (!plane_params_valid(p) || !model || N < 0 || N > (int64_t)0x7fffffff || (N > 0 && !pts) || (samples && (n_samples < 0 || p->max_planes > 1)))
    return O3S_ERR_BAD_ARGUMENT;
  const int64_t n_iter = samples ? std::min<int64_t>(p->num_iterations, n_samples) : (int64_t)p->num_iterations;
  if (samples && !plane_table_in_range(samples, n_iter * p->ransac_n, N)) return O3S_ERR_BAD_ARGUMENT;
  model[0] = model[1] = model[2] = model[3] = 0.0;
  if (n_inliers) *n_inliers = 0;
  if (best_iteration) *best_iteration = -1;
  if (est_k) *est_k = n_iter;
  if (evaluated) *evaluated = 0;
  if (N < p->ransac_n || n_iter == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  PlaneLease w(device, s);
  CK(w->in_p.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(w->in_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (samples) {
    CK(w->table.alloc((size_t)n_iter * p->ransac_n * 4));
    CK(hipMemcpyAsync(w->table.p, samples, (size_t)n_iter * p->ransac_n * 4, hipMemcpyHostToDevice, s));
  }
  if (inlier_indices) CK(w->out_i.alloc((size_t)N * 8));
  PlaneArea a;
  PlanePeel r;
  rc = plane_peel_dev(*w, a, p, w->in_p.as<double>(), N, samples ? w->table.as<int32_t>() : nullptr, n_iter, /*max_planes=*/1, /*min_inliers=*/0, /*label=*/false, &r, s);
  if (rc != O3S_OK) return rc;
  const PlaneHeader& h = r.first;
  if (est_k) *est_k = h.est_k;
  if (evaluated) *evaluated = h.evaluated;
  if (h.best_itr < 0) return O3S_OK;
  if (inlier_indices && h.n_list) {
    hipLaunchKernelGGL(k_or_kept_idx, dim3(nblk(N)), dim3(kB), 0, s, (const uint32_t*)a.iflag, (const uint32_t*)a.ioff, N, w->out_i.as<int64_t>());
    CK(hipGetLastError());
    CK(hipMemcpyAsync(inlier_indices, w->out_i.p, (size_t)h.n_list * 8, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
  }
  for (int c = 0; c < 4; ++c) model[c] = h.model[c];
  if (n_inliers) *n_inliers = h.n_list;
  if (best_iteration) *best_iteration = h.best_itr;
  return O3S_OK;
}

int o3s_segment_planes(int device, const o3s_plane_params* p, const double* pts, int64_t N, int32_t* labels, int32_t* n_planes, double* models, int64_t* counts) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->num_iterations == 0) return O3S_OK;
  if (!plane_params_valid(p) || !n_planes || !models || N < 0 || N > (int64_t)0x7fffffff || (N > 0 && (!pts || !labels))) return O3S_ERR_BAD_ARGUMENT;
  *n_planes = 0;
  if (N < p->ransac_n) {  // no sample can be drawn: no plane takes a point
    for (int64_t i = 0; i < N; ++i) labels[i] = -1;
    return O3S_OK;
  }
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  PlaneLease w(device, s);
  CK(w->in_p.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(w->in_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  PlaneArea a;
  PlanePeel r;
  rc = plane_peel_dev(*w, a, p, w->in_p.as<double>(), N, nullptr, 0, p->max_planes, p->min_inliers, /*label=*/true, &r, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(labels, a.labels, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  plane_models_out(r, n_planes, models, counts);
  return O3S_OK;
}

int o3s_plane_evaluate_samples(int device, const o3s_plane_params* p, const double* pts, int64_t N, const int32_t* samples, int64_t first_iteration, int64_t count,
                               int32_t* outcome, double* planes, int64_t* n_in, double* err) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->num_iterations == 0) return O3S_OK;
  if (!plane_params_valid(p) || !pts || !outcome || N < p->ransac_n || N > (int64_t)0x7fffffff || count < 0 || first_iteration < 0 ||
      (samples && (first_iteration != 0 || p->max_planes > 1)))
    return O3S_ERR_BAD_ARGUMENT;
  if (samples && !plane_table_in_range(samples, count * p->ransac_n, N)) return O3S_ERR_BAD_ARGUMENT;
  if (count == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  PlaneLease w(device, s);
  CK(w->in_p.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(w->in_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (samples) {
    CK(w->table.alloc((size_t)count * p->ransac_n * 4));
    CK(hipMemcpyAsync(w->table.p, samples, (size_t)count * p->ransac_n * 4, hipMemcpyHostToDevice, s));
  }
  const int batch = plane_eff_batch(plane_batch(), count, N);
  PlaneArea a;
  size_t tb = 0;
  rc = plane_lay_out(*w, a, N, batch, /*peel=*/false, &tb);
  if (rc != O3S_OK) return rc;
  const PlaneArgs g = plane_args(p, 0u, N);
  std::vector<uint32_t> n32((size_t)batch);
  for (int64_t done = 0; done < count; done += batch) {
    const int c = (int)std::min<int64_t>(batch, count - done);
    rc = plane_issue_batch(a, g, w->in_p.as<double>(), samples ? w->table.as<int32_t>() : nullptr, first_iteration + done, c, nullptr, s);
    if (rc != O3S_OK) return rc;
    CK(hipMemcpyAsync(outcome + done, a.outcome, (size_t)c * 4, hipMemcpyDeviceToHost, s));
    if (planes) CK(hipMemcpyAsync(planes + 4 * done, a.planes, (size_t)c * 32, hipMemcpyDeviceToHost, s));
    if (n_in) CK(hipMemcpyAsync(n32.data(), a.sv_n, (size_t)c * 4, hipMemcpyDeviceToHost, s));
    if (err) CK(hipMemcpyAsync(err + done, a.sv_e, (size_t)c * 8, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (n_in)
      for (int i = 0; i < c; ++i) n_in[done + i] = (int64_t)n32[(size_t)i];
  }
  return O3S_OK;
}

int o3s_submap_segment_planes(o3s_submap* m, const o3s_plane_params* p, int32_t* labels, int32_t* n_planes, double* models, int64_t* counts) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->num_iterations == 0) return O3S_OK;
  if (!plane_params_valid(p) || !n_planes || !models) return O3S_ERR_BAD_ARGUMENT;
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  *n_planes = 0;
  if (m->n == 0) return O3S_OK;
  if (!labels) return O3S_ERR_BAD_ARGUMENT;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  PlaneLease w(m->device, s);
  PlaneArea a;
  PlanePeel r;
  rc = plane_peel_dev(*w, a, p, m->pts[m->cur].as<double>(), m->n, nullptr, 0, p->max_planes, p->min_inliers, /*label=*/true, &r, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(labels, a.labels, (size_t)m->n * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  plane_models_out(r, n_planes, models, counts);
  return O3S_OK;
}

int o3s_submap_remove_planes(o3s_submap* m, const o3s_plane_params* p, int64_t* n_removed, int32_t* n_planes, double* models) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->num_iterations == 0) return O3S_OK;
  if (!plane_params_valid(p)) return O3S_ERR_BAD_ARGUMENT;
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (n_removed) *n_removed = 0;
  if (n_planes) *n_planes = 0;
  if (m->n == 0) return O3S_OK;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const int64_t Nm = m->n;
  PlaneLease w(m->device, s);
  PlaneArea a;
  PlanePeel r;
  int64_t n_keep = 0;
  rc = plane_keep_dev(*w, a, p, m->pts[m->cur].as<double>(), Nm, &r, &n_keep, s);
  if (rc != O3S_OK) return rc;
  rc = submap_keep_flagged(m, a.keep, a.koff, n_keep);  // the path carving removes by
  if (rc != O3S_OK) return rc;
  if (n_removed) *n_removed = Nm - n_keep;
  plane_models_out(r, n_planes, models, nullptr);
  return O3S_OK;
}

int o3s_scan_remove_planes(o3s_scan* sc, const o3s_cropper* scan_matcher_cropper, const o3s_plane_params* p, int64_t* n_merge, int64_t* n_match, int32_t* n_planes,
                           double* models) {
  if (!sc || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->num_iterations == 0) return O3S_OK;
  if (!plane_params_valid(p) || !scan_matcher_cropper) return O3S_ERR_BAD_ARGUMENT;
  if (n_merge) *n_merge = sc->n_wide;
  if (n_match) *n_match = sc->n_narrow;
  if (n_planes) *n_planes = 0;
  if (sc->n_wide == 0) return O3S_OK;
  if (hipSetDevice(sc->device) != hipSuccess) return O3S_ERR_HIP;
  hipStream_t s = sc->stream;
  int64_t n_keep = 0;
  {
    PlaneLease w(sc->device, s);
    PlaneArea a;
    PlanePeel r;
    int rc = plane_keep_dev(*w, a, p, sc->wide_p.as<double>(), sc->n_wide, &r, &n_keep, s);
    if (rc != O3S_OK) return rc;
    rc = scan_keep_flagged(sc, a.keep, a.koff, n_keep);
    if (rc != O3S_OK) return rc;
    plane_models_out(r, n_planes, models, nullptr);
  }
  return scan_recrop(sc, scan_matcher_cropper, n_keep, n_merge, n_match);
}

}  // extern "C"
