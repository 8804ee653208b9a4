// ransac_impl.h — host side and C entry points of the RANSAC registration (include/o3s_registration.h: o3s_registration_ransac_*,
// o3s_ransac_evaluate_samples; include/o3s_submap.h: o3s_submap_registration_ransac).  Included at the end of cloud_ops.hip after
// features_impl.h; the kernels are in ransac_dev.h.
#pragma once
#include "ransac_dev.h"
#include "features_impl.h"

#include <memory>

namespace {
namespace o3s_cloud {

// Grow-only work area of one RANSAC call: sized by the number of correspondences and the batch size, leased per call from a pool
// per device (o3s_ransac_reserve sizes one ahead of time), so that repeated closures do not allocate.
struct RansacWork {
  DevMem src, tgt, pairs, table, feat_pairs;  // staging of the host-buffer entries
  DevMem rec, hdr, flag, off, outcome, T, surv, part_n, part_e, sv_n, sv_e, scan_tmp, iflag, ioff, iout, slot_n, slot_e;
  PostBlock<> post;  // kRansacAhead slots of the common layout, one per batch in flight
  FeatNnWork nn;
  PlaceWork place;  // the one-to-many front end (place_impl.h)
  size_t scan_bytes = 0;
  RansacWork() = default;
  RansacWork(const RansacWork&) = delete;
  RansacWork& operator=(const RansacWork&) = delete;
  ~RansacWork() { post.release(); }  // only ever runs through o3s_ransac_release (the pool itself is never torn down)
};
using RansacLease = AreaLease<RansacWork, /*kAlwaysDrain=*/true>;  // every exit, an early error included, hands the area back behind a drained stream

inline int ransac_batch() {  // a constant in the product; the hooks build reads it per call (one test, several batch sizes)
  if (const char* e = O3S_HOOK_ENV("O3S_RANSAC_BATCH")) {
    const long v = atol(e);
    if (v >= 1 && v <= (1 << 20)) return (int)v;
  }
  return kRansacBatch;
}
inline int ransac_chunks(int64_t K) { return (int)((K + kRansacChunk - 1) / kRansacChunk); }

inline int ransac_size_work(RansacWork& w, int64_t K, int batch) {
  const size_t b = (size_t)batch, c = (size_t)ransac_chunks(std::max<int64_t>(K, 1));
  const size_t n_scan = std::max<size_t>(b, (size_t)K) + 1;
  CK(w.rec.alloc((size_t)K * 48));
  CK(w.hdr.alloc(sizeof(RansacHeader)));
  CK(w.flag.alloc((b + 1) * 4));
  CK(w.off.alloc((b + 1) * 4));
  CK(w.outcome.alloc(b * 4));
  CK(w.T.alloc(b * 96));
  CK(w.surv.alloc(b * 4));
  CK(w.part_n.alloc(b * c * 4));
  CK(w.part_e.alloc(b * c * 8));
  CK(w.sv_n.alloc(b * 4));
  CK(w.sv_e.alloc(b * 8));
  CK(w.iflag.alloc(((size_t)K + 1) * 4));
  CK(w.ioff.alloc(((size_t)K + 1) * 4));
  CK(w.iout.alloc((size_t)K * 8));
  w.scan_bytes = scan_temp_bytes((int64_t)n_scan);
  CK(w.scan_tmp.alloc(w.scan_bytes));
  if (!w.post && w.post.alloc((size_t)kRansacAhead * kRansacSlotWords * 4) != hipSuccess) return O3S_ERR_HIP;
  return O3S_OK;
}

inline bool ransac_params_ok(const o3s_ransac_params* p) {
  return p && p->ransac_n <= kRansacNMax && p->max_iteration >= 0 && p->confidence >= 0.0 && p->confidence <= 1.0 &&
         std::isfinite(p->max_correspondence_distance) && !std::isnan(p->distance_threshold) && !std::isnan(p->edge_length_similarity);
}
// RegistrationRANSACBasedOnCorrespondence returns an empty RegistrationResult for these
inline bool ransac_trivial(const o3s_ransac_params* p, int64_t K) {
  return p->ransac_n < 3 || K < p->ransac_n || !(p->max_correspondence_distance > 0.0);
}
inline void ransac_empty_result(o3s_ransac_result* r, int64_t max_iteration) {
  for (int k = 0; k < 16; ++k) r->transformation[k] = (k % 5 == 0) ? 1.0 : 0.0;
  r->fitness = r->inlier_rmse = 0.0;
  r->correspondences = 0;
  r->best_iteration = -1;
  r->est_k = max_iteration;
  r->evaluated = 0;
}
inline RansacArgs ransac_args(const o3s_ransac_params* p, int64_t K) {
  RansacArgs a;
  a.n = p->ransac_n;
  a.check_edge = p->check_edge_length != 0;
  a.check_dist = p->check_distance != 0;
  a.sim = p->edge_length_similarity;
  a.thr = p->distance_threshold;
  a.max_dist = p->max_correspondence_distance;
  a.confidence = p->confidence;
  a.seed = p->seed;
  a.K = K;
  return a;
}

// header, records: what every path starts with
inline int ransac_prepare(RansacWork& w, const double* d_src, int64_t ns, const double* d_tgt, int64_t nt, const int32_t* d_pairs, int64_t K,
                          int64_t n_iter, hipStream_t s) {
  hipLaunchKernelGGL(k_ransac_init, dim3(1), dim3(64), 0, s, w.hdr.as<RansacHeader>(), (long long)n_iter);
  hipLaunchKernelGGL(k_ransac_gather, dim3(nblk(K)), dim3(kB), 0, s, d_src, (long long)ns, d_tgt, (long long)nt, d_pairs, (long long)K, w.rec.as<double>(),
                     w.hdr.as<RansacHeader>());
  CK(hipGetLastError());
  return O3S_OK;
}

// the kernels of one batch up to the folded per-survivor sums; `hdr` nullable (o3s_ransac_evaluate_samples: no early end)
inline int ransac_issue_batch(RansacWork& w, const RansacArgs& a, const int32_t* d_table, int64_t itr0, int count, int batch, const RansacHeader* hdr,
                              long long* slot_n, double* slot_e, hipStream_t s) {
  const int chunks = ransac_chunks(a.K);
  hipLaunchKernelGGL(k_ransac_hyp, dim3(nblk(count)), dim3(kB), 0, s, a, (const double*)w.rec.as<double>(), d_table, (long long)itr0, count, hdr,
                     w.flag.as<uint32_t>(), w.outcome.as<int32_t>(), w.T.as<double>());
  // flag[count] = 0 makes off[count] the number of survivors
  CK(hipMemsetAsync(w.flag.as<uint32_t>() + count, 0, 4, s));
  const int rc = scan_flags_dev(w.flag.as<uint32_t>(), w.off.as<uint32_t>(), (int64_t)count + 1, w.scan_tmp.p, w.scan_bytes, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_ransac_scatter, dim3(nblk(count)), dim3(kB), 0, s, (const uint32_t*)w.flag.as<uint32_t>(), (const uint32_t*)w.off.as<uint32_t>(), count,
                     (long long)itr0, hdr, w.surv.as<int32_t>());
  hipLaunchKernelGGL(k_ransac_eval, dim3((unsigned)((count + kRansacEvalBlock - 1) / kRansacEvalBlock), (unsigned)chunks), dim3(kRansacEvalBlock), 0, s,
                     (const double*)w.rec.as<double>(), (long long)a.K, a.max_dist, (long long)itr0, hdr, (const uint32_t*)w.off.as<uint32_t>(), count,
                     (const int32_t*)w.surv.as<int32_t>(), (const double*)w.T.as<double>(), w.part_n.as<uint32_t>(), w.part_e.as<double>());
  hipLaunchKernelGGL(k_ransac_fold, dim3(nblk(count)), dim3(kB), 0, s, (long long)itr0, hdr, (const uint32_t*)w.off.as<uint32_t>(), count, chunks,
                     (const int32_t*)w.surv.as<int32_t>(), (const uint32_t*)w.part_n.as<uint32_t>(), (const double*)w.part_e.as<double>(),
                     w.sv_n.as<uint32_t>(), w.sv_e.as<double>(), slot_n, slot_e);
  CK(hipGetLastError());
  (void)batch;
  return O3S_OK;
}

// The whole registration on device arrays (points 3 x N, pairs 2 x K int32, table n_iter x ransac_n int32 or null).  The host issues
// batches up to kRansacAhead ahead of the last est_k it has seen; what it has not seen yet costs launches that return at once, never
// a different result.  out_inliers: host, 2 x K int32, nullable.
inline int ransac_run_dev(RansacWork& w, const double* d_src, int64_t ns, const double* d_tgt, int64_t nt, const int32_t* d_pairs, int64_t K,
                          const o3s_ransac_params* p, const int32_t* d_table, int64_t n_table, o3s_ransac_result* result, int32_t* out_inliers,
                          hipStream_t s) {
  const int64_t n_iter = d_table ? std::min<int64_t>(p->max_iteration, n_table) : (int64_t)p->max_iteration;
  ransac_empty_result(result, n_iter);
  if (K > (int64_t)(1 << 24)) return O3S_ERR_BAD_ARGUMENT;
  const int batch = ransac_batch();
  int rc = ransac_size_work(w, K, batch);
  if (rc != O3S_OK) return rc;
  rc = ransac_prepare(w, d_src, ns, d_tgt, nt, d_pairs, K, n_iter, s);
  if (rc != O3S_OK) return rc;
  const RansacArgs a = ransac_args(p, K);
  RansacHeader* hdr = w.hdr.as<RansacHeader>();
  const bool posts = posts_enabled() && w.post;
  uint32_t seqs[kRansacAhead] = {0, 0, 0, 0};
  int64_t est_k = n_iter;
  for (int64_t b = 0;; ++b) {
    const int slot = (int)(b % kRansacAhead);
    if (b >= kRansacAhead) {  // the post of batch b - kRansacAhead: one outstanding post per slot, read by its issuer
      const uint32_t* mb = w.post.host + slot * kRansacSlotWords;
      if (posts) {
        const uint32_t seq = seqs[slot];
        const int pw = poll_until([=] { return post_landed(mb, seq); }, s, kMailboxCadence);
        if (pw == kPollError) return O3S_ERR_HIP;
        if (pw == kPollPosted) est_k = (int64_t)post_get<unsigned long long>(mb, kPostVals);
      } else {
        RansacHeader h;
        CK(hipMemcpyAsync(&h, hdr, sizeof(h), hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        est_k = h.est_k;
      }
    }
    const int64_t itr0 = b * (int64_t)batch;
    if (itr0 >= est_k) break;
    const int count = (int)std::min<int64_t>(batch, n_iter - itr0);
    rc = ransac_issue_batch(w, a, d_table, itr0, count, batch, hdr, nullptr, nullptr, s);
    if (rc != O3S_OK) return rc;
    seqs[slot] = posts ? w.post.next() : 0u;
    hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(64), 0, s, a, hdr, (long long)itr0, (const uint32_t*)w.off.as<uint32_t>(), count,
                       (const int32_t*)w.surv.as<int32_t>(), (const uint32_t*)w.sv_n.as<uint32_t>(), (const double*)w.sv_e.as<double>(),
                       (const double*)w.T.as<double>(), posts ? w.post.dev + slot * kRansacSlotWords : (uint32_t*)nullptr, seqs[slot]);
    CK(hipGetLastError());
  }
  // the winner's inlier list, then the header: the one read-back of the call
  hipLaunchKernelGGL(k_ransac_inlier_flags, dim3(nblk(K)), dim3(kB), 0, s, (const double*)w.rec.as<double>(), (long long)K, a.max_dist,
                     (const RansacHeader*)hdr, w.iflag.as<uint32_t>());
  CK(hipMemsetAsync(w.iflag.as<uint32_t>() + K, 0, 4, s));
  rc = scan_flags_dev(w.iflag.as<uint32_t>(), w.ioff.as<uint32_t>(), K + 1, w.scan_tmp.p, w.scan_bytes, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_ransac_inlier_scatter, dim3(nblk(K)), dim3(kB), 0, s, (const uint32_t*)w.iflag.as<uint32_t>(), (const uint32_t*)w.ioff.as<uint32_t>(),
                     (long long)K, d_pairs, w.iout.as<int32_t>());
  CK(hipGetLastError());
  RansacHeader h;
  uint32_t n_list = 0;
  CK(hipMemcpyAsync(&h, hdr, sizeof(h), hipMemcpyDeviceToHost, s));
  CK(hipMemcpyAsync(&n_list, w.ioff.as<uint32_t>() + K, 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (h.bad) return O3S_ERR_BAD_ARGUMENT;
  result->est_k = h.est_k;
  result->evaluated = h.evaluated;
  if (h.best_itr < 0) return O3S_OK;
  if ((long long)n_list != h.n_in) return O3S_ERR_HIP;  // the list and the count come from the same arithmetic
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) result->transformation[c * 4 + r] = h.T[4 * r + c];
  result->fitness = h.fitness;
  result->inlier_rmse = h.rmse;
  result->correspondences = h.n_in;
  result->best_iteration = h.best_itr;
  if (out_inliers && n_list) CK(hipMemcpy(out_inliers, w.iout.p, (size_t)n_list * 8, hipMemcpyDeviceToHost));
  return O3S_OK;
}

inline int ransac_upload_clouds(RansacWork& w, const double* source, int64_t Ns, const double* target, int64_t Nt, const int32_t* pairs, int64_t K,
                                hipStream_t s) {
  CK(w.src.alloc((size_t)Ns * 24));
  CK(w.tgt.alloc((size_t)Nt * 24));
  CK(w.pairs.alloc((size_t)K * 8));
  CK(hipMemcpyAsync(w.src.p, source, (size_t)Ns * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(w.tgt.p, target, (size_t)Nt * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(w.pairs.p, pairs, (size_t)K * 8, hipMemcpyHostToDevice, s));
  return O3S_OK;
}
inline bool ransac_pairs_in_range(const int32_t* pairs, int64_t K, int64_t Ns, int64_t Nt) {
  for (int64_t k = 0; k < K; ++k)
    if (pairs[2 * k] < 0 || pairs[2 * k] >= Ns || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= Nt) return false;
  return true;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

void o3s_ransac_default_params(o3s_ransac_params* p) {
  if (!p) return;
  p->max_correspondence_distance = 0.75;
  p->ransac_n = 3;
  p->distance_threshold = 0.8;
  p->edge_length_similarity = 0.6;
  p->check_distance = 1;
  p->check_edge_length = 1;
  p->max_iteration = 10000000;
  p->confidence = 0.999;
  p->seed = 0;
}

int o3s_ransac_reserve(int device, int64_t max_correspondences) {
  if (max_correspondences < 0 || max_correspondences > (int64_t)(1 << 24)) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  RansacLease w(device);
  return ransac_size_work(*w, max_correspondences, ransac_batch());
}

int o3s_ransac_release(int device) { return release_idle_areas<RansacWork>(device); }

int o3s_registration_ransac_correspondence(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                                           const int32_t* correspondences, int64_t K, const o3s_ransac_params* params, const int32_t* samples,
                                           int64_t n_samples, o3s_ransac_result* result, int32_t* inlier_correspondences) {
  if (!result || !ransac_params_ok(params) || Ns < 0 || Nt < 0 || K < 0 || n_samples < 0 || (K > 0 && !correspondences)) return O3S_ERR_BAD_ARGUMENT;
  const int64_t n_iter = samples ? std::min<int64_t>(params->max_iteration, n_samples) : (int64_t)params->max_iteration;
  ransac_empty_result(result, n_iter);
  if (ransac_trivial(params, K)) return O3S_OK;
  if (!source || !target || Ns > (int64_t)0x7fffffff || Nt > (int64_t)0x7fffffff || K > (int64_t)(1 << 24) ||
      !ransac_pairs_in_range(correspondences, K, Ns, Nt))
    return O3S_ERR_BAD_ARGUMENT;
  if (samples)
    for (int64_t k = 0; k < n_iter * params->ransac_n; ++k)
      if (samples[k] < 0 || samples[k] >= K) return O3S_ERR_BAD_ARGUMENT;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  RansacLease w(device);
  rc = ransac_upload_clouds(*w, source, Ns, target, Nt, correspondences, K, w.s);
  if (rc != O3S_OK) return rc;
  if (samples && n_iter > 0) {
    CK(w->table.alloc((size_t)n_iter * params->ransac_n * 4));
    CK(hipMemcpyAsync(w->table.p, samples, (size_t)n_iter * params->ransac_n * 4, hipMemcpyHostToDevice, w.s));
  }
  return ransac_run_dev(*w, w->src.as<double>(), Ns, w->tgt.as<double>(), Nt, w->pairs.as<int32_t>(), K, params,
                        samples ? w->table.as<int32_t>() : nullptr, n_iter, result, inlier_correspondences, w.s);
}

int o3s_registration_ransac_feature_matching(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                                             const double* source_feature, const double* target_feature, int32_t dim, int32_t mutual_filter,
                                             const o3s_ransac_params* params, o3s_ransac_result* result, int32_t* inlier_correspondences,
                                             int64_t* n_correspondences) {
  if (!result || !ransac_params_ok(params) || Ns < 0 || Nt < 0 || dim < 1) return O3S_ERR_BAD_ARGUMENT;
  if (n_correspondences) *n_correspondences = 0;
  ransac_empty_result(result, params->max_iteration);
  if (Ns == 0 || Nt == 0) return O3S_OK;
  if (!source || !target || !source_feature || !target_feature) return O3S_ERR_BAD_ARGUMENT;
  std::vector<int32_t> pairs((size_t)Ns * 2);
  int64_t K = 0;
  const int rc = o3s_feature_correspondences(device, source_feature, Ns, target_feature, Nt, dim, mutual_filter, std::max(params->ransac_n, 0),
                                             pairs.data(), &K, nullptr);
  if (rc != O3S_OK) return rc;
  if (n_correspondences) *n_correspondences = K;
  return o3s_registration_ransac_correspondence(device, source, Ns, target, Nt, pairs.data(), K, params, nullptr, 0, result, inlier_correspondences);
}

int o3s_ransac_evaluate_samples(int device, const double* source, int64_t Ns, const double* target, int64_t Nt, const int32_t* correspondences,
                                int64_t K, const o3s_ransac_params* params, const int32_t* samples, int64_t first_iteration, int64_t H,
                                int32_t* outcome, double* transformations, int64_t* n_in, double* err2) {
  if (!ransac_params_ok(params) || params->ransac_n < 3 || K < params->ransac_n || !(params->max_correspondence_distance > 0.0) || H < 0 ||
      first_iteration < 0 || (samples && first_iteration != 0) || !source || !target || !correspondences || !outcome || Ns < 0 || Nt < 0 ||
      Ns > (int64_t)0x7fffffff || Nt > (int64_t)0x7fffffff || K > (int64_t)(1 << 24) || !ransac_pairs_in_range(correspondences, K, Ns, Nt))
    return O3S_ERR_BAD_ARGUMENT;
  if (H == 0) return O3S_OK;
  if (samples)
    for (int64_t k = 0; k < H * params->ransac_n; ++k)
      if (samples[k] < 0 || samples[k] >= K) return O3S_ERR_BAD_ARGUMENT;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  RansacLease w(device);
  hipStream_t s = w.s;
  const int batch = ransac_batch();
  rc = ransac_size_work(*w, K, batch);
  if (rc != O3S_OK) return rc;
  CK(w->slot_n.alloc((size_t)batch * 8));
  CK(w->slot_e.alloc((size_t)batch * 8));
  rc = ransac_upload_clouds(*w, source, Ns, target, Nt, correspondences, K, s);
  if (rc != O3S_OK) return rc;
  if (samples) {
    CK(w->table.alloc((size_t)H * params->ransac_n * 4));
    CK(hipMemcpyAsync(w->table.p, samples, (size_t)H * params->ransac_n * 4, hipMemcpyHostToDevice, s));
  }
  rc = ransac_prepare(*w, w->src.as<double>(), Ns, w->tgt.as<double>(), Nt, w->pairs.as<int32_t>(), K, H, s);
  if (rc != O3S_OK) return rc;
  const RansacArgs a = ransac_args(params, K);
  std::vector<double> T12((size_t)batch * 12);
  for (int64_t done = 0; done < H; done += batch) {
    const int count = (int)std::min<int64_t>(batch, H - done);
    CK(hipMemsetAsync(w->slot_n.p, 0, (size_t)count * 8, s));
    CK(hipMemsetAsync(w->slot_e.p, 0, (size_t)count * 8, s));
    rc = ransac_issue_batch(*w, a, samples ? w->table.as<int32_t>() : nullptr, first_iteration + done, count, batch, nullptr,
                            w->slot_n.as<long long>(), w->slot_e.as<double>(), s);
    if (rc != O3S_OK) return rc;
    CK(hipMemcpyAsync(outcome + done, w->outcome.p, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    if (transformations) CK(hipMemcpyAsync(T12.data(), w->T.p, (size_t)count * 96, hipMemcpyDeviceToHost, s));
    if (n_in) CK(hipMemcpyAsync(n_in + done, w->slot_n.p, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    if (err2) CK(hipMemcpyAsync(err2 + done, w->slot_e.p, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (transformations)
      for (int i = 0; i < count; ++i) {
        double* M = transformations + (size_t)(done + i) * 16;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 4; ++c) M[c * 4 + r] = T12[(size_t)i * 12 + 4 * r + c];
        M[3] = M[7] = M[11] = 0.0;
        M[15] = 1.0;
      }
  }
  return O3S_OK;
}

int o3s_submap_registration_ransac(const o3s_submap* source, const o3s_submap* target, int32_t mutual_filter, const o3s_ransac_params* params,
                                   o3s_ransac_result* result, int32_t* inlier_correspondences, int64_t* n_correspondences) {
  if (!source || !target || !result || !ransac_params_ok(params) || source->device != target->device) return O3S_ERR_BAD_ARGUMENT;
  if (source->n_feat < 0 || target->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  if (n_correspondences) *n_correspondences = 0;
  ransac_empty_result(result, params->max_iteration);
  if (source->n_feat == 0 || target->n_feat == 0) return O3S_OK;
  int rc = set_dev(source);
  if (rc != O3S_OK) return rc;
  hipStream_t s = source->stream;
  CK(hipStreamSynchronize(target->stream));  // both feature sets are complete; everything below runs on the source's stream
  RansacLease w(source->device, s);
  // the mutual filter of the two index arrays runs on the host (feature_correspondences_dev): 4 (n + m) bytes come down, the pairs go up
  std::vector<int32_t> pairs((size_t)source->n_feat * 2);
  int64_t K = 0;
  rc = feature_correspondences_dev(w->nn, source->feat_f.as<double>(), source->n_feat, target->feat_f.as<double>(), target->n_feat, kFpfhDim, mutual_filter,
                                   std::max(params->ransac_n, 0), pairs.data(), &K, nullptr, s);
  if (rc != O3S_OK) return rc;
  if (n_correspondences) *n_correspondences = K;
  if (ransac_trivial(params, K)) return O3S_OK;
  CK(w->feat_pairs.alloc((size_t)K * 8));
  CK(hipMemcpyAsync(w->feat_pairs.p, pairs.data(), (size_t)K * 8, hipMemcpyHostToDevice, s));
  rc = ransac_run_dev(*w, source->feat_p.as<double>(), source->n_feat, target->feat_p.as<double>(), target->n_feat, w->feat_pairs.as<int32_t>(), K, params, nullptr, 0,
                      result, inlier_correspondences, s);
  return rc;
}

}  // extern "C"
