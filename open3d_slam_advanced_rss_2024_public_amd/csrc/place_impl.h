// place_impl.h — C entry points of the one-to-many place-recognition front end (include/place_recognition/o3s_place_recognition.h).
// Included at the end of cloud_ops.hip after ransac_impl.h; the kernels and place_correspondences_dev are in fpfh_dev.h, the
// RANSAC is ransac_run_dev (ransac_impl.h), called once per target with that target's slice of the device pair buffer.
#pragma once
#include "../../include/place_recognition/o3s_place_recognition.h"
#include "ransac_impl.h"

namespace {
namespace o3s_cloud {

static_assert(kPlaceMaxTargets == O3S_PLACE_MAX_TARGETS, "the table of fpfh_dev.h holds O3S_PLACE_MAX_TARGETS targets");

// sizes a one-to-many call can index: K n_src + 1 flags go through one 32-bit scan, target columns are numbered together
inline bool place_sizes_ok(int64_t n_src, const int64_t* n_tgt, int K) {
  if (n_src < 0 || n_src > (int64_t)0x7fffffff || (int64_t)K * n_src >= (int64_t)0x7fffffff) return false;
  int64_t M = 0;
  for (int k = 0; k < K; ++k) {
    if (n_tgt[k] < 0 || n_tgt[k] > (int64_t)0x7fffffff) return false;
    M += n_tgt[k];
  }
  return M < (int64_t)0x7fffffff;
}

// the error rules of the resident entries, before any work is enqueued; fills the targets' feature arrays and sizes
inline int place_check_submaps(const o3s_submap* source, const o3s_submap* const* targets, int K, const double** f, int64_t* n_tgt) {
  if (!source || !targets || K < 1 || K > kPlaceMaxTargets) return O3S_ERR_BAD_ARGUMENT;
  for (int k = 0; k < K; ++k)
    if (!targets[k] || targets[k]->device != source->device) return O3S_ERR_BAD_ARGUMENT;
  if (source->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  for (int k = 0; k < K; ++k)
    if (targets[k]->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  for (int k = 0; k < K; ++k) {
    n_tgt[k] = targets[k]->n_feat;
    f[k] = n_tgt[k] > 0 ? targets[k]->feat_f.as<double>() : nullptr;
  }
  return place_sizes_ok(source->n_feat, n_tgt, K) ? O3S_OK : O3S_ERR_BAD_ARGUMENT;
}
// every target's feature set is complete before the source's stream reads it
inline int place_drain_targets(const o3s_submap* source, const o3s_submap* const* targets, int K) {
  for (int k = 0; k < K; ++k)
    if (targets[k]->stream != source->stream) CK(hipStreamSynchronize(targets[k]->stream));
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_feature_correspondences_multi(int device, const double* src_feat, int64_t n_src, const double* const* tgt_feat, const int64_t* n_tgt, int32_t K,
                                      int32_t dim, int32_t mutual_filter, int32_t ransac_n, int32_t* out_pairs, int64_t* n_out, int32_t* used_fallback) {
  if (K < 1 || K > kPlaceMaxTargets || !n_out || !n_tgt || !tgt_feat || dim < 1 || dim > kFcDimMax || ransac_n < 0 || !place_sizes_ok(n_src, n_tgt, K))
    return O3S_ERR_BAD_ARGUMENT;
  for (int k = 0; k < K; ++k) {
    n_out[k] = 0;
    if (used_fallback) used_fallback[k] = 0;
    if (n_tgt[k] > 0 && !tgt_feat[k]) return O3S_ERR_BAD_ARGUMENT;
  }
  if (n_src == 0) return O3S_OK;
  if (!src_feat || !out_pairs) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_a, d_b[kPlaceMaxTargets];
  PlaceWork w;
  const double* d_t[kPlaceMaxTargets];
  CK(d_a.alloc((size_t)n_src * (size_t)dim * 8));
  CK(hipMemcpyAsync(d_a.p, src_feat, (size_t)n_src * (size_t)dim * 8, hipMemcpyHostToDevice, s));
  for (int k = 0; k < K; ++k) {
    d_t[k] = nullptr;
    if (n_tgt[k] == 0) continue;
    CK(d_b[k].alloc((size_t)n_tgt[k] * (size_t)dim * 8));
    CK(hipMemcpyAsync(d_b[k].p, tgt_feat[k], (size_t)n_tgt[k] * (size_t)dim * 8, hipMemcpyHostToDevice, s));
    d_t[k] = d_b[k].as<double>();
  }
  const int rf = place_correspondences_dev(w, d_a.as<double>(), n_src, d_t, n_tgt, K, dim, mutual_filter, ransac_n, n_out, used_fallback, s);
  if (rf != O3S_OK) {
    (void)hipStreamSynchronize(s);  // the buffers above are freed on return
    return rf;
  }
  for (int k = 0; k < K; ++k)
    if (n_out[k] > 0)
      CK(hipMemcpy(out_pairs + 2 * (size_t)n_src * (size_t)k, w.pairs.as<int32_t>() + 2 * (size_t)n_src * (size_t)k, (size_t)n_out[k] * 8, hipMemcpyDeviceToHost));
  return O3S_OK;
}

int o3s_submaps_feature_correspondences(const o3s_submap* source, const o3s_submap* const* targets, int32_t K, int32_t mutual_filter, int32_t ransac_n,
                                        int32_t* out_pairs, int64_t* n_out, int32_t* used_fallback) {
  const double* f[kPlaceMaxTargets];
  int64_t n_tgt[kPlaceMaxTargets];
  if (!n_out || ransac_n < 0) return O3S_ERR_BAD_ARGUMENT;
  int rc = place_check_submaps(source, targets, K, f, n_tgt);
  if (rc != O3S_OK) return rc;
  for (int k = 0; k < K; ++k) {
    n_out[k] = 0;
    if (used_fallback) used_fallback[k] = 0;
  }
  const int64_t n = source->n_feat;
  if (n == 0) return O3S_OK;
  if (!out_pairs) return O3S_ERR_BAD_ARGUMENT;
  rc = set_dev(source);
  if (rc != O3S_OK) return rc;
  hipStream_t s = source->stream;
  rc = place_drain_targets(source, targets, K);
  if (rc != O3S_OK) return rc;
  RansacLease w(source->device, s);
  rc = place_correspondences_dev(w->place, source->feat_f.as<double>(), n, f, n_tgt, K, kFpfhDim, mutual_filter, ransac_n, n_out, used_fallback, s);
  if (rc != O3S_OK) return rc;
  for (int k = 0; k < K; ++k)
    if (n_out[k] > 0)
      CK(hipMemcpyAsync(out_pairs + 2 * (size_t)n * (size_t)k, w->place.pairs.as<int32_t>() + 2 * (size_t)n * (size_t)k, (size_t)n_out[k] * 8, hipMemcpyDeviceToHost,
                        s));
  CK(hipStreamSynchronize(s));
  return O3S_OK;
}

int o3s_submaps_registration_ransac(const o3s_submap* source, const o3s_submap* const* targets, int32_t K, int32_t mutual_filter,
                                    const o3s_ransac_params* params, o3s_ransac_result* results, int32_t* inlier_correspondences, int64_t* n_correspondences) {
  const double* f[kPlaceMaxTargets];
  int64_t n_tgt[kPlaceMaxTargets], n_pairs[kPlaceMaxTargets];
  if (!results || !ransac_params_ok(params)) return O3S_ERR_BAD_ARGUMENT;
  int rc = place_check_submaps(source, targets, K, f, n_tgt);
  if (rc != O3S_OK) return rc;
  for (int k = 0; k < K; ++k) {
    if (n_correspondences) n_correspondences[k] = 0;
    ransac_empty_result(&results[k], params->max_iteration);
  }
  const int64_t n = source->n_feat;
  if (n == 0) return O3S_OK;
  rc = set_dev(source);
  if (rc != O3S_OK) return rc;
  hipStream_t s = source->stream;
  rc = place_drain_targets(source, targets, K);
  if (rc != O3S_OK) return rc;
  RansacLease w(source->device, s);
  rc = place_correspondences_dev(w->place, source->feat_f.as<double>(), n, f, n_tgt, K, kFpfhDim, mutual_filter, std::max(params->ransac_n, 0), n_pairs, nullptr, s);
  if (rc != O3S_OK) return rc;
  for (int k = 0; k < K; ++k) {  // one target after the other, each from its slice of the device pair buffer
    if (n_correspondences) n_correspondences[k] = n_pairs[k];
    if (n_tgt[k] == 0 || ransac_trivial(params, n_pairs[k])) continue;
    rc = ransac_run_dev(*w, source->feat_p.as<double>(), n, targets[k]->feat_p.as<double>(), n_tgt[k], w->place.pairs.as<int32_t>() + 2 * (size_t)n * (size_t)k, n_pairs[k], params,
                        nullptr, 0, &results[k], inlier_correspondences ? inlier_correspondences + 2 * (size_t)n * (size_t)k : nullptr, s);
    if (rc != O3S_OK) return rc;
  }
  return O3S_OK;
}

}  // extern "C"
