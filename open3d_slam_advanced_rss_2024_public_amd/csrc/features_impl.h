// features_impl.h — C entry points of the place-recognition front end (include/o3s_cloud_ops.h: o3s_compute_fpfh,
// o3s_feature_correspondences; include/o3s_submap.h: o3s_submap_compute_features and its companions).  Included at the end of
// cloud_ops.hip after submap_impl.h; the kernels are in fpfh_dev.h.
#pragma once
#include "fpfh_dev.h"
#include "submap_impl.h"

extern "C" {

int o3s_compute_fpfh(int device, const double* pts, const double* normals, int64_t N, double radius, int32_t max_nn, double* out_fpfh,
                     double* out_spfh, int32_t* out_nn_idx) {
  if (N < 0 || max_nn < 1 || max_nn > kFpfhNnMax || !(radius > 0.0) || !std::isfinite(radius)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  if (!pts || !normals || !out_fpfh || N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_p, d_n, d_f;
  FpfhWork w;
  CK(d_p.alloc((size_t)N * 24));
  CK(d_n.alloc((size_t)N * 24));
  CK(d_f.alloc((size_t)N * kFpfhDim * 8));
  CK(hipMemcpyAsync(d_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(d_n.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  rc = fpfh_dev(w, d_p.as<double>(), d_n.as<double>(), N, radius, max_nn, d_f.as<double>(), s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(out_fpfh, d_f.p, (size_t)N * kFpfhDim * 8, hipMemcpyDeviceToHost, s));
  if (out_spfh) CK(hipMemcpyAsync(out_spfh, w.spfh.p, (size_t)N * kFpfhDim * 8, hipMemcpyDeviceToHost, s));
  if (out_nn_idx) CK(hipMemcpyAsync(out_nn_idx, w.idx.p, (size_t)N * (size_t)max_nn * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return O3S_OK;
}

int o3s_feature_correspondences(int device, const double* src_feat, int64_t n_src, const double* tgt_feat, int64_t n_tgt, int32_t dim,
                                int32_t mutual_filter, int32_t ransac_n, int32_t* out_pairs, int64_t* n_out, int32_t* used_fallback) {
  if (!n_out || n_src < 0 || n_tgt < 0 || dim < 1 || dim > kFcDimMax || ransac_n < 0) return O3S_ERR_BAD_ARGUMENT;
  *n_out = 0;
  if (used_fallback) *used_fallback = 0;
  if (n_src == 0 || n_tgt == 0) return O3S_OK;
  if (!src_feat || !tgt_feat || !out_pairs || n_src > (int64_t)0x7fffffff || n_tgt > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_a, d_b;
  FeatNnWork w;
  CK(d_a.alloc((size_t)n_src * (size_t)dim * 8));
  CK(d_b.alloc((size_t)n_tgt * (size_t)dim * 8));
  CK(hipMemcpyAsync(d_a.p, src_feat, (size_t)n_src * (size_t)dim * 8, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(d_b.p, tgt_feat, (size_t)n_tgt * (size_t)dim * 8, hipMemcpyHostToDevice, s));
  int fb = 0;
  const int rf = feature_correspondences_dev(w, d_a.as<double>(), n_src, d_b.as<double>(), n_tgt, dim, mutual_filter, ransac_n, out_pairs, n_out, &fb, s);
  if (used_fallback) *used_fallback = fb;
  return rf;
}

void o3s_submap_feature_params_default(o3s_submap_feature_params* p) {
  if (!p) return;
  p->feature_voxel_size = 0.5;
  p->normal_radius = 2.0;
  p->normal_knn = 20;
  p->feature_radius = 2.5;
  p->feature_knn = 100;
}

int o3s_submap_compute_features(o3s_submap* m, const o3s_submap_feature_params* params) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !params || !(params->feature_voxel_size > 0.0) || !(params->normal_radius > 0.0) || !(params->feature_radius > 0.0) ||
      !std::isfinite(params->feature_radius) || params->normal_knn < 1 || params->normal_knn > kNnMax || params->feature_knn < 1 ||
      params->feature_knn > kFpfhNnMax)
    return O3S_ERR_BAD_ARGUMENT;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const int64_t N = m->n;
  m->n_feat = -1;  // the old set is gone whatever happens below
  if (N == 0) {
    m->n_feat = 0;
    return O3S_OK;
  }
  // sparseMapCloud_ = *mapCopy.VoxelDownSample(featureVoxelSize_): at most one point per map point
  CK(m->feat_p.ensure((size_t)N * 24, 0, s));
  CK(m->feat_n.ensure((size_t)N * 24, 0, s));
  int64_t n_sparse = 0;
  rc = voxel_pipeline_dev(m->feat_w.grid.arena, 1, nullptr, params->feature_voxel_size, m->pts[m->cur].as<double>(), nullptr, N, m->feat_p.as<double>(), m->feat_n.as<double>(),
                          nullptr, &n_sparse, s);
  if (rc != O3S_OK) return rc;
  if (n_sparse > 0) {
    // EstimateNormals(Hybrid(normalEstimationRadius_, normalKnn_)) + NormalizeNormals + OrientNormalsTowardsCameraLocation(0)
    rc = estimate_normals_dev(m->feat_w.grid, m->feat_p.as<double>(), n_sparse, params->normal_radius, params->normal_knn, m->feat_n.as<double>(), nullptr, s);
    if (rc != O3S_OK) return rc;
    // feature_ = ComputeFPFHFeature(sparseMapCloud_, Hybrid(featureRadius_, featureKnn_))
    CK(m->feat_f.ensure((size_t)n_sparse * kFpfhDim * 8, 0, s));
    rc = fpfh_dev(m->feat_w, m->feat_p.as<double>(), m->feat_n.as<double>(), n_sparse, params->feature_radius, params->feature_knn, m->feat_f.as<double>(), s);
    if (rc != O3S_OK) return rc;
  }
  CK(hipStreamSynchronize(s));
  m->n_feat = n_sparse;
  return O3S_OK;
}

int64_t o3s_submap_features_size(const o3s_submap* m) { return m ? m->n_feat : -1; }

int o3s_submap_download_features(const o3s_submap* m, double* sparse_pts, double* sparse_normals, double* fpfh) {
  if (!m) return O3S_ERR_BAD_ARGUMENT;
  if (m->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  if (m->n_feat == 0) return O3S_OK;
  if (hipSetDevice(m->device) != hipSuccess) return O3S_ERR_HIP;
  CK(hipStreamSynchronize(m->stream));
  const size_t n = (size_t)m->n_feat;
  if (sparse_pts) CK(hipMemcpy(sparse_pts, m->feat_p.p, n * 24, hipMemcpyDeviceToHost));
  if (sparse_normals) CK(hipMemcpy(sparse_normals, m->feat_n.p, n * 24, hipMemcpyDeviceToHost));
  if (fpfh) CK(hipMemcpy(fpfh, m->feat_f.p, n * kFpfhDim * 8, hipMemcpyDeviceToHost));
  return O3S_OK;
}

int o3s_submap_feature_correspondences(const o3s_submap* source, const o3s_submap* target, int32_t mutual_filter, int32_t ransac_n,
                                       int32_t* out_pairs, int64_t* n_out, int32_t* used_fallback) {
  if (!source || !target || !n_out || ransac_n < 0 || source->device != target->device) return O3S_ERR_BAD_ARGUMENT;
  if (source->n_feat < 0 || target->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  *n_out = 0;
  if (used_fallback) *used_fallback = 0;
  if (source->n_feat == 0 || target->n_feat == 0) return O3S_OK;
  if (!out_pairs) return O3S_ERR_BAD_ARGUMENT;
  const int rc = set_dev(source);
  if (rc != O3S_OK) return rc;
  // both feature sets are complete (compute_features returns after its work); the search runs on the source's stream
  CK(hipStreamSynchronize(target->stream));
  FeatNnWork w;
  int fb = 0;
  const int rf = feature_correspondences_dev(w, source->feat_f.as<double>(), source->n_feat, target->feat_f.as<double>(), target->n_feat, kFpfhDim, mutual_filter, ransac_n,
                                             out_pairs, n_out, &fb, source->stream);
  if (used_fallback) *used_fallback = fb;
  return rf;
}

}  // extern "C"
