// cluster_impl.h — host side and C entry points of DBSCAN clustering and small-cluster removal (include/clustering/o3s_clustering.h).
// Included at the end of cloud_ops.hip behind outlier_impl.h, whose resident paths it shares; the kernels are in cluster_dev.h.
#pragma once
#include "cluster_dev.h"
#include "outlier_impl.h"

#include "../../include/clustering/o3s_clustering.h"

namespace {
namespace o3s_cloud {

using ClusterLease = AreaLease<ClusterWork, /*kAlwaysDrain=*/true>;  // every exit hands the area back behind a drained stream

// the parameter checks of the five entries (min_points 0 is the caller's: it returns before this)
inline bool dbscan_params_valid(const o3s_dbscan_params* p) {
  return p && p->min_points > 0 && p->eps > 0.0 && std::isfinite(p->eps) && p->min_cluster_size >= 0;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_cluster_dbscan(int device, const o3s_dbscan_params* p, const double* pts, int64_t N, int32_t* labels, int32_t* n_clusters, int32_t* cluster_sizes) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_points == 0) return O3S_OK;
  if (!dbscan_params_valid(p) || !n_clusters || N < 0 || N > (int64_t)0x7fffffff || (N > 0 && (!pts || !labels))) return O3S_ERR_BAD_ARGUMENT;
  *n_clusters = 0;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  ClusterLease w(device, s);
  DevMem d_p;
  CK(d_p.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  ClusterResult r;
  rc = dbscan_dev(*w, p->eps, p->min_points, 0, /*with_keep=*/false, d_p.as<double>(), N, &r, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(labels, r.labels, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  if (cluster_sizes && r.n_clusters) CK(hipMemcpyAsync(cluster_sizes, r.size, (size_t)r.n_clusters * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *n_clusters = (int32_t)r.n_clusters;
  return O3S_OK;
}

int o3s_remove_small_clusters(int device, const o3s_dbscan_params* p, const double* pts, const double* normals, int64_t N, double* out_pts, double* out_normals,
                              int64_t* out_indices, int64_t* n_out, int32_t* labels, int32_t* n_clusters) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_points == 0) return O3S_OK;
  if (!dbscan_params_valid(p) || !n_out || N < 0 || N > (int64_t)0x7fffffff || (N > 0 && (!pts || !out_pts || (normals && !out_normals))))
    return O3S_ERR_BAD_ARGUMENT;
  *n_out = 0;
  if (n_clusters) *n_clusters = 0;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  ClusterLease w(device, s);
  DevMem d_p, d_n;
  CK(d_p.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(d_n.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(d_n.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  CK(w->out_p.alloc((size_t)N * 24));
  CK(w->out_n.alloc((size_t)N * 24));
  if (out_indices) CK(w->out_i.alloc((size_t)N * 8));
  ClusterResult r;
  rc = dbscan_dev(*w, p->eps, p->min_points, p->min_cluster_size, /*with_keep=*/true, d_p.as<double>(), N, &r, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_compact, dim3(nblk(N)), dim3(kB), 0, s, d_p.as<double>(), normals ? d_n.as<double>() : nullptr, N, r.keep, r.off, w->out_p.as<double>(),
                     w->out_n.as<double>(), (int32_t*)nullptr);
  if (out_indices) hipLaunchKernelGGL(k_or_kept_idx, dim3(nblk(N)), dim3(kB), 0, s, r.keep, r.off, N, w->out_i.as<int64_t>());
  CK(hipGetLastError());
  const size_t k = (size_t)r.n_keep;
  if (k) {
    CK(hipMemcpyAsync(out_pts, w->out_p.p, k * 24, hipMemcpyDeviceToHost, s));
    if (normals) CK(hipMemcpyAsync(out_normals, w->out_n.p, k * 24, hipMemcpyDeviceToHost, s));
    if (out_indices) CK(hipMemcpyAsync(out_indices, w->out_i.p, k * 8, hipMemcpyDeviceToHost, s));
  }
  if (labels) CK(hipMemcpyAsync(labels, r.labels, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *n_out = r.n_keep;
  if (n_clusters) *n_clusters = (int32_t)r.n_clusters;
  return O3S_OK;
}

int o3s_submap_cluster_dbscan(o3s_submap* m, const o3s_dbscan_params* p, int32_t* labels, int32_t* n_clusters) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_points == 0) return O3S_OK;
  if (!dbscan_params_valid(p) || !n_clusters) return O3S_ERR_BAD_ARGUMENT;
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  *n_clusters = 0;
  if (m->n == 0) return O3S_OK;
  if (!labels) return O3S_ERR_BAD_ARGUMENT;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  ClusterLease w(m->device, s);
  ClusterResult r;
  rc = dbscan_dev(*w, p->eps, p->min_points, 0, /*with_keep=*/false, m->pts[m->cur].as<double>(), m->n, &r, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(labels, r.labels, (size_t)m->n * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *n_clusters = (int32_t)r.n_clusters;
  return O3S_OK;
}

int o3s_submap_remove_small_clusters(o3s_submap* m, const o3s_dbscan_params* p, int64_t* n_removed, int32_t* n_clusters) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_points == 0) return O3S_OK;
  if (!dbscan_params_valid(p)) return O3S_ERR_BAD_ARGUMENT;
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (n_removed) *n_removed = 0;
  if (n_clusters) *n_clusters = 0;
  if (m->n == 0) return O3S_OK;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const int64_t Nm = m->n;
  ClusterLease w(m->device, s);
  ClusterResult r;
  rc = dbscan_dev(*w, p->eps, p->min_points, p->min_cluster_size, /*with_keep=*/true, m->pts[m->cur].as<double>(), Nm, &r, s);
  if (rc != O3S_OK) return rc;
  rc = submap_keep_flagged(m, r.keep, r.off, r.n_keep);  // the path carving removes by
  if (rc != O3S_OK) return rc;
  if (n_removed) *n_removed = Nm - r.n_keep;
  if (n_clusters) *n_clusters = (int32_t)r.n_clusters;
  return O3S_OK;
}

int o3s_scan_remove_small_clusters(o3s_scan* sc, const o3s_cropper* scan_matcher_cropper, const o3s_dbscan_params* p, int64_t* n_merge, int64_t* n_match) {
  if (!sc || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_points == 0) return O3S_OK;
  if (!dbscan_params_valid(p) || !scan_matcher_cropper) return O3S_ERR_BAD_ARGUMENT;
  if (n_merge) *n_merge = sc->n_wide;
  if (n_match) *n_match = sc->n_narrow;
  if (sc->n_wide == 0) return O3S_OK;
  if (hipSetDevice(sc->device) != hipSuccess) return O3S_ERR_HIP;
  hipStream_t s = sc->stream;
  int64_t n_keep = 0;
  {
    ClusterLease w(sc->device, s);
    ClusterResult r;
    int rc = dbscan_dev(*w, p->eps, p->min_points, p->min_cluster_size, /*with_keep=*/true, sc->wide_p.as<double>(), sc->n_wide, &r, s);
    if (rc != O3S_OK) return rc;
    n_keep = r.n_keep;
    rc = scan_keep_flagged(sc, r.keep, r.off, n_keep);
    if (rc != O3S_OK) return rc;
  }
  return scan_recrop(sc, scan_matcher_cropper, n_keep, n_merge, n_match);
}

}  // extern "C"
