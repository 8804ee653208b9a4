// outlier_impl.h — host side and C entry points of the outlier filters (include/outlier_removal/o3s_outlier_removal.h).  Included at
// the end of cloud_ops.hip after submap_impl.h (the resident submap and scan); the kernels are in outlier_dev.h.
#pragma once
#include "outlier_dev.h"
#include "submap_impl.h"

#include "../../include/outlier_removal/o3s_outlier_removal.h"

namespace {
namespace o3s_cloud {

using OutlierLease = AreaLease<OutlierWork, /*kAlwaysDrain=*/true>;  // every exit hands the area back behind a drained stream

// the parameter checks of the three entries (kind 0 is the caller's: it returns before this)
inline bool outlier_params_valid(const o3s_outlier_params* p) {
  if (!p || (p->kind != 1 && p->kind != 2)) return false;
  if (p->nb < 1 || !(p->value > 0.0) || !std::isfinite(p->value)) return false;
  return p->kind == 1 || p->nb <= kNnMax;
}

// the two halves of a filter on a resident pre-processed scan (the outlier filters, the small-cluster removal)
// ... the survivors of the merge cloud, in order, through the pre-process's staging arrays (N <= the raw scan they were sized for);
// keep / off: one flag per merge point and its exclusive scan, on the scan's stream.  Returns on a drained stream
inline int scan_keep_flagged(o3s_scan* sc, const uint32_t* keep, const uint32_t* off, int64_t n_keep) {
  const int64_t N = sc->n_wide;
  if (n_keep >= N) return O3S_OK;
  hipStream_t s = sc->stream;
  CK(sc->tmp_p.ensure((size_t)N * 24, 0, s));
  CK(sc->tmp_n.ensure((size_t)N * 24, 0, s));
  hipLaunchKernelGGL(k_compact, dim3(nblk(N)), dim3(kB), 0, s, (const double*)sc->wide_p.as<double>(), (const double*)sc->wide_n.as<double>(), N, keep, off,
                     sc->tmp_p.as<double>(), sc->tmp_n.as<double>(), (int32_t*)nullptr);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s));
  std::swap(sc->wide_p, sc->tmp_p);
  std::swap(sc->wide_n, sc->tmp_n);
  return O3S_OK;
}
// ... and narrowCropped = scanMatcherCropper_->crop(*wideCropped), as scan_preprocess_impl applies it, over the n_keep survivors
inline int scan_recrop(o3s_scan* sc, const o3s_cropper* scan_matcher_cropper, int64_t n_keep, int64_t* n_merge, int64_t* n_match) {
  hipStream_t s = sc->stream;
  int64_t n_narrow = 0;
  const int rc = crop_dev(sc->arena, *scan_matcher_cropper, sc->wide_p.as<double>(), sc->wide_n.as<double>(), n_keep, sc->narrow_p.as<double>(), sc->narrow_n.as<double>(),
                          &n_narrow, s);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(s));
  sc->n_wide = n_keep;
  sc->n_narrow = n_narrow;
  sc->pm_ready = false;  // the reading in the ICP layout is rebuilt by the next o3s_scan_set_reading
  if (n_merge) *n_merge = n_keep;
  if (n_match) *n_match = n_narrow;
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_remove_outliers(int device, const o3s_outlier_params* p, const double* pts, const double* normals, int64_t N, double* out_pts,
                        double* out_normals, int64_t* out_indices, int64_t* n_out, double* avg_dist, double stats4[4]) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->kind == 0) return O3S_OK;
  if (!outlier_params_valid(p) || !n_out || N < 0 || N > (int64_t)0x7fffffff || (N > 0 && (!pts || !out_pts || (normals && !out_normals))))
    return O3S_ERR_BAD_ARGUMENT;
  *n_out = 0;
  if (N == 0) {
    if (stats4 && p->kind == 2) {  // the contract's arithmetic on no points: 0 / 0
      stats4[0] = stats4[1] = stats4[2] = std::numeric_limits<double>::quiet_NaN();
      stats4[3] = 0.0;
    }
    return O3S_OK;
  }
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  OutlierLease w(device, s);
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
  OutlierResult r;
  rc = outlier_flags_dev(*w, p->kind, p->nb, p->value, d_p.as<double>(), N, &r, s);
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
  if (avg_dist && r.avg) CK(hipMemcpyAsync(avg_dist, r.avg, (size_t)N * 8, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (stats4 && p->kind == 2)
    for (int a = 0; a < 4; ++a) stats4[a] = r.stats[a];
  *n_out = r.n_keep;
  return O3S_OK;
}

int o3s_submap_remove_outliers(o3s_submap* m, const o3s_outlier_params* p, int64_t* n_removed, double stats4[4]) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->kind == 0) return O3S_OK;
  if (!outlier_params_valid(p)) return O3S_ERR_BAD_ARGUMENT;
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (n_removed) *n_removed = 0;
  if (m->n == 0) {
    if (stats4 && p->kind == 2) {
      stats4[0] = stats4[1] = stats4[2] = std::numeric_limits<double>::quiet_NaN();
      stats4[3] = 0.0;
    }
    return O3S_OK;
  }
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const int64_t Nm = m->n;
  OutlierLease w(m->device, s);
  OutlierResult r;
  rc = outlier_flags_dev(*w, p->kind, p->nb, p->value, m->pts[m->cur].as<double>(), Nm, &r, s);
  if (rc != O3S_OK) return rc;
  rc = submap_keep_flagged(m, r.keep, r.off, r.n_keep);  // the path carving removes by
  if (rc != O3S_OK) return rc;
  if (stats4 && p->kind == 2)
    for (int a = 0; a < 4; ++a) stats4[a] = r.stats[a];
  if (n_removed) *n_removed = Nm - r.n_keep;
  return O3S_OK;
}

int o3s_scan_remove_outliers(o3s_scan* sc, const o3s_cropper* scan_matcher_cropper, const o3s_outlier_params* p, int64_t* n_merge, int64_t* n_match) {
  if (!sc || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->kind == 0) return O3S_OK;
  if (!outlier_params_valid(p) || !scan_matcher_cropper) return O3S_ERR_BAD_ARGUMENT;
  if (n_merge) *n_merge = sc->n_wide;
  if (n_match) *n_match = sc->n_narrow;
  if (sc->n_wide == 0) return O3S_OK;
  if (hipSetDevice(sc->device) != hipSuccess) return O3S_ERR_HIP;
  hipStream_t s = sc->stream;
  const int64_t N = sc->n_wide;
  int64_t n_keep = 0;
  {
    OutlierLease w(sc->device, s);
    OutlierResult r;
    int rc = outlier_flags_dev(*w, p->kind, p->nb, p->value, sc->wide_p.as<double>(), N, &r, s);
    if (rc != O3S_OK) return rc;
    n_keep = r.n_keep;
    rc = scan_keep_flagged(sc, r.keep, r.off, n_keep);
    if (rc != O3S_OK) return rc;
  }
  return scan_recrop(sc, scan_matcher_cropper, n_keep, n_merge, n_match);
}

}  // extern "C"
