// keypoints_impl.h — host side and C entry points of the ISS keypoints (include/keypoints/o3s_keypoints.h).  Included at the end of
// cloud_ops.hip behind plane_impl.h; the kernels are in keypoints_dev.h.
#pragma once
#include "keypoints_dev.h"
#include "features_impl.h"

#include "../../include/keypoints/o3s_keypoints.h"

namespace {
namespace o3s_cloud {

using IssLease = AreaLease<IssWork, /*kAlwaysDrain=*/true>;  // every exit hands the area back behind a drained stream

// the parameter checks of the three entries (min_neighbors 0 is the caller's: it returns before this)
inline bool iss_params_valid(const o3s_iss_params* p) {
  if (!p || p->min_neighbors < 0) return false;
  if (!(p->salient_radius >= 0.0) || !std::isfinite(p->salient_radius) || !(p->non_max_radius >= 0.0) || !std::isfinite(p->non_max_radius)) return false;
  return p->gamma_21 > 0.0 && p->gamma_32 > 0.0;  // (a NaN fails both)
}

// the radii an empty cloud reports: the contract's resolution of no points is 0
inline void iss_radii_of_empty(const o3s_iss_params* p, double* radii2) {
  if (!radii2) return;
  const bool from_res = p->salient_radius == 0.0 || p->non_max_radius == 0.0;
  radii2[0] = from_res ? 0.0 : p->salient_radius;
  radii2[1] = from_res ? 0.0 : p->non_max_radius;
}

inline int iss_run(IssWork& w, const o3s_iss_params* p, const double* d_pts, int64_t N, IssResult* r, hipStream_t s) {
  return iss_flags_dev(w, p->salient_radius, p->non_max_radius, p->gamma_21, p->gamma_32, p->min_neighbors, d_pts, N, r, s);
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

int o3s_iss_keypoints(int device, const o3s_iss_params* p, const double* pts, const double* normals, int64_t N, double* out_pts, double* out_normals,
                      int64_t* out_indices, int64_t* n_keypoints, double* saliency, double radii2[2]) {
  if (!p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_neighbors == 0) return O3S_OK;
  if (!iss_params_valid(p) || !n_keypoints || N < 0 || N > (int64_t)0x7fffffff || (N > 0 && (!pts || !out_pts || (normals && !out_normals))))
    return O3S_ERR_BAD_ARGUMENT;
  *n_keypoints = 0;
  if (N == 0) {
    iss_radii_of_empty(p, radii2);
    return O3S_OK;
  }
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  IssLease w(device, s);
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
  IssResult r;
  rc = iss_run(*w, p, d_p.as<double>(), N, &r, s);
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
  if (saliency) CK(hipMemcpyAsync(saliency, r.sal, (size_t)N * 8, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (radii2) radii2[0] = r.radii[0], radii2[1] = r.radii[1];
  *n_keypoints = r.n_keep;
  return O3S_OK;
}

int o3s_submap_select_keypoints(o3s_submap* m, const o3s_iss_params* p, int64_t* out_indices, int64_t* n_keypoints, double radii2[2]) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_neighbors == 0) return O3S_OK;
  if (!iss_params_valid(p)) return O3S_ERR_BAD_ARGUMENT;
  if (m->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  if (n_keypoints) *n_keypoints = 0;
  const int64_t N = m->n_feat;
  if (N == 0) {
    iss_radii_of_empty(p, radii2);
    return O3S_OK;
  }
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  IssLease w(m->device, s);
  IssResult r;
  rc = iss_run(*w, p, m->feat_p.as<double>(), N, &r, s);
  if (rc != O3S_OK) return rc;
  const size_t k = (size_t)r.n_keep;
  // the survivors go to the area's arrays, which then change places with the submap's: no kernel compacts onto what another still reads
  CK(w->out_i.alloc((size_t)N * 8));
  CK(w->out_p.alloc(k * 24));
  CK(w->out_n.alloc(k * 24));
  CK(w->out_f.alloc(k * kFpfhDim * 8));
  hipLaunchKernelGGL(k_or_kept_idx, dim3(nblk(N)), dim3(kB), 0, s, r.keep, r.off, N, w->out_i.as<int64_t>());
  if (k)
    hipLaunchKernelGGL(k_iss_gather_feat, dim3(nblk((int64_t)k * kIssRow)), dim3(kB), 0, s, (const int64_t*)w->out_i.as<int64_t>(), (int64_t)k,
                       (const double*)m->feat_p.as<double>(), (const double*)m->feat_n.as<double>(), (const double*)m->feat_f.as<double>(), w->out_p.as<double>(),
                       w->out_n.as<double>(), w->out_f.as<double>());
  CK(hipGetLastError());
  if (out_indices && k) CK(hipMemcpyAsync(out_indices, w->out_i.p, k * 8, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  std::swap(m->feat_p, w->out_p);
  std::swap(m->feat_n, w->out_n);
  std::swap(m->feat_f, w->out_f);
  m->n_feat = r.n_keep;
  if (radii2) radii2[0] = r.radii[0], radii2[1] = r.radii[1];
  if (n_keypoints) *n_keypoints = r.n_keep;
  return O3S_OK;
}

int o3s_submap_feature_keypoints(const o3s_submap* m, const o3s_iss_params* p, int32_t* flags, double* saliency, int64_t* n_keypoints, double radii2[2]) {
  if (!m || !p) return O3S_ERR_BAD_ARGUMENT;
  if (p->min_neighbors == 0) return O3S_OK;
  if (!iss_params_valid(p)) return O3S_ERR_BAD_ARGUMENT;
  if (m->n_feat < 0) return O3S_ERR_NOT_INITIALIZED;
  if (n_keypoints) *n_keypoints = 0;
  const int64_t N = m->n_feat;
  if (N == 0) {
    iss_radii_of_empty(p, radii2);
    return O3S_OK;
  }
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  IssLease w(m->device, s);
  IssResult r;
  rc = iss_run(*w, p, m->feat_p.as<double>(), N, &r, s);
  if (rc != O3S_OK) return rc;
  if (flags) CK(hipMemcpyAsync(flags, r.keep, (size_t)N * 4, hipMemcpyDeviceToHost, s));  // 0 / 1 words
  if (saliency) CK(hipMemcpyAsync(saliency, r.sal, (size_t)N * 8, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (radii2) radii2[0] = r.radii[0], radii2[1] = r.radii[1];
  if (n_keypoints) *n_keypoints = r.n_keep;
  return O3S_OK;
}

}  // extern "C"
