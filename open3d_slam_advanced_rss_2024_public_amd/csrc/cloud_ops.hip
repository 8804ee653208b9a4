// cloud_ops.hip — open3d_slam-side point-cloud operators on HOST buffers (C ABI: include/o3s_cloud_ops.h), gfx950 only.
// The kernels and the device-level pipelines live in cloud_dev.h (shared with the device-resident submap, submap.hip);
// this file stages the caller's buffers through HBM.
#include <chrono>

#include "cloud_dev.h"
#include "undistort_dev.h"
#include "trajectory_dev.h"

using namespace o3s_cloud;

namespace {

// host-buffer wrapper of voxel_pipeline_dev (colours / covariances optional)
int voxel_pipeline(int mode, const o3s_cropper* crop, double voxel, const double* pts, const double* normals, const double* colors,
                   const double* covariances, int64_t N, double* out_pts, double* out_normals, double* out_colors, double* out_covariances,
                   int32_t* out_voxel_idx, int64_t* n_out) {
  *n_out = 0;
  if (N == 0) return O3S_OK;
  if (N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  hipStream_t s = nullptr;
  DevMem d_pts, d_nrm, d_opts, d_on, d_oidx, d_col, d_cov, d_ocol, d_ocov;
  Arena ar;
  CK(d_pts.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d_pts.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(d_nrm.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(d_nrm.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  Attrs at;
  if (colors) {
    CK(d_col.alloc((size_t)N * 24));
    CK(d_ocol.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(d_col.p, colors, (size_t)N * 24, hipMemcpyHostToDevice, s));
    at.col = d_col.as<double>();
    at.out_col = d_ocol.as<double>();
  }
  if (covariances) {
    CK(d_cov.alloc((size_t)N * 72));
    CK(d_ocov.alloc((size_t)N * 72));
    CK(hipMemcpyAsync(d_cov.p, covariances, (size_t)N * 72, hipMemcpyHostToDevice, s));
    at.cov = d_cov.as<double>();
    at.out_cov = d_ocov.as<double>();
  }
  CK(d_opts.alloc((size_t)N * 24));
  CK(d_on.alloc((size_t)N * 24));
  CK(d_oidx.alloc((size_t)N * 12));
  int64_t total = 0;
  const int rc = voxel_pipeline_dev(ar, mode, crop, voxel, d_pts.as<double>(), normals ? d_nrm.as<double>() : nullptr, N, d_opts.as<double>(),
                                    d_on.as<double>(), d_oidx.as<int32_t>(), &total, s, &at);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(out_pts, d_opts.p, (size_t)total * 24, hipMemcpyDeviceToHost, s));
  if (normals && out_normals) CK(hipMemcpyAsync(out_normals, d_on.p, (size_t)total * 24, hipMemcpyDeviceToHost, s));
  if (colors) CK(hipMemcpyAsync(out_colors, d_ocol.p, (size_t)total * 24, hipMemcpyDeviceToHost, s));
  if (covariances) CK(hipMemcpyAsync(out_covariances, d_ocov.p, (size_t)total * 72, hipMemcpyDeviceToHost, s));
  if (out_voxel_idx) CK(hipMemcpyAsync(out_voxel_idx, d_oidx.p, (size_t)total * 12, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *n_out = total;
  return O3S_OK;
}

}  // namespace

extern "C" {

int o3s_voxel_idx(int device, const double* pts, int64_t N, double voxel_size, int32_t* idx) {
  if (!pts || !idx || N < 0 || !(voxel_size > 0.0)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  DevMem a, b;
  CK(a.alloc((size_t)N * 24));
  CK(b.alloc((size_t)N * 12));
  CK(hipMemcpy(a.p, pts, (size_t)N * 24, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_voxel_idx, dim3(nblk(3 * N)), dim3(kB), 0, nullptr, a.as<double>(), 3 * N, 1.0 / voxel_size, b.as<int32_t>());
  CK(hipGetLastError());
  CK(hipMemcpy(idx, b.p, (size_t)N * 12, hipMemcpyDeviceToHost));
  return O3S_OK;
}

int o3s_voxel_hash(int device, const int32_t* idx, int64_t N, uint64_t* hash) {
  if (!idx || !hash || N < 0) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  DevMem a, b;
  CK(a.alloc((size_t)N * 12));
  CK(b.alloc((size_t)N * 8));
  CK(hipMemcpy(a.p, idx, (size_t)N * 12, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_voxel_hash, dim3(nblk(N)), dim3(kB), 0, nullptr, a.as<int32_t>(), N, b.as<uint64_t>());
  CK(hipGetLastError());
  CK(hipMemcpy(hash, b.p, (size_t)N * 8, hipMemcpyDeviceToHost));
  return O3S_OK;
}

int o3s_o3d_to_pm(int device, const double* pts, const double* normals, int64_t N, float* xyzw, float* out_normals) {
  if (!pts || !xyzw || N < 0 || (normals && !out_normals)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  DevMem a, b, c, d;
  CK(a.alloc((size_t)N * 24));
  CK(c.alloc((size_t)N * 16));
  CK(hipMemcpy(a.p, pts, (size_t)N * 24, hipMemcpyHostToDevice));
  if (normals) {
    CK(b.alloc((size_t)N * 24));
    CK(d.alloc((size_t)N * 12));
    CK(hipMemcpy(b.p, normals, (size_t)N * 24, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(k_o3d_to_pm, dim3(nblk(N)), dim3(kB), 0, nullptr, a.as<double>(), normals ? b.as<double>() : nullptr, N, c.as<float4>(),
                     d.as<float>());
  CK(hipGetLastError());
  CK(hipMemcpy(xyzw, c.p, (size_t)N * 16, hipMemcpyDeviceToHost));
  if (normals) CK(hipMemcpy(out_normals, d.p, (size_t)N * 12, hipMemcpyDeviceToHost));
  return O3S_OK;
}

int o3s_crop_attr(int device, const o3s_cropper* c, const double* pts, const double* normals, const double* colors, const double* covariances,
                  int64_t N, double* out_pts, double* out_normals, double* out_colors, double* out_covariances, int64_t* n_out) {
  if (!c || !pts || !out_pts || !n_out || N < 0 || (normals && !out_normals) || (colors && !out_colors) || (covariances && !out_covariances))
    return O3S_ERR_BAD_ARGUMENT;
  *n_out = 0;
  if (N == 0) return O3S_OK;
  if (N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_pts, d_nrm, d_opts, d_on, d_col, d_cov, d_ocol, d_ocov;
  Arena ar;
  CK(d_pts.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d_pts.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(d_nrm.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(d_nrm.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  Attrs at;
  if (colors) {
    CK(d_col.alloc((size_t)N * 24));
    CK(d_ocol.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(d_col.p, colors, (size_t)N * 24, hipMemcpyHostToDevice, s));
    at.col = d_col.as<double>();
    at.out_col = d_ocol.as<double>();
  }
  if (covariances) {
    CK(d_cov.alloc((size_t)N * 72));
    CK(d_ocov.alloc((size_t)N * 72));
    CK(hipMemcpyAsync(d_cov.p, covariances, (size_t)N * 72, hipMemcpyHostToDevice, s));
    at.cov = d_cov.as<double>();
    at.out_cov = d_ocov.as<double>();
  }
  CK(d_opts.alloc((size_t)N * 24));
  CK(d_on.alloc((size_t)N * 24));
  int64_t kept = 0;
  rc = crop_dev(ar, *c, d_pts.as<double>(), normals ? d_nrm.as<double>() : nullptr, N, d_opts.as<double>(), d_on.as<double>(), &kept, s, &at);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(s));
  CK(hipMemcpy(out_pts, d_opts.p, (size_t)kept * 24, hipMemcpyDeviceToHost));
  if (normals) CK(hipMemcpy(out_normals, d_on.p, (size_t)kept * 24, hipMemcpyDeviceToHost));
  if (colors) CK(hipMemcpy(out_colors, d_ocol.p, (size_t)kept * 24, hipMemcpyDeviceToHost));
  if (covariances) CK(hipMemcpy(out_covariances, d_ocov.p, (size_t)kept * 72, hipMemcpyDeviceToHost));
  *n_out = kept;
  return O3S_OK;
}

int o3s_crop(int device, const o3s_cropper* c, const double* pts, const double* normals, int64_t N, double* out_pts, double* out_normals,
             int64_t* n_out) {
  return o3s_crop_attr(device, c, pts, normals, nullptr, nullptr, N, out_pts, out_normals, nullptr, nullptr, n_out);
}

int o3s_voxelize_within_crop_attr(int device, const o3s_cropper* c, double voxel_size, const double* pts, const double* normals,
                                  const double* colors, const double* covariances, int64_t N, double* out_pts, double* out_normals,
                                  double* out_colors, double* out_covariances, int32_t* out_voxel_idx, int64_t* n_out) {
  if (!c || !pts || !out_pts || !n_out || N < 0 || (normals && !out_normals) || (colors && !out_colors) || (covariances && !out_covariances))
    return O3S_ERR_BAD_ARGUMENT;
  if (voxel_size <= 0.0) {  // helpers.cpp:122-125: the cloud is returned unchanged
    std::memcpy(out_pts, pts, (size_t)N * 24);
    if (normals) std::memcpy(out_normals, normals, (size_t)N * 24);
    if (colors) std::memcpy(out_colors, colors, (size_t)N * 24);
    if (covariances) std::memcpy(out_covariances, covariances, (size_t)N * 72);
    if (out_voxel_idx)
      for (int64_t i = 0; i < 3 * N; ++i) out_voxel_idx[i] = INT32_MIN;
    *n_out = N;
    return O3S_OK;
  }
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  return voxel_pipeline(0, c, voxel_size, pts, normals, colors, covariances, N, out_pts, out_normals, out_colors, out_covariances, out_voxel_idx, n_out);
}

int o3s_voxelize_within_crop(int device, const o3s_cropper* c, double voxel_size, const double* pts, const double* normals, int64_t N,
                             double* out_pts, double* out_normals, int32_t* out_voxel_idx, int64_t* n_out) {
  return o3s_voxelize_within_crop_attr(device, c, voxel_size, pts, normals, nullptr, nullptr, N, out_pts, out_normals, nullptr, nullptr,
                                       out_voxel_idx, n_out);
}

int o3s_voxel_downsample_attr(int device, double voxel_size, const double* pts, const double* normals, const double* colors,
                              const double* covariances, int64_t N, double* out_pts, double* out_normals, double* out_colors,
                              double* out_covariances, int32_t* out_voxel_idx, int64_t* n_out) {
  if (!pts || !out_pts || !n_out || N < 0 || !(voxel_size > 0.0) || (normals && !out_normals) || (colors && !out_colors) ||
      (covariances && !out_covariances))
    return O3S_ERR_BAD_ARGUMENT;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  return voxel_pipeline(1, nullptr, voxel_size, pts, normals, colors, covariances, N, out_pts, out_normals, out_colors, out_covariances, out_voxel_idx,
                        n_out);
}

int o3s_voxel_downsample(int device, double voxel_size, const double* pts, const double* normals, int64_t N, double* out_pts,
                         double* out_normals, int32_t* out_voxel_idx, int64_t* n_out) {
  return o3s_voxel_downsample_attr(device, voxel_size, pts, normals, nullptr, nullptr, N, out_pts, out_normals, nullptr, nullptr, out_voxel_idx, n_out);
}

// ConstantVelocityMotionCompensation::undistortInputPointCloud on host buffers (out may alias pts)
int o3s_undistort_cloud(int device, const o3s_motion* m, const double* pts, int64_t N, double* out) {
  if (!motion_valid(m) || N < 0 || (N > 0 && (!pts || !out))) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  if (motion_is_zero(*m)) {  // motion is the identity for every phase: the reference's result is p
    if (out != pts) std::memmove(out, pts, (size_t)N * 24);
    return O3S_OK;
  }
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d;
  CK(d.alloc((size_t)N * 24));
  CK(hipMemcpyAsync(d.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  rc = undistort_dev(d.as<double>(), N, *m, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(out, d.p, (size_t)N * 24, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return O3S_OK;
}

int o3s_motion_from_poses(const double T_start[16], double t_start, const double T_finish[16], double t_finish, o3s_motion* m) {
  if (!T_start || !T_finish || !m) return O3S_ERR_BAD_ARGUMENT;
  motion_from_poses(T_start, t_start, T_finish, t_finish, m);
  return O3S_OK;
}

// ---- include/trajectory/o3s_trajectory.h: the host arithmetic (no device call) ----
int o3s_transform_interpolate(const o3s_stamped_pose* start, const o3s_stamped_pose* end, double t, o3s_stamped_pose* out) {
  if (!start || !end || !out) return O3S_ERR_BAD_ARGUMENT;
  return transform_interpolate(start, end, t, out);
}

int o3s_transform_extrapolate(const o3s_stamped_pose* start, const o3s_stamped_pose* end, double t, o3s_stamped_pose* out) {
  if (!start || !end || !out) return O3S_ERR_BAD_ARGUMENT;
  return transform_extrapolate(start, end, t, out);
}

int o3s_trajectory_has(const o3s_stamped_pose* poses, int64_t K, double t) { return trajectory_has(poses, K, t) ? 1 : 0; }

int o3s_trajectory_lookup(const o3s_stamped_pose* poses, int64_t K, double t, double out_T[16]) {
  if (!out_T) return O3S_ERR_BAD_ARGUMENT;
  return trajectory_lookup(poses, K, t, out_T);
}

int o3s_trajectory_get_transform(const o3s_stamped_pose* poses, int64_t K, double t, double out_T[16]) {
  if (!out_T) return O3S_ERR_BAD_ARGUMENT;
  return trajectory_get_transform(poses, K, t, out_T);
}

// the de-skew along a trajectory on host buffers (out may alias pts)
int o3s_undistort_cloud_trajectory(int device, const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew* params, const double* pts,
                                   const double* dt, int64_t N, double* out) {
  if (!trajectory_call_valid(poses, K, params, dt != nullptr) || N < 0 || (N > 0 && (!pts || !out))) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  if (K == 1) {  // G is the same pose at every stamp: A * G * C^-1 is the identity
    if (out != pts) std::memmove(out, pts, (size_t)N * 24);
    return O3S_OK;
  }
  TrajectoryArgs a;
  std::vector<double> tab;
  int rc = trajectory_prepare(poses, K, *params, &a, &tab);
  if (rc != O3S_OK) return rc;
  rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d, d_dt, d_tab;
  CK(d.alloc((size_t)N * 24));
  CK(d_tab.alloc(tab.size() * 8));
  CK(hipMemcpyAsync(d.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
  if (dt) {
    CK(d_dt.alloc((size_t)N * 8));
    CK(hipMemcpyAsync(d_dt.p, dt, (size_t)N * 8, hipMemcpyHostToDevice, s));
  }
  rc = undistort_trajectory_dev(d.as<double>(), dt ? d_dt.as<double>() : nullptr, N, d_tab.as<double>(), a, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(out, d.p, (size_t)N * 24, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return O3S_OK;
}

}  // extern "C"

#include "o3d_icp_impl.h"
#include "submap_impl.h"
#include "assemble_impl.h"
#include "features_impl.h"
#include "ransac_impl.h"
#include "place_impl.h"
#include "dense_map_impl.h"
#include "overlap_impl.h"
#include "pose_search_impl.h"  // (includes pose_search_dev.h, the kernels)
#include "constraints_impl.h"
#include "outlier_impl.h"  // (includes outlier_dev.h, the kernels)
#include "cluster_impl.h"  // (includes cluster_dev.h, the kernels)
#include "plane_impl.h"    // (includes plane_dev.h, the kernels)
#include "keypoints_impl.h"  // (includes keypoints_dev.h, the kernels)

#ifdef O3S_TEST_HOOKS
// hooks build only (tools/trajectory_deskew_bench.py): the host's share of one trajectory de-skew — A, C^-1, the extrapolation and
// the table of K knots — `reps` times; *ms_per_call is the mean wall time of one
extern "C" int o3s_test_trajectory_prepare(const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew* params, int reps, double* ms_per_call) {
  using namespace o3s_cloud;
  if (!trajectory_call_valid(poses, K, params, false) || reps < 1 || !ms_per_call) return O3S_ERR_BAD_ARGUMENT;
  TrajectoryArgs a;
  std::vector<double> tab;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < reps; ++k) {
    const int rc = trajectory_prepare(poses, K, *params, &a, &tab);
    if (rc != O3S_OK) return rc;
  }
  *ms_per_call = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
  return O3S_OK;
}

// hooks build only (tools/trajectory_deskew_bench.py): the device time of ONE de-skew kernel on the staged sweep, between two HIP
// events on its stream — k_undistort when a motion is given, else k_undistort_trajectory (its table is uploaded before the first
// event).  The sweep is rewritten in place, as by the product entries
extern "C" int o3s_test_deskew_kernel_ms(o3s_raw_scan* r, const o3s_motion* m, const o3s_stamped_pose* poses, int64_t K,
                                         const o3s_trajectory_deskew* params, float* ms) {
  using namespace o3s_cloud;
  if (!r || r->N == 0 || !ms) return O3S_ERR_BAD_ARGUMENT;
  if (m ? !motion_valid(m) : (K < 2 || !trajectory_call_valid(poses, K, params, r->has_times != 0))) return O3S_ERR_BAD_ARGUMENT;
  if (hipSetDevice(r->device) != hipSuccess) return O3S_ERR_HIP;
  TrajectoryArgs a;
  if (!m) {
    std::vector<double> tab;
    const int rc = trajectory_prepare(poses, K, *params, &a, &tab);
    if (rc != O3S_OK) return rc;
    CK(r->traj.ensure(tab.size() * 8, 0, r->stream));
    CK(hipMemcpyAsync(r->traj.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, r->stream));
    CK(hipStreamSynchronize(r->stream));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  CK(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return O3S_ERR_HIP;
  }
  int rc = hipEventRecord(e0, r->stream) == hipSuccess ? O3S_OK : O3S_ERR_HIP;
  if (rc == O3S_OK)
    rc = m ? undistort_dev(r->p.as<double>(), r->N, *m, r->stream)
           : undistort_trajectory_dev(r->p.as<double>(), r->has_times ? r->dt.as<double>() : nullptr, r->N, r->traj.as<double>(), a, r->stream);
  if (rc == O3S_OK && (hipEventRecord(e1, r->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                       hipEventElapsedTime(ms, e0, e1) != hipSuccess))
    rc = O3S_ERR_HIP;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

// hooks build only (tests/test_gpu_cloud_ops.py): the pair sort of the work areas (cloud_dev.h sort_pairs) on host arrays
extern "C" int o3s_test_sort_pairs(int device, const uint64_t* keys, const uint32_t* vals, int64_t n, int end_bit, uint64_t* keys_out, uint32_t* vals_out) {
  using namespace o3s_cloud;
  if (n <= 0 || !keys || !vals || !keys_out || !vals_out) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  DevMem k1, k2, v1, v2, tmp;
  size_t tb = sort_temp_bytes(n);
  CK(k1.alloc((size_t)n * 8));
  CK(k2.alloc((size_t)n * 8));
  CK(v1.alloc((size_t)n * 4));
  CK(v2.alloc((size_t)n * 4));
  CK(tmp.alloc(tb));
  CK(hipMemcpy(k1.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(v1.p, vals, (size_t)n * 4, hipMemcpyHostToDevice));
  CK(sort_pairs(tmp.p, tb, k1.as<uint64_t>(), k2.as<uint64_t>(), v1.as<uint32_t>(), v2.as<uint32_t>(), (size_t)n, end_bit, nullptr));
  CK(hipMemcpy(keys_out, k2.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(vals_out, v2.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return O3S_OK;
}
// hooks build only (tests/test_gpu_cloud_edges.py): the run heads of `n` sorted keys and their exclusive scan, as the voxelisers chain them —
// k_heads, then scan_flags.  with_blk: k_heads leaves its per-block counts in the scan's temp (put_block_count), as the hinted
// pipelines do, and the scan is k_scan_flags_blk; otherwise rocPRIM's scan.  head_out: n words, off_out: n + 1, *count: the total
// as the host receives it (posted, or copied under O3S_NO_MAILBOX)
extern "C" int o3s_test_scan_flags(int device, const uint64_t* keys, int64_t n, uint64_t pass_key, int key_shift, int with_blk, uint32_t* head_out,
                                   uint32_t* off_out, int64_t* count) {
  using namespace o3s_cloud;
  if (n <= 0 || n > (int64_t)0x7fffffff || !keys || !head_out || !off_out || !count || key_shift < 0 || key_shift > 63) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  DevMem d_keys, d_head, d_off, d_tmp;
  const size_t tb = scan_temp_bytes(n);
  CK(d_keys.alloc((size_t)n * 8));
  CK(d_head.alloc((size_t)n * 4));
  CK(d_off.alloc((size_t)(n + 1) * 4));
  CK(d_tmp.alloc(tb));
  CK(hipMemcpy(d_keys.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
  CK(hipMemset(d_off.p, 0xff, (size_t)(n + 1) * 4));
  uint32_t* blk = with_blk ? reinterpret_cast<uint32_t*>(d_tmp.p) : nullptr;
  hipLaunchKernelGGL(k_heads, dim3(nblk(n)), dim3(kB), 0, nullptr, d_keys.as<uint64_t>(), n, pass_key, d_head.as<uint32_t>(), key_shift, blk);
  CK(hipGetLastError());
  const int rs = scan_flags(d_head.as<uint32_t>(), d_off.as<uint32_t>(), n, d_tmp.p, tb, count, nullptr, blk);
  if (rs != O3S_OK) return rs;
  CK(hipMemcpy(head_out, d_head.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(off_out, d_off.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost));
  return O3S_OK;
}
// hooks build only (tests/test_gpu_cloud_ops.py): the bounds of a host cloud through the shared reduction (cloud_bounds.h) — fill,
// k_bounds over the flat source on the production grid, fold and fetch; out6 = min x, y, z, max x, y, z
extern "C" int o3s_test_cloud_bounds(int device, const double* pts, int64_t n, double* out6) {
  using namespace o3s_cloud;
  if (n <= 0 || !pts || !out6) return O3S_ERR_BAD_ARGUMENT;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  DevMem d_pts, d_bb;
  CK(d_pts.alloc((size_t)n * 24));
  CK(d_bb.alloc((size_t)kBoundsWords * 8));
  CK(hipMemcpy(d_pts.p, pts, (size_t)n * 24, hipMemcpyHostToDevice));
  unsigned long long bb[6];
  const int rb = cloud_bounds(FlatPoints{d_pts.as<double>()}, n, d_bb.as<unsigned long long>(), nullptr, bb);
  if (rb != O3S_OK) return rb;
  for (int a = 0; a < 6; ++a) out6[a] = from_ordered_bits(bb[a]);
  return O3S_OK;
}
// hooks build only (tests/test_o3d_update_host.py, tests/test_gpu_registration_edges.py): the host arithmetic of one
// ComputeTransformation of the loop-closure ICP, as o3d_icp_run calls it (o3d_host_update) — type: o3s_o3d_estimation_type, sums: the 30
// sums of a pass, shift: what the point-to-point sums are relative to (else unread, nullable), update: 4 x 4 column-major, x (nullable):
// the solved 6-vector.  Touches no device
extern "C" int o3s_test_o3d_update(int type, const double* sums, const double* shift, double* update, double* x) {
  using namespace o3s_cloud;
  if ((type != kEstPlane && type != kEstPoint && type != kEstGicp) || !sums || !update || (type == kEstPoint && !shift)) return O3S_ERR_BAD_ARGUMENT;
  o3d_host_update(type, sums, shift, update, x);
  return O3S_OK;
}
// hooks build only (tests/test_gpu_registration_edges.py): o3s_o3d_registration_icp_ex up to and including its first pass
// (o3d_icp_setup + one o3d_corr_pass) on host clouds.  sums: the 30 sums; corr: the correspondence of every SOURCE INDEX (the
// device holds them in search order: undone with the work area's `order`); scov / tcov (GICP only, nullable): xx xy xz yy yz zz of
// every source / target point by point index, the source's as placed (untransformed); shift (nullable): the point-to-point shift
extern "C" int o3s_test_o3d_first_pass(int device, const double* source, const double* source_normals, const double* source_cov, int64_t Ns,
                                       const double* target, const double* target_normals, const double* target_cov, int64_t Nt, double max_dist,
                                       const double init[16], const o3s_o3d_estimation* est, double* sums, int32_t* corr, double* scov, double* tcov,
                                       double* shift) {
  using namespace o3s_cloud;
  if (!o3d_est_valid(est) || !sums || !corr) return O3S_ERR_BAD_ARGUMENT;
  O3dEstIn e;
  e.type = est->type;
  e.eps = est->gicp_epsilon;
  e.src_n = source_normals;
  e.src_cov = source_cov;
  e.tgt_cov = target_cov;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  RegLease area(device, nullptr);
  O3dIcpWork& w = area->reg;
  GridIndex gi;
  double Racc[9];
  int r = o3d_icp_setup(w, source, Ns, target, target_normals, Nt, max_dist, init, e, &gi, Racc, nullptr, false, nullptr);
  if (r == O3S_OK) r = o3d_corr_pass(w, Ns, gi, max_dist * max_dist, 0, sums, nullptr);
  if (r != O3S_OK) return area.end(r);
  auto fetch = [&]() -> int {
    const size_t n = (size_t)Ns;
    std::vector<uint32_t> order(n);
    std::vector<int32_t> c(n);
    CK(hipMemcpy(order.data(), w.order, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(c.data(), w.d_corr.p, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) corr[order[i]] = c[i];
    if (e.type == kEstGicp && scov) {
      std::vector<double> sc(6 * n);
      CK(hipMemcpy(sc.data(), w.d_scov.p, 48 * n, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 6; ++k) scov[6 * (size_t)order[i] + k] = sc[6 * i + k];
    }
    if (e.type == kEstGicp && tcov) CK(hipMemcpy(tcov, w.d_tcov.p, 48 * (size_t)Nt, hipMemcpyDeviceToHost));
    if (e.type == kEstPoint && shift)
      for (int a = 0; a < 3; ++a) shift[a] = w.ea.c[a];
    return O3S_OK;
  };
  return area.end(fetch());
}
#endif
