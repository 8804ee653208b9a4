// pose_search_impl.h — host side and C entry points of the initial pose search (include/pose_search/o3s_pose_search.h).
// Included at the end of cloud_ops.hip behind submap_impl.h (the snapshot it searches is the submap's); the kernels are in pose_search_dev.h.
//
// One call: the yaw rotations (formed here, with libm) go up, k_ps_score writes the P scores, k_ps_peaks marks the eligible poses
// and counts them per score, k_ps_threshold finds the score at which top_k is reached, the poses above it take a slot each, the
// ties at it are ranked in index order by one scan (scan_flags_dev) and the first of them fill the rest, k_ps_finish orders the
// winners.  One small copy brings the result block back; the scores cross the bus only when scores_out is given.
#pragma once
#include "pose_search_dev.h"
#include "submap_impl.h"

#include <cmath>

namespace {
namespace o3s_cloud {

constexpr int64_t kPsMaxPoses = (int64_t)1 << 26, kPsMaxPoints = (int64_t)1 << 20, kPsMaxLookups = (int64_t)1 << 34;
constexpr size_t kPsKeepBytes = (size_t)64 << 20;  // an area that grew beyond this goes back to the allocator behind its call

// work area of one search: n_pts host points staged (0: a resident scan), n_yaw rotations, P scores / flags / offsets,
// the scan's scratch, n_bins histogram words
struct PoseSearchArea {
  static constexpr size_t kSlack = 4096;
  double *pts, *rot;
  uint32_t *scores, *flag, *off;
  char* tmp;
  uint32_t* hist;
  PsSelect* sel;
  template <class A>
  void lay(A& a, size_t n_pts, size_t n_yaw, size_t P, size_t tb_scan, size_t n_bins) {
    take(a, pts, 3 * n_pts);
    take(a, rot, 9 * n_yaw);
    take(a, scores, P);
    take(a, flag, P);
    take(a, off, P + 1);
    take(a, tmp, tb_scan);
    take(a, hist, n_bins);
    take(a, sel, 1);
  }
};
struct PoseSearchWork {
  Arena arena;
};
using PoseSearchLease = AreaLease<PoseSearchWork, /*kAlwaysDrain=*/true>;

// P, or -1 for parameters the search refuses
inline int64_t ps_count(const o3s_pose_search_params* p) {
  if (!p) return -1;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(p->center[k])) return -1;
  if (!std::isfinite(p->step_xy) || !std::isfinite(p->step_z) || !std::isfinite(p->step_yaw) || !std::isfinite(p->yaw0)) return -1;
  const int32_t H = O3S_POSE_SEARCH_MAX_HALF_WIDTH;
  if (p->n_x < 0 || p->n_x > H || p->n_y < 0 || p->n_y > H || p->n_z < 0 || p->n_z > H) return -1;
  if (p->n_yaw < 1 || p->n_yaw > O3S_POSE_SEARCH_MAX_YAWS) return -1;
  if ((p->n_x > 0 || p->n_y > 0) && !(p->step_xy > 0.0)) return -1;
  if (p->n_z > 0 && !(p->step_z > 0.0)) return -1;
  if (p->n_yaw > 1 && !(p->step_yaw > 0.0)) return -1;
  if (p->point_stride < 1 || p->top_k < 1 || p->top_k > kPsMaxTopK) return -1;
  if ((p->yaw_ring != 0 && p->yaw_ring != 1) || (p->local_maxima != 0 && p->local_maxima != 1)) return -1;
  const int64_t P = (int64_t)(2 * p->n_x + 1) * (2 * p->n_y + 1) * (2 * p->n_z + 1) * p->n_yaw;  // < 2^13 * 2^13 * 2^13 * 2^16
  return P > kPsMaxPoses ? -1 : P;
}
// R = Rz(psi_l) R_c, row-major
inline void ps_rotation(const o3s_pose_search_params* p, int64_t l, double R[9]) {
  const double psi = p->yaw0 + (double)l * p->step_yaw;
  const double c = std::cos(psi), s = std::sin(psi);
  for (int col = 0; col < 3; ++col) {
    const double r0 = p->center[4 * col], r1 = p->center[4 * col + 1], r2 = p->center[4 * col + 2];
    const double a = c * r0, b = s * r1, d = s * r0, e = c * r1;
    R[col] = a - b;
    R[3 + col] = d + e;
    R[6 + col] = r2;
  }
}

// everything that can be refused is refused here: P, the counted points M
inline int ps_front(const o3s_submap* m, int64_t N, const o3s_pose_search_params* p, const o3s_pose_search_result* result, int64_t* P, int64_t* M) {
  if (!m || !p || !result || N < 0) return O3S_ERR_BAD_ARGUMENT;
  *P = ps_count(p);
  if (*P < 0 || N > kPsMaxPoints) return O3S_ERR_BAD_ARGUMENT;
  *M = (N + p->point_stride - 1) / p->point_stride;
  if (*M > 0 && *P > kPsMaxLookups / *M) return O3S_ERR_BAD_ARGUMENT;
  return O3S_OK;
}

// d_pts: the points on the device, or null with h_pts the host points to stage (N > 0); everything runs on m's stream
int ps_run(const o3s_submap* m, const double* d_pts, const double* h_pts, int64_t N, const o3s_pose_search_params* p, int64_t P, int64_t M,
           o3s_pose_search_result* result, uint32_t* scores_out) {
  hipStream_t s = m->stream;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, m->device) != hipSuccess || khz <= 0) khz = 100000;
  PsGrid g;
  for (int a = 0; a < 3; ++a) g.tc[a] = p->center[12 + a];
  g.step_xy = p->step_xy;
  g.step_z = p->step_z;
  g.nx = p->n_x;
  g.ny = p->n_y;
  g.nz = p->n_z;
  g.cx = 2 * p->n_x + 1;
  g.cy = 2 * p->n_y + 1;
  g.cz = 2 * p->n_z + 1;
  g.cl = p->n_yaw;
  g.tiles_x = (g.cx + kPsTile - 1) / kPsTile;
  g.tiles_y = (g.cy + kPsTile - 1) / kPsTile;
  g.ring = (p->yaw_ring && p->n_yaw >= 3) ? 1 : 0;
  const size_t n_bins = (size_t)M + 1;  // a score is at most M
  const size_t tb_scan = scan_temp_bytes(P);
  std::vector<double> rot((size_t)p->n_yaw * 9);
  for (int64_t l = 0; l < p->n_yaw; ++l) ps_rotation(p, l, rot.data() + 9 * l);

  PoseSearchLease area(m->device, s);
  PoseSearchArea a;
  CK(lay_out(area->arena, a, h_pts ? (size_t)N : (size_t)0, (size_t)p->n_yaw, (size_t)P, tb_scan, n_bins));
  struct Shrink {  // (declared behind the lease: runs first, and drains the stream before the block goes)
    PoseSearchLease& l;
    ~Shrink() {
      if (l->arena.mem.cap > kPsKeepBytes) {
        (void)hipStreamSynchronize(l.s);
        l->arena.release();
      }
    }
  } shrink{area};
  if (h_pts) {
    CK(hipMemcpyAsync(a.pts, h_pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
    d_pts = a.pts;
  }
  CK(hipMemcpyAsync(a.rot, rot.data(), rot.size() * 8, hipMemcpyHostToDevice, s));
  CK(hipMemsetAsync(a.hist, 0, n_bins * 4, s));
  CK(hipMemsetAsync(a.sel, 0, sizeof(PsSelect), s));
  const int64_t n_blocks = (int64_t)g.tiles_x * g.tiles_y * g.cz * g.cl;  // <= P <= 2^26
  hipLaunchKernelGGL(k_ps_score, dim3((unsigned)n_blocks), dim3(kB), 0, s, d_pts, M, (int64_t)p->point_stride, (const double*)a.rot, g, 1.0 / m->vox_size,
                     reinterpret_cast<const unsigned long long*>(m->vox_tab.p), m->vox_slots - 1u, a.scores, a.sel);
  hipLaunchKernelGGL(k_ps_peaks, dim3(nblk(P)), dim3(kB), 0, s, (const uint32_t*)a.scores, P, g, (int)p->local_maxima, p->min_score, a.flag, a.hist,
                     (uint32_t)n_bins);
  hipLaunchKernelGGL(k_ps_threshold, dim3(1), dim3(kB), 0, s, (const uint32_t*)a.hist, (uint32_t)n_bins, p->min_score, (uint32_t)p->top_k, a.sel);
  hipLaunchKernelGGL(k_ps_ties, dim3(nblk(P)), dim3(kB), 0, s, (const uint32_t*)a.scores, P, a.flag, a.sel);
  CK(hipGetLastError());
  if (const int rc = scan_flags_dev(a.flag, a.off, P, a.tmp, tb_scan, s); rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_ps_take_ties, dim3(nblk(P)), dim3(kB), 0, s, (const uint32_t*)a.scores, P, (const uint32_t*)a.flag, (const uint32_t*)a.off, a.sel);
  hipLaunchKernelGGL(k_ps_finish, dim3(1), dim3(64), 0, s, a.sel);
  CK(hipGetLastError());
  PsSelect h;
  CK(hipMemcpyAsync(&h, a.sel, sizeof(PsSelect), hipMemcpyDeviceToHost, s));
  std::vector<uint32_t> sc;  // the caller's array is written only by a call that succeeds
  if (scores_out) {
    sc.resize((size_t)P);
    CK(hipMemcpyAsync(sc.data(), a.scores, (size_t)P * 4, hipMemcpyDeviceToHost, s));
  }
  CK(hipStreamSynchronize(s));
  if (h.n_found > (uint32_t)p->top_k) return O3S_ERR_HIP;
  o3s_pose_search_result r;
  std::memset(&r, 0, sizeof(r));
  r.n_poses = P;
  r.n_found = (int32_t)h.n_found;
  r.n_points_counted = M;
  for (int k = 0; k < kPsMaxTopK; ++k) {
    const bool on = k < r.n_found;
    r.index[k] = on ? (int64_t)(0xffffffffu - (uint32_t)(h.cand[k] & 0xffffffffull)) : -1;
    r.score[k] = on ? (int64_t)(h.cand[k] >> 32) : 0;
  }
  r.gpu_ms = h.t_end > h.t_start ? (float)((double)(h.t_end - h.t_start) / (double)khz) : 0.f;
  *result = r;
  if (scores_out) std::memcpy(scores_out, sc.data(), (size_t)P * 4);
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace

extern "C" {

void o3s_pose_search_default_params(o3s_pose_search_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->center[0] = p->center[5] = p->center[10] = p->center[15] = 1.0;
  p->step_xy = 0.5;
  p->step_z = 0.5;
  p->step_yaw = 5.0 * 3.14159265358979323846 / 180.0;
  p->yaw0 = 0.0;
  p->n_x = p->n_y = 8;
  p->n_z = 0;
  p->n_yaw = 72;
  p->yaw_ring = 1;
  p->point_stride = 1;
  p->local_maxima = 1;
  p->top_k = 8;
  p->min_score = 1;
}

int64_t o3s_pose_search_count(const o3s_pose_search_params* p) { return o3s_cloud::ps_count(p); }

int o3s_pose_search_pose(const o3s_pose_search_params* p, int64_t index, double T_out[16]) {
  using namespace o3s_cloud;
  const int64_t P = ps_count(p);
  if (P < 0 || !T_out || index < 0 || index >= P) return O3S_ERR_BAD_ARGUMENT;
  const int64_t cx = 2 * p->n_x + 1, cy = 2 * p->n_y + 1, cz = 2 * p->n_z + 1;
  const int64_t i = index % cx, j = index / cx % cy, k = index / (cx * cy) % cz, l = index / (cx * cy * cz);
  double R[9];
  ps_rotation(p, l, R);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T_out[4 * c + r] = R[3 * r + c];
  T_out[3] = T_out[7] = T_out[11] = 0.0;
  const double ox = (double)(i - p->n_x) * p->step_xy, oy = (double)(j - p->n_y) * p->step_xy, oz = (double)(k - p->n_z) * p->step_z;
  T_out[12] = p->center[12] + ox;
  T_out[13] = p->center[13] + oy;
  T_out[14] = p->center[14] + oz;
  T_out[15] = 1.0;
  return O3S_OK;
}

int o3s_submap_pose_search(const o3s_submap* m, const double* pts, int64_t N, const o3s_pose_search_params* p, o3s_pose_search_result* result,
                           uint32_t* scores_out) {
  using namespace o3s_cloud;
  int64_t P = 0, M = 0;
  if (const int rc = ps_front(m, N, p, result, &P, &M); rc != O3S_OK) return rc;
  if (N > 0 && !pts) return O3S_ERR_BAD_ARGUMENT;
  if (m->n_vox < 0) return O3S_ERR_NOT_INITIALIZED;
  if (const int rc = set_dev(m); rc != O3S_OK) return rc;
  return ps_run(m, nullptr, N > 0 ? pts : nullptr, N, p, P, M, result, scores_out);
}

int o3s_submap_pose_search_scan(const o3s_submap* m, const struct o3s_scan* scan, int which, const o3s_pose_search_params* p,
                                o3s_pose_search_result* result, uint32_t* scores_out) {
  using namespace o3s_cloud;
  if (!scan || (which != 0 && which != 1)) return O3S_ERR_BAD_ARGUMENT;
  const int64_t N = which == 0 ? scan->n_wide : scan->n_narrow;
  int64_t P = 0, M = 0;
  if (const int rc = ps_front(m, N, p, result, &P, &M); rc != O3S_OK) return rc;
  if (m->device != scan->device) return O3S_ERR_BAD_ARGUMENT;
  if (m->n_vox < 0) return O3S_ERR_NOT_INITIALIZED;
  if (const int rc = set_dev(m); rc != O3S_OK) return rc;
  if (scan->stream != m->stream) {  // the scan's clouds are complete before the search reads them
    CK(hipEventRecord(scan->handover, scan->stream));
    CK(hipStreamWaitEvent(m->stream, scan->handover, 0));
  }
  return ps_run(m, (which == 0 ? scan->wide_p : scan->narrow_p).as<double>(), nullptr, N, p, P, M, result, scores_out);  // blocking: the scan may be refilled
}

}  // extern "C"
