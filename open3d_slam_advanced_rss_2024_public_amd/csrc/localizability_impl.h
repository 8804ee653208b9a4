// localizability_impl.h — host side of include/localizability/o3s_localizability.h: included by o3s_icp.hip behind the definition
// of the o3s_icp handle and its helpers (fail, HIP_TRY, nblocks).  The kernels are in localizability_dev.h.
#pragma once
#include "../../include/localizability/o3s_localizability.h"

namespace {

const char* loc_params_error(const o3s_localizability_params& p) {
  if (!(p.filter_min >= 0.0 && p.filter_min <= p.strong_min && p.strong_min <= 1.0)) return "localizability: 0 <= filter_min <= strong_min <= 1 does not hold";
  if (!(std::isfinite(p.sum_all_min) && std::isfinite(p.sum_strong_min) && std::isfinite(p.sum_partial_min)))
    return "localizability: sum_all_min, sum_strong_min and sum_partial_min have no default: calibrate and set them";
  if (!(p.sum_all_min >= p.sum_strong_min && p.sum_strong_min >= p.sum_partial_min && p.sum_partial_min >= 0.0))
    return "localizability: sum_all_min >= sum_strong_min >= sum_partial_min >= 0 does not hold";
  return nullptr;
}

// the four launches on the handle's stream and the wait for k_loc_post's values.  ext_*: the module-level source (device, 3 x n AoS)
int loc_run(o3s_icp* h, int n, const float* rx, const float* ry, const float* rz, float max_out_r2, const float* ext_p, const float* ext_n,
            const o3s_localizability_params& p, o3s_localizability* out, const float* ext_q = nullptr, kern::DegPartialLast* partial = nullptr) {
  const int nb = loc_blocks(n);
  HIP_TRY(h, h->d_loc.ensure(kLocBufBytes));
  double* base = h->d_loc.as<double>();
  double *part1 = base, *dirs = base + kLocOffDirs, *part2 = base + kLocOffPart2, *vals = base + kLocOffOut;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base + kLocOffCnt);
  unsigned long long* t_start = reinterpret_cast<unsigned long long*>(base + kLocOffStart);
  const IcpState* st = ext_p ? nullptr : h->d_state.as<IcpState>();
  const kern::LocThresholds th{p.filter_min, p.strong_min, p.sum_all_min, p.sum_strong_min, p.sum_partial_min};
  hipLaunchKernelGGL(kern::k_loc_hessian, dim3(nb), dim3(kern::kBlock), 0, h->stream, rx, ry, rz, n, h->d_mn.as<float4>(), h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), max_out_r2, h->d_state.as<IcpState>(), ext_p, ext_n, part1, t_start, 0);
  hipLaunchKernelGGL(kern::k_loc_eig, dim3(1), dim3(kern::kBlock), 0, h->stream, part1, nb, dirs, (const IcpState*)nullptr);
  if (partial) {  // the module-level source with its matched points (degeneracy_partial_impl.h): pass 2 flagged, the caller has sized d_degp
    const kern::LocPartialIo pio{nullptr, ext_q, h->d_degp.as<double>()};
    hipLaunchKernelGGL(kern::k_loc_contrib_partial, dim3(nb), dim3(kern::kBlock), 0, h->stream, rx, ry, rz, n, h->d_mn.as<float4>(),
                       h->d_pos.as<int32_t>(), h->d_d2.as<float>(), max_out_r2, h->d_state.as<IcpState>(), ext_p, ext_n, dirs, p.filter_min,
                       p.strong_min, part2, cnt, 0, pio);
  } else {
    hipLaunchKernelGGL(kern::k_loc_contrib, dim3(nb), dim3(kern::kBlock), 0, h->stream, rx, ry, rz, n, h->d_mn.as<float4>(), h->d_pos.as<int32_t>(),
                       h->d_d2.as<float>(), max_out_r2, h->d_state.as<IcpState>(), ext_p, ext_n, dirs, p.filter_min, p.strong_min, part2, cnt, 0);
  }
  const uint32_t seq = h->cov_mb.next();
  hipLaunchKernelGGL(kern::k_loc_post, dim3(1), dim3(kern::kBlock), 0, h->stream, part2, cnt, nb, dirs, th, st, t_start, vals, h->cov_mb.dev, seq);
  if (partial) {
    kern::DegPartialLast* rec = reinterpret_cast<kern::DegPartialLast*>(h->d_degp.as<char>() + kDegpOffLast);
    hipLaunchKernelGGL(kern::k_deg_partial_post, dim3(1), dim3(kern::kBlock), 0, h->stream, h->d_degp.as<double>(), nb, vals, rec);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(partial, rec, sizeof(*partial), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  HIP_TRY(h, hipGetLastError());
  double v[kern::kLocPostVals];
  const int w = host_post::fetch_post(h->cov_mb, seq, h->stream, reinterpret_cast<uint32_t*>(v), 2 * kern::kLocPostVals, host_post::kPostVals, vals);
  if (w == host_post::kPollError) return fail(h, O3S_ERR_HIP, "localizability: the kernels failed");
  o3s_localizability r;
  std::memset(&r, 0, sizeof(r));
  const double* q = v;
  for (int j = 0; j < 6; ++j) r.eval[j] = *q++;
  for (int j = 0; j < 6; ++j)
    for (int c = 0; c < 3; ++c) r.evec[j][c] = *q++;
  for (int j = 0; j < 6; ++j) r.sum_all[j] = *q++;
  for (int j = 0; j < 6; ++j) r.sum_strong[j] = *q++;
  long long iv;
  for (int j = 0; j < 6; ++j) std::memcpy(&iv, q++, 8), r.n_strong[j] = iv;
  for (int j = 0; j < 6; ++j) std::memcpy(&iv, q++, 8), r.category[j] = (int32_t)iv;
  std::memcpy(&iv, q++, 8), r.kept = iv;
  for (int c = 0; c < 3; ++c) r.centre[c] = *q++ + (ext_p ? 0.0 : (double)h->mean[c]);  // <refMean> -> the reference cloud's own frame
  unsigned long long t0, t1;
  std::memcpy(&t0, q++, 8);
  std::memcpy(&t1, q++, 8);
  if (t1 > t0) r.gpu_ms = (float)((double)(t1 - t0) / h->wall_clock_khz);
  if (r.kept == 0) {  // nothing to analyse: all zeros (the sums are; the directions of a zero matrix mean nothing)
    const float ms = r.gpu_ms;
    std::memset(&r, 0, sizeof(r));
    r.gpu_ms = ms;
  }
  *out = r;
  return O3S_OK;
}

// ---- column-major 4 x 4 in fp64 ----------------------------------------------------------------------------------------------
inline double& LM(double* T, int r, int c) { return T[c * 4 + r]; }
inline double LMc(const double* T, int r, int c) { return T[c * 4 + r]; }
void loc_mul4(const double* A, const double* B, double* C) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += LMc(A, r, k) * LMc(B, k, c);
      LM(C, r, c) = s;
    }
}

}  // namespace

extern "C" {

void o3s_localizability_default_params(o3s_localizability_params* p) {
  if (!p) return;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  p->filter_min = 0.17364817766693041;  // cos 80 deg
  p->strong_min = 0.81915204428899180;  // cos 35 deg
  p->sum_all_min = p->sum_strong_min = p->sum_partial_min = nan;
}

int o3s_icp_localizability(o3s_icp* h, const o3s_localizability_params* params, o3s_localizability* out) {
  if (!params || !out) return O3S_ERR_BAD_ARGUMENT;
  if (const char* why = loc_params_error(*params)) return h ? fail(h, O3S_ERR_BAD_CONFIG, why) : O3S_ERR_BAD_CONFIG;  // (the parameters first: a caller
  if (!h) return O3S_ERR_BAD_ARGUMENT;                                                                                //  can check them without a device)
  if (h->shard.active) return fail(h, O3S_ERR_BAD_CONFIG, "the localizability analysis is not available in the sharded mode");
  if (!h->cov_valid || !h->elements_valid || h->prepared_N <= 0)
    return fail(h, O3S_ERR_NOT_INITIALIZED, "localizability: no successful compute on this handle whose pairs are still resident");
  HIP_TRY(h, hipSetDevice(h->device));
  const int N = h->prepared_N;
  const float* r = h->d_r.as<float>();
  return loc_run(h, N, r, r + (size_t)N, r + 2 * (size_t)N, h->last_max_out_r2, nullptr, nullptr, *params, out);
}

int o3s_localizability_estimate(o3s_icp* h, const float* reading_c, const float* normals, int64_t K, const o3s_localizability_params* params,
                                o3s_localizability* out) {
  if (!reading_c || !normals || !params || !out) return O3S_ERR_BAD_ARGUMENT;
  if (const char* why = loc_params_error(*params)) return h ? fail(h, O3S_ERR_BAD_CONFIG, why) : O3S_ERR_BAD_CONFIG;
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (K <= 0) return fail(h, O3S_ERR_NO_POINTS, "localizability_estimate: no pairs");
  if (K > (int64_t)(1 << 30)) return fail(h, O3S_ERR_BAD_ARGUMENT, "localizability_estimate: more than 2^30 pairs");
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)K * 12;
  HIP_TRY(h, h->d_mod_a.ensure(bytes));
  HIP_TRY(h, h->d_mod_c.ensure(bytes));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (upload_reading: a copy from pageable memory into a busy stream takes the slow path)
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_a.p, reading_c, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_c.p, normals, bytes, hipMemcpyHostToDevice, h->stream));
  return loc_run(h, (int)K, nullptr, nullptr, nullptr, 0.f, h->d_mod_a.as<float>(), h->d_mod_c.as<float>(), *params, out);
}

int o3s_localizability_remap(const o3s_localizability* loc, int32_t min_category, const double T_prior[16], const double T_icp[16], double T_out[16],
                             int32_t* n_replaced) {
  if (!loc || !T_prior || !T_icp || !T_out) return O3S_ERR_BAD_ARGUMENT;
  if (min_category != 1 && min_category != 2) return O3S_ERR_BAD_ARGUMENT;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(T_prior[k]) || !std::isfinite(T_icp[k])) return O3S_ERR_BAD_ARGUMENT;
  int32_t replaced = 0;
  for (int j = 0; j < 6; ++j) replaced += loc->category[j] < min_category ? 1 : 0;
  if (replaced == 0) {  // every direction keeps the ICP's correction: the pose itself, not a recomputation of it
    double keep[16];
    std::memcpy(keep, T_icp, sizeof(keep));
    std::memcpy(T_out, keep, sizeof(keep));
    if (n_replaced) *n_replaced = 0;
    return O3S_OK;
  }
  // dT = T_icp . T_prior^-1: the inverse of the affine [A, t] itself (cofactors), not [A^T, -A^T t] — a prior that went through
  // fp32 is orthonormal to 1e-7 only, and dT . T_prior has to give T_icp back
  double Pinv[16] = {0}, dT[16];
  {
    const double a = LMc(T_prior, 0, 0), b = LMc(T_prior, 0, 1), c = LMc(T_prior, 0, 2), d = LMc(T_prior, 1, 0), e = LMc(T_prior, 1, 1),
                 f = LMc(T_prior, 1, 2), g = LMc(T_prior, 2, 0), h = LMc(T_prior, 2, 1), i = LMc(T_prior, 2, 2);
    const double co[3][3] = {{e * i - f * h, c * h - b * i, b * f - c * e}, {f * g - d * i, a * i - c * g, c * d - a * f}, {d * h - e * g, b * g - a * h, a * e - b * d}};
    const double det = (a * co[0][0] + b * co[1][0]) + c * co[2][0];
    if (!(std::fabs(det) > 0.0) || !std::isfinite(1.0 / det)) return O3S_ERR_BAD_ARGUMENT;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) LM(Pinv, r, k) = co[r][k] / det;
      LM(Pinv, r, 3) = -((LMc(Pinv, r, 0) * LMc(T_prior, 0, 3) + LMc(Pinv, r, 1) * LMc(T_prior, 1, 3)) + LMc(Pinv, r, 2) * LMc(T_prior, 2, 3));
    }
  }
  LM(Pinv, 3, 3) = 1.0;
  loc_mul4(T_icp, Pinv, dT);
  const double* m = loc->centre;
  double u[3], a[3], rv[3] = {0, 0, 0};
  for (int r = 0; r < 3; ++r) u[r] = (((LMc(dT, r, 0) * m[0] + LMc(dT, r, 1) * m[1]) + LMc(dT, r, 2) * m[2]) + LMc(dT, r, 3)) - m[r];
  a[0] = 0.5 * (LMc(dT, 2, 1) - LMc(dT, 1, 2));
  a[1] = 0.5 * (LMc(dT, 0, 2) - LMc(dT, 2, 0));
  a[2] = 0.5 * (LMc(dT, 1, 0) - LMc(dT, 0, 1));
  const double na = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  const double theta = std::atan2(na, (((LMc(dT, 0, 0) + LMc(dT, 1, 1)) + LMc(dT, 2, 2)) - 1.0) / 2.0);
  if (!(theta < 1.5707963267948966)) return O3S_ERR_BAD_ARGUMENT;  // not a correction one may linearise
  if (na > 0.0)
    for (int c = 0; c < 3; ++c) rv[c] = (theta / na) * a[c];
  double up[3] = {0, 0, 0}, rp[3] = {0, 0, 0};
  for (int j = 0; j < 6; ++j) {
    if (loc->category[j] < min_category) continue;
    const double* d = loc->evec[j];
    const double* src = j < 3 ? u : rv;
    double* dst = j < 3 ? up : rp;
    const double s = (d[0] * src[0] + d[1] * src[1]) + d[2] * src[2];
    for (int c = 0; c < 3; ++c) dst[c] += s * d[c];
  }
  // exp(r') by Rodrigues' formula
  double E[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const double phi = std::sqrt((rp[0] * rp[0] + rp[1] * rp[1]) + rp[2] * rp[2]);
  if (phi > 0.0) {
    const double k[3] = {rp[0] / phi, rp[1] / phi, rp[2] / phi};
    const double K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
    const double s = std::sin(phi), c1 = 1.0 - std::cos(phi);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double k2 = 0.0;
        for (int t = 0; t < 3; ++t) k2 += K[r][t] * K[t][c];
        E[r][c] += s * K[r][c] + c1 * k2;
      }
  }
  double corr[16] = {0}, res[16];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) LM(corr, r, c) = E[r][c];
    LM(corr, r, 3) = (m[r] + up[r]) - ((E[r][0] * m[0] + E[r][1] * m[1]) + E[r][2] * m[2]);
  }
  LM(corr, 3, 3) = 1.0;
  loc_mul4(corr, T_prior, res);
  std::memcpy(T_out, res, sizeof(res));
  if (n_replaced) *n_replaced = replaced;
  return O3S_OK;
}

}  // extern "C"
