// degeneracy_partial_impl.h — host side of include/degeneracy/o3s_degeneracy_partial.h: included by o3s_icp.hip behind
// degeneracy_impl.h (it uses deg_set_error).  The kernels are the flagged instantiations in localizability_dev.h and
// degeneracy_dev.h; their launches stand in the issue loop (launch_constrain, o3s_icp.hip).
#pragma once
#include "../../include/degeneracy/o3s_degeneracy_partial.h"

namespace {

static_assert(sizeof(kern::DegPartialLast) == sizeof(o3s_degeneracy_partial), "the device's record is the ABI's");

void deg_partial_from(const kern::DegPartialLast& r, o3s_degeneracy_partial* out) {
  std::memset(out, 0, sizeof(*out));
  for (int j = 0; j < 6; ++j) out->num[j] = r.num[j], out->den[j] = r.den[j], out->value[j] = r.value[j], out->category[j] = r.category[j];
  out->partial_mask = (int32_t)r.partial_mask;
  out->constrained_mask = (int32_t)r.constrained_mask;
}

}  // namespace

extern "C" {

int o3s_icp_set_degen_partial(o3s_icp* h, int32_t enable) {
  if (!h || (enable != 0 && enable != 1)) return h ? fail(h, O3S_ERR_BAD_ARGUMENT, "degeneracy partial: enable must be 0 or 1") : O3S_ERR_BAD_ARGUMENT;
  if (enable) {  // here, not inside a compute: an allocation moves alloc_gen (ensure_iteration_buffers)
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->d_degp.ensure(kDegpBufBytes));
  }
  if ((enable != 0) != h->deg_partial) ++h->deg_gen;  // another chain: its graph is another graph
  h->deg_partial = enable != 0;
  h->deg_partial_valid = false;
  return O3S_OK;
}

int o3s_icp_get_degen_partial(o3s_icp* h, int32_t* enabled, o3s_degeneracy_partial* last) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (enabled) *enabled = h->deg_partial ? 1 : 0;
  if (last) {
    kern::DegPartialLast r;
    std::memset(&r, 0, sizeof(r));
    if (h->deg_partial_valid) {
      HIP_TRY(h, hipSetDevice(h->device));
      HIP_TRY(h, hipMemcpyAsync(&r, h->d_degp.as<char>() + kDegpOffLast, sizeof(r), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    deg_partial_from(r, last);
  }
  return O3S_OK;
}

int32_t o3s_icp_degen_partial_trace(o3s_icp* h, int32_t* partial_masks, double* values, int32_t cap) {
  if (!h || !partial_masks || !values || cap <= 0 || !h->deg_partial_valid) return 0;
  const int n = std::min(std::min(h->last_iters, (int)cap), kDegMaskCap);
  if (n <= 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  const char* base = h->d_degp.as<char>();
  if (hipMemcpyAsync(partial_masks, base + kDegpOffMasks, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipMemcpyAsync(values, base + kDegpOffValues, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return 0;
  return n;
}

int o3s_degen_partial_estimate(o3s_icp* h, const float* reading_c, const float* reference_c, const float* normals, int64_t K,
                               const o3s_localizability_params* params, o3s_localizability* loc, o3s_degeneracy_partial* out) {
  if (!reading_c || !reference_c || !normals || !params || !out) return O3S_ERR_BAD_ARGUMENT;
  if (const char* why = loc_params_error(*params)) return h ? fail(h, O3S_ERR_BAD_CONFIG, why) : O3S_ERR_BAD_CONFIG;
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (K <= 0) return fail(h, O3S_ERR_NO_POINTS, "degeneracy partial estimate: no pairs");
  if (K > (int64_t)(1 << 30)) return fail(h, O3S_ERR_BAD_ARGUMENT, "degeneracy partial estimate: more than 2^30 pairs");
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)K * 12;
  HIP_TRY(h, h->d_mod_a.ensure(bytes));
  HIP_TRY(h, h->d_mod_b.ensure(bytes));
  HIP_TRY(h, h->d_mod_c.ensure(bytes));
  HIP_TRY(h, h->d_degp.ensure(kDegpBufBytes));
  h->deg_partial_valid = false;  // k_deg_partial_post leaves this call's record where a compute leaves its last one
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (upload_reading: a copy from pageable memory into a busy stream takes the slow path)
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_a.p, reading_c, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_b.p, reference_c, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_c.p, normals, bytes, hipMemcpyHostToDevice, h->stream));
  kern::DegPartialLast rec;
  o3s_localizability l;
  const int rc = loc_run(h, (int)K, nullptr, nullptr, nullptr, 0.f, h->d_mod_a.as<float>(), h->d_mod_c.as<float>(), *params, &l, h->d_mod_b.as<float>(), &rec);
  if (rc != O3S_OK) return rc;
  if (loc) *loc = l;
  deg_partial_from(rec, out);
  return O3S_OK;
}

int o3s_icp_minimize_degen_values(o3s_icp* h, const float* reading_xyzw, const int32_t* ids, const float* dists2, const float* weights, int64_t N,
                                  const o3s_degeneracy_set* set, const double rot_values[3], const double trans_values[3], float T_out[16],
                                  float A_out[36], float b_out[6], float x_out[6]) {
  kern::DegFixed fixed;
  if (const char* why = deg_set_error(set, &fixed)) return h ? fail(h, O3S_ERR_BAD_ARGUMENT, why) : O3S_ERR_BAD_ARGUMENT;
  double vals[6] = {0, 0, 0, 0, 0, 0};  // the mask's order: translation 0..2, rotation 3..5
  for (int j = 0; j < set->n_trans; ++j)
    if (trans_values) vals[j] = trans_values[j];
  for (int j = 0; j < set->n_rot; ++j)
    if (rot_values) vals[3 + j] = rot_values[j];
  for (int j = 0; j < 6; ++j)
    if (!std::isfinite(vals[j])) return h ? fail(h, O3S_ERR_BAD_ARGUMENT, "degeneracy values: a value is not finite") : O3S_ERR_BAD_ARGUMENT;
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, h->d_deg.ensure(kDegBufBytes));
  h->deg_trace_valid = false;  // k_constrain leaves this call's set where a compute leaves its last one
  const bool plain = !rot_values && !trans_values;  // o3s_icp_minimize_degeneracy itself
  return minimize_impl(h, reading_xyzw, ids, dists2, weights, N, &fixed, plain ? nullptr : vals, T_out, A_out, b_out, x_out);
}

}  // extern "C"
