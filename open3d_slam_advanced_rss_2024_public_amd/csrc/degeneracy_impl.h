// degeneracy_impl.h — host side of include/degeneracy/o3s_degeneracy.h: included by o3s_icp.hip behind localizability_impl.h (it
// uses loc_params_error).  The kernel is in degeneracy_dev.h; its launches stand in the issue loop (launch_constrain, o3s_icp.hip).
#pragma once
#include "../../include/degeneracy/o3s_degeneracy.h"

namespace {

// a set the contract refuses: null; else the caller's set as k_constrain takes it (the mask's order: translation 0..2, rotation 3..5)
const char* deg_set_error(const o3s_degeneracy_set* s, kern::DegFixed* out) {
  if (!s) return "degeneracy: no set";
  if (s->n_rot < 0 || s->n_rot > 3 || s->n_trans < 0 || s->n_trans > 3) return "degeneracy: n_rot and n_trans must be 0..3";
  kern::DegFixed f;
  std::memset(&f, 0, sizeof(f));
  for (int g = 0; g < 2; ++g) {
    const int n = g ? s->n_rot : s->n_trans;
    const double(*d)[3] = g ? s->rot : s->trans;
    for (int j = 0; j < n; ++j) {
      for (int c = 0; c < 3; ++c)
        if (!std::isfinite(d[j][c])) return "degeneracy: a direction is not finite";
      for (int k = 0; k <= j; ++k) {
        const double dot = (d[j][0] * d[k][0] + d[j][1] * d[k][1]) + d[j][2] * d[k][2];
        if (!(std::fabs(dot - (k == j ? 1.0 : 0.0)) <= 1e-9)) return "degeneracy: the directions of a group must be unit and mutually orthogonal to 1e-9";
      }
      for (int c = 0; c < 3; ++c) f.dir[3 * g + j][c] = d[j][c];
      f.mask |= 1u << (3 * g + j);
    }
  }
  if (out) *out = f;
  return nullptr;
}

}  // namespace

extern "C" {

void o3s_degeneracy_default_config(o3s_degeneracy_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->mode = O3S_DEGENERACY_OFF;
  c->min_category = 2;
  o3s_localizability_default_params(&c->loc_params);
}

int o3s_icp_set_degeneracy(o3s_icp* h, int32_t mode, const o3s_degeneracy_set* fixed_set, const o3s_localizability_params* loc_params,
                           int32_t min_category) {
  o3s_degeneracy_config next;
  o3s_degeneracy_default_config(&next);
  kern::DegFixed fixed;
  std::memset(&fixed, 0, sizeof(fixed));
  next.mode = mode;
  if (mode == O3S_DEGENERACY_FIXED) {  // the arguments first: a caller can check them without a device
    if (const char* why = deg_set_error(fixed_set, &fixed)) return h ? fail(h, O3S_ERR_BAD_ARGUMENT, why) : O3S_ERR_BAD_ARGUMENT;
    next.fixed_set = *fixed_set;
  } else if (mode == O3S_DEGENERACY_ANALYSE) {
    if (!loc_params || (min_category != 1 && min_category != 2))
      return h ? fail(h, O3S_ERR_BAD_ARGUMENT, "degeneracy: ANALYSE needs the localizability parameters and min_category 1 or 2") : O3S_ERR_BAD_ARGUMENT;
    if (const char* why = loc_params_error(*loc_params)) return h ? fail(h, O3S_ERR_BAD_CONFIG, why) : O3S_ERR_BAD_CONFIG;
    next.loc_params = *loc_params;
    next.min_category = min_category;
  } else if (mode != O3S_DEGENERACY_OFF) {
    return h ? fail(h, O3S_ERR_BAD_ARGUMENT, "degeneracy: unknown mode") : O3S_ERR_BAD_ARGUMENT;
  }
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (mode != O3S_DEGENERACY_OFF) {  // here, not inside a compute: an allocation moves alloc_gen (ensure_iteration_buffers)
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->d_deg.ensure(kDegBufBytes));
    if (mode == O3S_DEGENERACY_ANALYSE) HIP_TRY(h, h->d_loc.ensure(kLocBufBytes));
  }
  if (std::memcmp(&next, &h->deg, sizeof(next)) != 0) ++h->deg_gen;  // another chain: its graph is another graph
  h->deg = next;
  h->deg_fixed = fixed;
  h->deg_trace_valid = h->deg_partial_valid = false;
  return O3S_OK;
}

int o3s_icp_get_degeneracy(o3s_icp* h, o3s_degeneracy_config* out, o3s_degeneracy_set* last_set) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (out) *out = h->deg;
  if (last_set) {
    o3s_degeneracy_set r;
    std::memset(&r, 0, sizeof(r));
    if (h->deg_trace_valid) {
      kern::DegLast last;
      HIP_TRY(h, hipSetDevice(h->device));
      HIP_TRY(h, hipMemcpyAsync(&last, h->d_deg.p, sizeof(last), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      for (int j = 0; j < 3; ++j) {  // packed in the mask's order
        if (last.mask & (1u << j)) std::memcpy(r.trans[r.n_trans++], last.dir[j], sizeof(last.dir[j]));
        if (last.mask & (8u << j)) std::memcpy(r.rot[r.n_rot++], last.dir[3 + j], sizeof(last.dir[j]));
      }
    }
    *last_set = r;
  }
  return O3S_OK;
}

int32_t o3s_icp_degeneracy_trace(o3s_icp* h, int32_t* masks, int32_t cap) {
  if (!h || !masks || cap <= 0 || !h->deg_trace_valid) return 0;
  const int n = std::min(std::min(h->last_iters, (int)cap), kDegMaskCap);
  if (n <= 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (hipMemcpyAsync(masks, h->d_deg.as<char>() + sizeof(kern::DegLast), (size_t)n * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return 0;
  return n;
}

int o3s_icp_minimize_degeneracy(o3s_icp* h, const float* reading_xyzw, const int32_t* ids, const float* dists2, const float* weights, int64_t N,
                                const o3s_degeneracy_set* set, float T_out[16], float A_out[36], float b_out[6], float x_out[6]) {
  kern::DegFixed fixed;
  if (const char* why = deg_set_error(set, &fixed)) return h ? fail(h, O3S_ERR_BAD_ARGUMENT, why) : O3S_ERR_BAD_ARGUMENT;
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, h->d_deg.ensure(kDegBufBytes));
  h->deg_trace_valid = false;  // k_constrain leaves this call's set where a compute leaves its last one
  return minimize_impl(h, reading_xyzw, ids, dists2, weights, N, &fixed, nullptr, T_out, A_out, b_out, x_out);
}

}  // extern "C"
