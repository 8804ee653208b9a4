// pose_search_dev.h — kernels of the initial pose search (include/pose_search/o3s_pose_search.h); gfx950 only.  Included at the
// end of cloud_ops.hip.  The voxel key (vm_key's arithmetic, field by field: dm_field) and the hash (ov_hash) are voxel_table.h's
// and the isometry arithmetic is k_vm_count's (overlap_impl.h, of which nothing is used here), so the score of a pose is the count
// k_vm_count gives for it, bit for bit.
//
// k_ps_score is the hot kernel: P poses x M points lookups into the snapshot table, which is small (77 k voxels: 2 MB) and stays
// in L2, so the kernel is bound by dependent lookups, not by bandwidth.  Its shape:
//   - A block owns a tile of kPsTile x kPsTile xy cells of ONE yaw and ONE z cell outright and walks all points: no atomics,
//     no reduction between blocks, one plain store per pose — the scores cannot depend on a run-time order.
//   - A lane takes one point at a time.  The rotated part s = (R0 x + R1 y) + R2 z depends on (yaw, point) only and is formed
//     once; q = s + t is the last operation for every translation, as the contract has it.  floor(q * inv) separates per axis:
//     the x parts of the key are formed once per point for the kPsTile columns, the y part once per row, the z part once.
//   - The kPsTile lookups of a row are independent: their first probes are issued together, and the (common: the table is at up
//     to half load) later probes go round by round with every open lookup of the row in flight.  The probe bound is k_vm_count's.
//   - A pose's hits are a ballot; its population count goes into a register of the lane that owns the pose (lane = row * kPsTile
//     + column).  The four waves, which split the points, are summed through LDS.
#pragma once
#include "../../include/pose_search/o3s_pose_search.h"
#include "cloud_dev.h"
#include "voxel_table.h"

namespace {
namespace o3s_cloud {

constexpr int kPsTile = 8;  // xy cells per tile side: kPsTile^2 = the 64 lanes that own the tile's poses
static_assert(kPsTile * kPsTile == 64, "one lane per pose of a tile");
constexpr int kPsMaxTopK = O3S_POSE_SEARCH_MAX_TOP_K;

struct PsGrid {  // the grid as the kernels read it
  double tc[3];
  double step_xy, step_z;
  int32_t nx, ny, nz;     // half widths
  int32_t cx, cy, cz, cl; // cells per axis: 2 n + 1, n_yaw
  int32_t tiles_x, tiles_y;
  int32_t ring;           // the yaw axis wraps for the local-maximum rule (yaw_ring and n_yaw >= 3)
};

// what the selection kernels hand from one to the next, and the result block that is copied to the host
struct PsSelect {
  unsigned long long t_start, t_end;  // wall_clock64 stamps: k_ps_score's block 0, k_ps_finish
  uint32_t tau;      // threshold score: every eligible pose above it is a winner
  uint32_t n_above;  // eligible poses with score > tau (< top_k)
  uint32_t take_tie; // of the eligible poses with score == tau the first take_tie in index order are winners
  uint32_t n_slot;   // slots handed out to the poses above tau (k_ps_ties)
  uint32_t n_found;
  uint32_t pad;
  unsigned long long cand[kPsMaxTopK];  // keys of the winners: slot order, then (k_ps_finish) best first
};
// a winner's key: larger = earlier in (score descending, index ascending); P <= 2^26 < 2^32
__device__ __forceinline__ unsigned long long ps_key(uint32_t score, int64_t p) {
  return ((unsigned long long)score << 32) | (unsigned long long)(0xffffffffu - (uint32_t)p);
}

// rot: n_yaw x 9 doubles, row-major R of each yaw (formed on the host).  pts: 3 x N; point m of the strided set is point m * stride.
__global__ void __launch_bounds__(kB) k_ps_score(const double* __restrict__ pts, int64_t M, int64_t stride, const double* __restrict__ rot, PsGrid g,
                                                 double inv, const unsigned long long* __restrict__ tab, uint32_t mask,
                                                 uint32_t* __restrict__ scores, PsSelect* __restrict__ sel) {
  __shared__ uint32_t s_part[kB / 64][64];
  if (blockIdx.x == 0 && threadIdx.x == 0) sel->t_start = wall_clock64();
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  // block -> (yaw l, z cell k, tile row ty, tile column tx); tx runs fastest
  uint32_t b = blockIdx.x;
  const int tx = (int)(b % (uint32_t)g.tiles_x);
  b /= (uint32_t)g.tiles_x;
  const int ty = (int)(b % (uint32_t)g.tiles_y);
  b /= (uint32_t)g.tiles_y;
  const int k = (int)(b % (uint32_t)g.cz);
  const int l = (int)(b / (uint32_t)g.cz);
  const int i0 = tx * kPsTile, j0 = ty * kPsTile;
  const int cols = min(kPsTile, g.cx - i0), rows = min(kPsTile, g.cy - j0);  // the tile's cells inside the grid (uniform)

  double R[9];
#pragma unroll
  for (int a = 0; a < 9; ++a) R[a] = rot[(size_t)l * 9 + a];
  double tcol[kPsTile];  // t.x of the tile's columns
#pragma unroll
  for (int u = 0; u < kPsTile; ++u) tcol[u] = g.tc[0] + (double)(i0 + u - g.nx) * g.step_xy;
  const double tz = g.tc[2] + (double)(k - g.nz) * g.step_z;

  uint32_t mine = 0;  // hits of the pose this lane owns, over this wave's points
  for (int64_t m0 = (int64_t)wave * 64; m0 < M; m0 += kB) {  // (uniform trip count per wave)
    const int64_t m = m0 + lane;
    const bool have = m < M;
    double x = 0.0, y = 0.0, z = 0.0;
    if (have) {
      const double* p = pts + 3 * (m * stride);
      x = p[0];
      y = p[1];
      z = p[2];
    }
    double s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double v = R[3 * a] * x;
      v = v + R[3 * a + 1] * y;
      v = v + R[3 * a + 2] * z;
      s[a] = v;
    }
    // the key, axis by axis: dm_pack's fields
    const double fz = floor((s[2] + tz) * inv);
    const bool okz = have && dm_in_range(fz);
    const unsigned long long kz = okz ? dm_field((int32_t)fz, 2) : 0ull;
    unsigned long long kx[kPsTile];
    uint32_t okx = 0;
#pragma unroll
    for (int u = 0; u < kPsTile; ++u) {
      const double fx = floor((s[0] + tcol[u]) * inv);
      const bool ok = okz && u < cols && dm_in_range(fx);
      kx[u] = ok ? dm_field((int32_t)fx, 0) : 0ull;
      okx |= ok ? 1u << u : 0u;
    }
    for (int r = 0; r < rows; ++r) {
      const double trow = g.tc[1] + (double)(j0 + r - g.ny) * g.step_xy;
      const double fy = floor((s[1] + trow) * inv);
      const bool oky = dm_in_range(fy);
      const unsigned long long kzy = kz | (oky ? dm_field((int32_t)fy, 1) : 0ull);
      const uint32_t valid = oky ? okx : 0u;
      unsigned long long k1[kPsTile], v[kPsTile];
      uint32_t h[kPsTile];
#pragma unroll
      for (int u = 0; u < kPsTile; ++u) {
        k1[u] = (kzy | kx[u]) + 1ull;
        h[u] = ov_hash(k1[u]) & mask;
      }
#pragma unroll
      for (int u = 0; u < kPsTile; ++u) v[u] = (valid >> u & 1u) ? tab[h[u]] : 0ull;  // the row's first probes: all in flight
      uint32_t hit = 0, open = 0;
#pragma unroll
      for (int u = 0; u < kPsTile; ++u) {
        const bool on = (valid >> u & 1u) != 0u;
        hit |= (on && v[u] == k1[u]) ? 1u << u : 0u;
        open |= (on && v[u] != k1[u] && v[u] != 0ull) ? 1u << u : 0u;
      }
      // later probes, round by round (the table is never full: an empty slot ends every miss; the bound is k_vm_count's)
      for (uint32_t probe = 1; open != 0u && probe <= mask; ++probe) {
#pragma unroll
        for (int u = 0; u < kPsTile; ++u) {
          h[u] = (h[u] + 1u) & mask;
          v[u] = (open >> u & 1u) ? tab[h[u]] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kPsTile; ++u) {
          const bool on = (open >> u & 1u) != 0u;
          const bool found = on && v[u] == k1[u];
          hit |= found ? 1u << u : 0u;
          if (on && (found || v[u] == 0ull)) open &= ~(1u << u);
        }
      }
#pragma unroll
      for (int u = 0; u < kPsTile; ++u) {
        const uint32_t c = (uint32_t)__popcll(__ballot((hit >> u & 1u) != 0u));
        mine += lane == r * kPsTile + u ? c : 0u;
      }
    }
  }
  s_part[wave][lane] = mine;
  __syncthreads();
  if (wave == 0) {
    const int r = lane / kPsTile, u = lane % kPsTile;
    if (r < rows && u < cols) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < kB / 64; ++w) total += s_part[w][lane];
      const int64_t p = (((int64_t)l * g.cz + k) * g.cy + (j0 + r)) * g.cx + (i0 + u);
      scores[p] = total;
    }
  }
}

// elig[p] = 1 when pose p may be selected: score >= min_score, and (local_maxima) no neighbour beats it.  The eligible poses are
// counted per score in hist (n_bins = the largest possible score + 1): the lanes of a wave that share the score of its first
// open lane add their number with one atomic (a constant field — no overlap anywhere — is one atomic per wave, not P on one word).
__global__ void __launch_bounds__(kB) k_ps_peaks(const uint32_t* __restrict__ scores, int64_t P, PsGrid g, int local_maxima, int64_t min_score,
                                                 uint32_t* __restrict__ elig, uint32_t* __restrict__ hist, uint32_t n_bins) {
  const int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  bool ok = false;
  uint32_t sc = 0;
  if (p < P) {
    sc = scores[p];
    ok = (int64_t)sc >= min_score && sc < n_bins;
    if (ok && local_maxima) {
      int64_t rest = p;
      const int i = (int)(rest % g.cx);
      rest /= g.cx;
      const int j = (int)(rest % g.cy);
      rest /= g.cy;
      const int k = (int)(rest % g.cz);
      const int l = (int)(rest / g.cz);
      for (int dl = -1; dl <= 1 && ok; ++dl) {
        int ql = l + dl;
        if (ql < 0 || ql >= g.cl) {
          if (!g.ring) continue;
          ql = ql < 0 ? ql + g.cl : ql - g.cl;
        }
        for (int dk = -1; dk <= 1 && ok; ++dk) {
          const int qk = k + dk;
          if (qk < 0 || qk >= g.cz) continue;
          for (int dj = -1; dj <= 1 && ok; ++dj) {
            const int qj = j + dj;
            if (qj < 0 || qj >= g.cy) continue;
            for (int di = -1; di <= 1; ++di) {
              const int qi = i + di;
              if (qi < 0 || qi >= g.cx) continue;
              const int64_t q = (((int64_t)ql * g.cz + qk) * g.cy + qj) * g.cx + qi;
              if (q == p) continue;  // (with 3 or more yaws on a ring no other offset comes back to p)
              const uint32_t sq = scores[q];
              if (sq > sc || (sq == sc && q < p)) ok = false;
            }
          }
        }
      }
    }
    elig[p] = ok ? 1u : 0u;
  }
  bool pending = ok;
  for (;;) {
    const unsigned long long open = __ballot(pending);
    if (!open) break;
    const int leader = __ffsll((long long)open) - 1;
    const uint32_t ls = (uint32_t)__shfl((int)sc, leader);
    const bool same = pending && sc == ls;
    const unsigned long long grp = __ballot(same);
    if (lane == leader) atomicAdd(&hist[ls], (uint32_t)__popcll(grp));
    pending = pending && !same;
  }
}

// One block: the threshold.  Walks the histogram from the top bin down to lo = max(min_score, 0): tau = the largest score with
// at least top_k eligible poses at or above it, or lo when there are fewer; n_above = those above tau, take_tie = how many of
// the poses AT tau are still wanted.  Also resets the slot counter of k_ps_ties.
__global__ void __launch_bounds__(kB) k_ps_threshold(const uint32_t* __restrict__ hist, uint32_t n_bins, int64_t min_score, uint32_t top_k,
                                                     PsSelect* __restrict__ sel) {
  __shared__ unsigned long long s_sum[kB];
  if (blockIdx.x != 0) return;
  const int64_t lo = min_score > 0 ? min_score : 0, hi = (int64_t)n_bins - 1;
  if (lo > hi) {  // nothing can reach min_score (uniform)
    if (threadIdx.x == 0) {
      sel->tau = 0xffffffffu;
      sel->n_above = sel->take_tie = sel->n_slot = 0u;
    }
    return;
  }
  // thread t takes the t-th chunk of the bins in DESCENDING order: bins hi - t * per ... down
  const int64_t n = hi - lo + 1, per = (n + kB - 1) / kB;
  const int64_t first = hi - (int64_t)threadIdx.x * per;  // this thread's highest bin
  const int64_t last = first - per + 1 > lo ? first - per + 1 : lo;
  unsigned long long mine = 0;
  for (int64_t bin = first; bin >= last; --bin) mine += hist[bin];
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  unsigned long long before = 0;  // eligible poses in the bins above this thread's
  for (int t = 0; t < (int)threadIdx.x; ++t) before += s_sum[t];
  unsigned long long total = 0;
  for (int t = 0; t < kB; ++t) total += s_sum[t];
  if (total < top_k) {  // fewer eligible poses than wanted: all of them
    if (threadIdx.x == 0) {
      sel->tau = (uint32_t)lo;
      sel->n_above = (uint32_t)(total - hist[lo]);
      sel->take_tie = hist[lo];
      sel->n_slot = 0u;
    }
    return;
  }
  if (before < top_k && before + mine >= top_k) {  // the crossing lies in this thread's chunk: exactly one thread
    unsigned long long above = before;
    for (int64_t bin = first; bin >= last; --bin) {
      const uint32_t c = hist[bin];
      if (above + c >= top_k) {
        sel->tau = (uint32_t)bin;
        sel->n_above = (uint32_t)above;
        sel->take_tie = (uint32_t)(top_k - above);
        sel->n_slot = 0u;
        break;
      }
      above += c;
    }
  }
}

// The eligible poses above tau (fewer than top_k) take a slot each; flag[p] (in place of elig) = the pose is eligible AT tau.
// The slot order is whatever the atomics make it: k_ps_finish orders the winners by their keys, which are all different.
__global__ void __launch_bounds__(kB) k_ps_ties(const uint32_t* __restrict__ scores, int64_t P, uint32_t* __restrict__ flag, PsSelect* __restrict__ sel) {
  const int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (p >= P) return;
  const uint32_t tau = sel->tau;
  const uint32_t sc = scores[p];
  const bool el = flag[p] != 0u;
  if (el && sc > tau) {
    const uint32_t slot = atomicAdd(&sel->n_slot, 1u);
    if (slot < (uint32_t)kPsMaxTopK) sel->cand[slot] = ps_key(sc, p);
  }
  flag[p] = (el && sc == tau) ? 1u : 0u;
}
// off: the exclusive scan of flag — a tie's rank in index order
__global__ void __launch_bounds__(kB) k_ps_take_ties(const uint32_t* __restrict__ scores, int64_t P, const uint32_t* __restrict__ flag,
                                                     const uint32_t* __restrict__ off, PsSelect* __restrict__ sel) {
  const int64_t p = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (p >= P || !flag[p]) return;
  const uint32_t rank = off[p], at = sel->n_above + rank;
  if (rank < sel->take_tie && at < (uint32_t)kPsMaxTopK) sel->cand[at] = ps_key(scores[p], p);
}
// One wave: the winners in order (each lane ranks its key among the others: the keys are all different), and the end stamp.
__global__ void __launch_bounds__(64) k_ps_finish(PsSelect* __restrict__ sel) {
  if (blockIdx.x != 0) return;
  __shared__ unsigned long long s_key[kPsMaxTopK];
  const int lane = (int)threadIdx.x;
  uint32_t n = sel->n_above + sel->take_tie;
  n = n > (uint32_t)kPsMaxTopK ? (uint32_t)kPsMaxTopK : n;
  const unsigned long long key = lane < (int)n ? sel->cand[lane] : 0ull;
  s_key[lane] = key;
  __syncthreads();
  uint32_t rank = 0;
  for (uint32_t q = 0; q < n; ++q) rank += s_key[q] > key ? 1u : 0u;
  __syncthreads();
  if (lane < (int)n) sel->cand[rank] = key;
  if (lane == 0) {
    sel->n_found = n;
    sel->t_end = wall_clock64();
  }
}

}  // namespace o3s_cloud
}  // namespace
