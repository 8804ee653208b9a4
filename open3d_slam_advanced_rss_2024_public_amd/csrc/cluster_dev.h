// cluster_dev.h — Open3D's PointCloud::ClusterDBSCAN(eps, min_points) on device arrays (part of the cloud_ops.hip translation unit;
// Open3D v0.15.1, geometry/PointCloudCluster.cpp; Ester et al. 1996).  The contract is restated in closed form in
// include/clustering/o3s_clustering.h: core points by an exact count, clusters = the connected components of the eps-graph on the
// core points, numbered by their smallest core index, border points to the smallest id among their core neighbours.  The
// neighbour search is the radius filter's (outlier_dev.h: grid over the finite points with cell >= eps, the 3 x 3 x 3 block as
// nine runs).  fp64 distances without FMA contraction, integer atomics only: every result is an integer that no launch order,
// cell size or arrival order of an atomic can move.
//
// The components: a union-find over parent[] (indexed by input index, identity at the start), built by k_db_link.
//   Invariant   parent[x] <= x, always.  The only write to parent[] inside k_db_link is an agent-scope CAS(&parent[r], r, lo)
//               with lo < r: it succeeds only on a root, so every word is written at most once, from r to something smaller.  The
//               links form a forest whose roots are the smallest members of their trees, and a tree never splits.
//   Stale reads A load inside the launch may miss another workgroup's store (other XCD, other L2).  Since a word changes once, a
//               load of parent[x] gives either x (possibly stale) or the final parent of x: both are ancestors-or-self of x in the
//               true forest.  A find by plain loads therefore ends at SOME ancestor of its start, not always the root.
//   Union       find both ends to (a, b); a == b: the two starts share an ancestor, so they are in one tree already, and trees never
//               split — skipping is right whatever was stale.  Else hi = max, lo = min and old = CAS(&parent[hi], hi, lo).
//               old == hi: linked (hi was a root; lo need not be one: hanging a root under any member of the other tree joins the
//               two trees and keeps parent[x] <= x).  old != hi: hi was no root; old is its true parent, old < hi, and the union
//               continues from (old, lo).
//   Bounded     No lane waits for another.  Every step of a find and every failed CAS replaces an index by a strictly smaller
//               one; the pair (a, b) of a union decreases in the sum a + b with every retry, so a union ends after at most
//               2 N steps, in practice after the heights of the two trees.
//   Published   by the kernel boundary: k_db_flatten, a launch of its own, reads the final forest.
#pragma once
#include "outlier_dev.h"

namespace {
namespace o3s_cloud {

constexpr uint32_t kDbCore = 0x80000000u;  // bit 31 of sid[]: the point is core (input indices are below 2^31)
constexpr uint32_t kDbIdx = 0x7fffffffu;

// Pass 1: count to min_points (self included) with the radius filter's early stop.  sid[t], in cell-sorted order beside sp: the
// input index of sorted point t, with kDbCore set for a core point — what the later passes stream instead of gathering flags by
// input index.  parent[input index] = input index.
__global__ void __launch_bounds__(kB) k_db_core(const double* __restrict__ sp, const uint32_t* __restrict__ vals, int64_t N, NGrid g,
                                                const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, int min_points, double r2,
                                                const uint32_t* __restrict__ fmap /*nullable: identity*/, uint32_t* __restrict__ sid,
                                                uint32_t* __restrict__ parent) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  uint32_t lo[9], hi[9];
  block_runs(qx, qy, qz, g, cbeg, cend, lo, hi);
  int count = 0;
  walk_block(sp, lo, hi, qx, qy, qz, r2, [&](uint32_t, uint32_t m) { count += __popc(m); }, [&]() { return count >= min_points; });
  const uint32_t f = vals[t];
  const uint32_t i = fmap ? fmap[f] : f;
  sid[t] = i | (count >= min_points ? kDbCore : 0u);
  parent[i] = i;
}

// an ancestor-or-self of x (the root, when no load was stale): see the head of the file
__device__ __forceinline__ uint32_t db_find(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = parent[x];
    if (p >= x) return x;  // p == x; ">=" only so that no value could ever make the walk climb
    x = p;
  }
}

// joins the trees of a and b; returns a member of the joined tree to start the next find from (see the head of the file)
__device__ __forceinline__ uint32_t db_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = db_find(parent, a);
    b = db_find(parent, b);
    if (a == b) return a;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = atomicCAS(&parent[hi], hi, lo);  // agent scope; the returned value is what the word really held
    if (old == hi) return lo;
    a = old;  // hi had a parent already: old < hi, an ancestor in hi's tree
    b = lo;
  }
}

// Pass 2: one core query per lane (cell-sorted order).  Every core candidate of the block at d2 < r2 with a smaller input index is
// united with the query — every edge of the core graph is seen from its larger end.  The distance comes first, the finds run only
// for candidates that pass; `mine` carries a member of the query's tree from one union to the next, so later finds start low —
// mostly at the root, which is also what most neighbours' parent[] already says: those candidates cost no dependent load at all.
__global__ void __launch_bounds__(kB) k_db_link(const double* __restrict__ sp, const uint32_t* __restrict__ sid, int64_t N, NGrid g,
                                                const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, double r2, uint32_t* parent) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const uint32_t s = sid[t];
  if (!(s & kDbCore)) return;
  const uint32_t i = s & kDbIdx;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  uint32_t lo[9], hi[9];
  block_runs(qx, qy, qz, g, cbeg, cend, lo, hi);
  uint32_t mine = i;
  walk_block(
      sp, lo, hi, qx, qy, qz, r2,
      [&](uint32_t j0, uint32_t m) {
        // the batch's flags, then the first step of every find, as independent loads; only then the dependent walks
        uint32_t c[kWalkBatch], p[kWalkBatch];
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) c[u] = (m >> u) & 1u ? sid[j0 + (uint32_t)u] : 0u;
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) {
          const bool want = (c[u] & kDbCore) && (c[u] & kDbIdx) < i;
          p[u] = want ? parent[c[u] & kDbIdx] : 0xffffffffu;  // the candidate's parent or itself: a member of its tree
        }
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u)
          if (p[u] != 0xffffffffu && p[u] != mine) mine = db_unite(parent, mine, p[u]);  // p == mine: one tree already
      },
      [&]() { return false; });
}

// Pass 3a (a launch of its own: the boundary publishes parent[]): every core point's root, in cell-sorted order beside sid, and
// is_root[input index] = 1 for the roots (the array is zeroed beforehand).  The root of a tree is its smallest member, so the
// exclusive scan of is_root ranks the clusters by their smallest core index: rid[root] is the cluster's id.
__global__ void __launch_bounds__(kB) k_db_flatten(const uint32_t* __restrict__ sid, int64_t N, const uint32_t* __restrict__ parent, uint32_t* __restrict__ root_s,
                                                   uint32_t* __restrict__ is_root) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const uint32_t s = sid[t];
  uint32_t r = 0xffffffffu;
  if (s & kDbCore) {
    r = db_find(parent, s & kDbIdx);
    if (r == (s & kDbIdx)) is_root[r] = 1u;
  }
  root_s[t] = r;
}

// Pass 3b: the labels.  A core point takes the id of its root; a finite non-core point walks the block once more for the smallest
// root among its core neighbours — the smallest root is the smallest id — else -1 (labels[] starts at -1: non-finite points keep
// it).  size[label] += 1 by integer atomics, one per distinct label of a wave (neighbouring lanes mostly share theirs).
__global__ void __launch_bounds__(kB) k_db_label(const double* __restrict__ sp, const uint32_t* __restrict__ sid, const uint32_t* __restrict__ root_s, int64_t N,
                                                 NGrid g, const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, double r2,
                                                 const uint32_t* __restrict__ rid, int32_t* __restrict__ labels, uint32_t* __restrict__ size) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  int32_t lab = -1;
  if (t < N) {
    const uint32_t s = sid[t];
    uint32_t m = root_s[t];
    if (!(s & kDbCore)) {
      const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
      uint32_t lo[9], hi[9];
      block_runs(qx, qy, qz, g, cbeg, cend, lo, hi);
      walk_block(
          sp, lo, hi, qx, qy, qz, r2,
          [&](uint32_t j0, uint32_t hit) {
            uint32_t r[kWalkBatch];
#pragma unroll
            for (int u = 0; u < kWalkBatch; ++u) r[u] = (hit >> u) & 1u ? root_s[j0 + (uint32_t)u] : 0xffffffffu;  // non-core: 0xffffffff as well
#pragma unroll
            for (int u = 0; u < kWalkBatch; ++u) m = min(m, r[u]);
          },
          [&]() { return false; });
    }
    if (m != 0xffffffffu) lab = (int32_t)rid[m];
    labels[s & kDbIdx] = lab;
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(lab >= 0);
  while (todo) {  // wave-uniform: at most one turn per distinct label
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t l0 = __shfl(lab, leader);
    const unsigned long long same = __ballot(lab == l0);
    if (lane == leader) atomicAdd(&size[l0], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// keep = label >= 0 && size[label] >= min_cluster_size, in input order, with the per-block counts for the one-launch scan
__global__ void __launch_bounds__(kB) k_db_keep(const int32_t* __restrict__ labels, const uint32_t* __restrict__ size, int64_t N, uint32_t min_size,
                                                uint32_t* __restrict__ keep, uint32_t* __restrict__ blk_cnt) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  uint32_t f = 0u;
  if (i < N) {
    const int32_t l = labels[i];
    f = (l >= 0 && size[l] >= min_size) ? 1u : 0u;
    keep[i] = f;
  }
  put_block_count(f, blk_cnt);
}

// work area of one clustering call over n points (the grid index has its own: NormalsWork)
struct ClusterArea {
  static constexpr size_t kSlack = 4096;
  uint32_t *fin, *off, *fmap, *sid, *parent, *root_s, *is_root, *rid, *size, *keep, *koff;
  int32_t* labels;
  double* fpts;
  char* tmp;
  template <class A>
  void lay(A& a, size_t n, size_t tb_scan) {
    take(a, fin, n);
    take(a, off, n + 1);
    take(a, fmap, n);
    take(a, fpts, n * 3);
    take(a, sid, n);
    take(a, parent, n);
    take(a, root_s, n);
    take(a, is_root, n);
    take(a, rid, n + 1);
    take(a, size, n);
    take(a, labels, n);
    take(a, keep, n);
    take(a, koff, n + 1);
    take(a, tmp, tb_scan);
  }
};

struct ClusterWork {  // grow-only, leased per call from the device's pool
  NormalsWork grid;
  Arena arena;
  DevMem out_p, out_n, out_i;  // where the host-array entry compacts to before it copies out
};

struct ClusterResult {
  const int32_t* labels;       // N labels (device)
  const uint32_t* size;        // n_clusters sizes (device)
  const uint32_t *keep, *off;  // with_keep: keep flags and their exclusive scan (off[N] = n_keep)
  int64_t n_clusters, n_keep;
};

// DBSCAN(eps, min_points) on d_pts (3 x N doubles on the device, N > 0, parameters checked by the caller); with_keep also the keep
// flags of min_cluster_size and their scan.  Returns with everything in the work area and the two counts on the host.
inline int dbscan_dev(ClusterWork& w, double eps, int min_points, int min_cluster_size, bool with_keep, const double* d_pts, int64_t N, ClusterResult* out,
                      hipStream_t s) {
  if (N <= 0 || N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  const size_t tb = scan_temp_bytes(N);
  ClusterArea a;
  CK(lay_out(w.arena, a, (size_t)N, tb));
  uint32_t* blk = reinterpret_cast<uint32_t*>(a.tmp);
  out->labels = a.labels;
  out->size = a.size;
  out->keep = a.keep;
  out->off = a.koff;
  out->n_clusters = 0;
  out->n_keep = 0;
  // the finite points: the grid is built over them alone
  hipLaunchKernelGGL(k_or_finite, dim3(nblk(N)), dim3(kB), 0, s, d_pts, N, a.fin, blk, (double*)nullptr);
  int64_t Nf = 0;
  int rc = scan_flags(a.fin, a.off, N, a.tmp, tb, &Nf, s, blk);
  if (rc != O3S_OK) return rc;
  const double* fp = d_pts;
  const uint32_t* fmap = nullptr;
  if (Nf < N && Nf > 0) {
    hipLaunchKernelGGL(k_compact, dim3(nblk(N)), dim3(kB), 0, s, d_pts, (const double*)nullptr, N, a.fin, a.off, a.fpts, (double*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_or_fmap, dim3(nblk(N)), dim3(kB), 0, s, a.fin, a.off, N, a.fmap);
    fp = a.fpts;
    fmap = a.fmap;
  }
  CK(hipMemsetAsync(a.labels, 0xff, (size_t)N * 4, s));  // -1
  if (Nf > 0) {
    // cell = eps, a hair above (see outlier_flags_dev): every neighbour lies in the 3 x 3 x 3 block, also when the build made the cell coarser
    GridIndex gi;
    rc = build_grid_index(w.grid, fp, Nf, eps * (1.0 + 1e-6), 0.0, 0.0, &gi, s, nullptr, /*keep_cell=*/true, outlier_max_cells());
    if (rc != O3S_OK) return rc;
    const double r2 = eps * eps;
    const dim3 gr(nblk(Nf)), bl(kB);
    CK(hipMemsetAsync(a.is_root, 0, (size_t)N * 4, s));
    hipLaunchKernelGGL(k_db_core, gr, bl, 0, s, gi.sp, gi.vals, Nf, gi.g, gi.cbeg, gi.cend, min_points, r2, fmap, a.sid, a.parent);
    hipLaunchKernelGGL(k_db_link, gr, bl, 0, s, gi.sp, (const uint32_t*)a.sid, Nf, gi.g, gi.cbeg, gi.cend, r2, a.parent);
    hipLaunchKernelGGL(k_db_flatten, gr, bl, 0, s, (const uint32_t*)a.sid, Nf, (const uint32_t*)a.parent, a.root_s, a.is_root);
    CK(hipGetLastError());
    rc = scan_flags(a.is_root, a.rid, N, a.tmp, tb, &out->n_clusters, s);
    if (rc != O3S_OK) return rc;
    if (out->n_clusters > 0) {
      CK(hipMemsetAsync(a.size, 0, (size_t)out->n_clusters * 4, s));
      hipLaunchKernelGGL(k_db_label, gr, bl, 0, s, gi.sp, (const uint32_t*)a.sid, (const uint32_t*)a.root_s, Nf, gi.g, gi.cbeg, gi.cend, r2, (const uint32_t*)a.rid, a.labels,
                         a.size);
      CK(hipGetLastError());
    }
  }
  if (with_keep) {
    hipLaunchKernelGGL(k_db_keep, dim3(nblk(N)), dim3(kB), 0, s, (const int32_t*)a.labels, (const uint32_t*)a.size, N, (uint32_t)min_cluster_size, a.keep, blk);
    CK(hipGetLastError());
    rc = scan_flags(a.keep, a.koff, N, a.tmp, tb, &out->n_keep, s, blk);
    if (rc != O3S_OK) return rc;
  }
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace
