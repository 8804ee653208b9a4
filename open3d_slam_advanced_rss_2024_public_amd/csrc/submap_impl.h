// submap_impl.h — device-resident active submap (C ABI: include/o3s_submap.h), gfx950 only.  Included at the end of
// cloud_ops.hip so that both share one instantiation of the kernels and of the rocPRIM sort / scan in cloud_dev.h.
#pragma once
#include "../../include/o3s_scan.h"
#include "../../include/o3s_submap.h"

#include "cloud_dev.h"
#include "normals_dev.h"
#include "fpfh_dev.h"

namespace {

// o3d_slam::transform (helpers.cpp:283-318): p' = (T [p 1]).head<3>() / w, n' = (T [n 0]).head<3>() (o3d_transform_point /
// o3d_transform_dir, cloud_dev.h)
__device__ __forceinline__ void transform_append_one(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t i, const double* T,
                                                     double* __restrict__ out_pts, double* __restrict__ out_n) {
  double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
  o3d_transform_point(T, x, y, z);
  out_pts[3 * i] = x;
  out_pts[3 * i + 1] = y;
  out_pts[3 * i + 2] = z;
  if (nrm) {
    double w[3];
    o3d_transform_dir(T, nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], w);
    out_n[3 * i] = w[0];
    out_n[3 * i + 1] = w[1];
    out_n[3 * i + 2] = w[2];
  }
}
__global__ void __launch_bounds__(kB) k_transform_append_v(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t N, Pose4d Tm,
                                                           double* __restrict__ out_pts, double* __restrict__ out_n) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  transform_append_one(pts, nrm, i, Tm.m, out_pts, out_n);
}
__global__ void __launch_bounds__(kB) k_transform_append(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t N,
                                                         const double* __restrict__ Tm /*16, column-major*/, double* __restrict__ out_pts,
                                                         double* __restrict__ out_n) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  double T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = Tm[k];
  transform_append_one(pts, nrm, i, T, out_pts, out_n);
}

// Open3D PointCloud::Transform on a resident submap, in place (o3s_submap_transform): lanes [0, n_map) take the map cloud, lanes
// [n_map, n_map + n_feat) the feature cloud.  The arithmetic is transform_append_one's; there is no almost-identity branch here
// (that one belongs to o3d_slam::transform).  A lane reads its own 24 + 24 bytes before it writes them and touches nobody else's,
// which is what makes the in-place form safe (undistort_dev.h).  No LDS, no atomics, no scratch
// (profiles/pose_graph/resource_usage.txt).
__global__ void __launch_bounds__(kB) k_submap_transform(double* map_p, double* map_n /*nullable*/, int64_t n_map, double* feat_p, double* feat_n,
                                                         int64_t n_feat, Pose4d Tm) {
  int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= n_map + n_feat) return;
  double* p = map_p;
  double* q = map_n;
  if (i >= n_map) {
    i -= n_map;
    p = feat_p;
    q = feat_n;
  }
  double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
  o3d_transform_point(Tm.m, x, y, z);
  p[3 * i] = x;
  p[3 * i + 1] = y;
  p[3 * i + 2] = z;
  if (q) {
    double w[3];
    o3d_transform_dir(Tm.m, q[3 * i], q[3 * i + 1], q[3 * i + 2], w);
    q[3 * i] = w[0];
    q[3 * i + 1] = w[1];
    q[3 * i + 2] = w[2];
  }
}

// o3d_slam::transform (helpers.cpp:283-318) on host buffers: points (/ w), normals, covariances R C R^T; an (almost-)identity
// T returns the cloud TWICE (the copy of :285-288 followed by the loop's appends), which is what the reference does.
__global__ void __launch_bounds__(kB) k_transform_cov(const double* __restrict__ cov, int64_t N, const double* __restrict__ Tm, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  double R[3][3], C[3][3], RC[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      R[r][c] = Tm[c * 4 + r];
      C[r][c] = cov[9 * i + c * 3 + r];  // Eigen::Matrix3d is column-major
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double s = R[r][0] * C[0][c];
      s = s + R[r][1] * C[1][c];
      s = s + R[r][2] * C[2][c];
      RC[r][c] = s;
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double s = RC[r][0] * R[c][0];
      s = s + RC[r][1] * R[c][1];
      s = s + RC[r][2] * R[c][2];
      out[9 * i + c * 3 + r] = s;
    }
}

// getVoxelIdx(p, 1 / voxel) (VoxelHashMap.hpp:48-51) of the carving VoxelMap, made total: the reference's int cast is undefined for a
// floor that is NaN, infinite or beyond int32 (x86 gives INT_MIN, which names no voxel of any map; the conversion here gives 0 for
// NaN and saturates otherwise — 0 is the voxel at the map's origin).  Such a coordinate names no voxel: a map point that has one is
// in no voxel and is never carved, a stop of a ray that has one finds nothing.  Finite in-range input takes the cast it always took.
__device__ __forceinline__ bool carve_idx_ok(double f) { return f >= -2147483648.0 && f <= 2147483647.0; }  // false for NaN
__device__ __forceinline__ bool carve_voxel_of(double x, double y, double z, double inv, int32_t v[3]) {
  const double fx = floor(x * inv), fy = floor(y * inv), fz = floor(z * inv);
  if (!(carve_idx_ok(fx) && carve_idx_ok(fy) && carve_idx_ok(fz))) return false;
  v[0] = (int32_t)fx;
  v[1] = (int32_t)fy;
  v[2] = (int32_t)fz;
  return true;
}
// voxel key of the carving VoxelMap, packed relative to the subset's index box; points outside the subset (and points of it that
// are in no voxel) get `out_key` — the next power of two above every packed key — and sort last
__global__ void __launch_bounds__(kB) k_carve_keys(const double* __restrict__ pts, int64_t N, const uint32_t* __restrict__ inflag, double inv,
                                                   int32_t x0, int32_t y0, int32_t z0, uint64_t ex, uint64_t ey, uint64_t out_key,
                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  vals[i] = (uint32_t)i;
  int32_t v[3];
  if (!inflag[i] || !carve_voxel_of(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], inv, v)) {
    keys[i] = out_key;
    return;
  }
  const int64_t x = (int64_t)v[0] - x0, y = (int64_t)v[1] - y0, z = (int64_t)v[2] - z0;
  keys[i] = ((uint64_t)z * ey + (uint64_t)y) * ex + (uint64_t)x;
}
__global__ void __launch_bounds__(kB) k_carve_box(const double* __restrict__ pts, int64_t N, const uint32_t* __restrict__ inflag, double inv,
                                                  int32_t* __restrict__ mm_slots /*[kExtSlots][min[3], max[3]]*/) {
  int32_t* mm = mm_slots + 6 * (blockIdx.x & (kExtSlots - 1));
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  int32_t vx[3] = {0, 0, 0};
  const bool live = i < N && inflag[i] && carve_voxel_of(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], inv, vx);
  for (int a = 0; a < 3; ++a) {
    const int32_t v = vx[a];
    const int32_t lo = wave_min_i32(live ? v : INT32_MAX), hi = wave_max_i32(live ? v : INT32_MIN);
    if ((threadIdx.x & 63) == 0 && lo <= hi) {  // a (possibly stale) look first: extrema are monotone, so skipping is safe
      if (lo < __atomic_load_n(&mm[a], __ATOMIC_RELAXED)) atomicMin(&mm[a], lo);
      if (hi > __atomic_load_n(&mm[3 + a], __ATOMIC_RELAXED)) atomicMax(&mm[3 + a], hi);
    }
  }
}
// getIdxsOfCarvedPoints (helpers.cpp:252-281): one lane per ray, the same sequential march as the reference
__global__ void __launch_bounds__(kB) k_carve_rays(const double* __restrict__ scan /*map frame*/, int64_t Ns, double sx, double sy, double sz,
                                                   double voxel, double inv, double max_len, double trunc, double min_dot,
                                                   const uint64_t* __restrict__ keys /*sorted*/, const uint32_t* __restrict__ vals, int64_t n_in,
                                                   int32_t x0, int32_t y0, int32_t z0, int64_t ex, int64_t ey, int64_t ez,
                                                   const double* __restrict__ map_n /*nullable*/, uint32_t* __restrict__ remove) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= Ns) return;
  const double dx = scan[3 * i] - sx, dy = scan[3 * i + 1] - sy, dz = scan[3 * i + 2] - sz;
  const double length = sqrt((dx * dx + dy * dy) + dz * dz);
  if (!(length > 0.0)) return;  // a return at the sensor origin: the reference's NaN positions never find a voxel
  const double ux = dx / length, uy = dy / length, uz = dz / length;
  double distance = 0.0;
  const double max_path = fmax(voxel, fmin(length - trunc, max_len));
  while (distance < max_path) {  // NaN lengths (a return at the sensor origin) make this false, like the reference
    const double cx = distance * ux + sx, cy = distance * uy + sy, cz = distance * uz + sz;
    int32_t v[3] = {0, 0, 0};
    const bool named = carve_voxel_of(cx, cy, cz, inv, v);  // false: an overflowed return has length inf and a NaN direction
    const int64_t x = (int64_t)v[0] - x0, y = (int64_t)v[1] - y0, z = (int64_t)v[2] - z0;
    if (named && x >= 0 && x < ex && y >= 0 && y < ey && z >= 0 && z < ez) {
      const uint64_t key = ((uint64_t)z * (uint64_t)ey + (uint64_t)y) * (uint64_t)ex + (uint64_t)x;
      int64_t lo = 0, hi = n_in;  // lower_bound in the sorted subset keys
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
      }
      for (int64_t j = lo; j < n_in && keys[j] == key; ++j) {
        const uint32_t id = vals[j];
        bool rm = true;
        if (map_n) {
          double nx = map_n[3 * (size_t)id], ny = map_n[3 * (size_t)id + 1], nz = map_n[3 * (size_t)id + 2];
          const double zz = (nx * nx + ny * ny) + nz * nz;  // Eigen normalized()
          if (zz > 0) {
            const double s = sqrt(zz);
            nx /= s;
            ny /= s;
            nz /= s;
          }
          rm = fabs((ux * nx + uy * ny) + uz * nz) > min_dot;
        }
        if (rm) remove[id] = 1u;
      }
    }
    distance += voxel;
  }
}
// Submap::computeSubmapCenter = open3d PointCloud::GetCenter(): the mean of the map points.  Per-block fp64 partial sums in a
// fixed order (thread-strided, wave reduction, then the four waves), folded by block 0's caller on the host in block order.
__global__ void __launch_bounds__(kB) k_center_part(const double* __restrict__ pts, int64_t N, double* __restrict__ part /*[grid][3]*/) {
  double s[3] = {0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < N; i += (int64_t)gridDim.x * kB)
    for (int a = 0; a < 3; ++a) s[a] += pts[3 * i + a];
  __shared__ double sh[kB / 64][3];
  for (int a = 0; a < 3; ++a) {
    double v = s[a];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_down(v, m, 64);  // its own tree (halves first): not wave_sum's, so it stays
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = sh[0][threadIdx.x];
    for (int w = 1; w < kB / 64; ++w) v += sh[w][threadIdx.x];
    part[(size_t)blockIdx.x * 3 + threadIdx.x] = v;
  }
}
__global__ void __launch_bounds__(kB) k_invert_flags(const uint32_t* __restrict__ remove, int64_t N, uint32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i < N) keep[i] = remove[i] ? 0u : 1u;
}

}  // namespace

// csrc/o3s_icp.hip (same library, not part of the C ABI): index build over a reference whose point count is a word on the device
extern "C" int o3s_icp_init_reference_dev_counted_async(o3s_icp* h, const void* d_xyzw, const void* d_normals, const uint32_t* d_count, int64_t max_M,
                                                        int64_t* M_out);

struct o3s_submap {
  int device = 0;
  double voxel = 0.0;
  o3s_cropper cropper{};
  hipStream_t stream = nullptr;
  bool owns_stream = true;        // false: `stream` is one of the device's shared submap streams (submap_streams)
  hipEvent_t handover = nullptr;  // recorded on `stream`, waited for by the ICP handle's stream (o3s_icp_wait_event)
  DevMem pts[2], nrm[2];  // ping-pong: voxelisation reads [cur] and writes [1 - cur]
  int cur = 0;
  int64_t n = 0;
  // layout of the map array after a voxelisation: [n_pt pass-through points | one point per voxel in key order]; valid only while
  // nothing else has rewritten the array (voxel_insert_merge_dev relies on it, and checks it on the device)
  int64_t n_pt = 0;
  bool layout_valid = false;
  int merge_backoff = 0;              // inserts left before the merge path is tried again after it had to give way to the sort
  int64_t n_merged = 0, n_sorted = 0, n_fell_back = 0;  // how the voxelising inserts ran (o3s_submap_insert_stats)
  int has_normals = -1;  // -1: undecided (empty map)
  DevMem col[2];           // colours of the map cloud (open3d PointCloud::colors_), ping-pong like the points
  int has_colors = 0;    // 1 while the map carries one colour per point (PointCloud::HasColors())
  DevMem scan_c;
  DevMem scan_p, scan_n, carve_scan, d_T, patch_xyzw, patch_n32;
  Arena arena;
  // An insert whose completion is looked at later (o3s_submap_insert_processed): everything is enqueued, the merge path's counts and
  // verdict are on their way to a mailbox slot, and `n`, `cur`, `n_pt` still describe the map BEFORE the insert.  submap_settle() —
  // the first thing every entry point does — fetches them (waiting only if the GPU has not got there yet), runs the sort-based
  // pipeline if the merge had to give way, and commits the new state.
  struct PendingInsert {
    bool active = false;
    LazyPost post;
    int c = 0;
    int64_t n_tmp = 0;
    bool hn = false;
    VoxHint vh{};
  } pend;
  DevMem d_post;                      // 4 words the pending insert's counts also go to (lazy_post_fetch's fallback)
  hipEvent_t scan_read = nullptr;   // recorded when an insert has read its device scan: the scan's stream waits for it before the object is rewritten
  // the feature set of o3s_submap_compute_features: sparse cloud, its normals, FPFH (33 x n_feat); -1: none.  It describes the map
  // as it was when it was computed; inserts leave it alone
  DevMem feat_p, feat_n, feat_f;
  int64_t n_feat = -1;
  FpfhWork feat_w;  // grid, neighbour lists and SPFH of the last computation (given back by o3s_submap_trim)
  // the occupancy snapshot of o3s_submap_build_voxel_map (Submap::voxelMap_): an open-addressing table of packed voxel keys + 1
  // (0: empty), vox_slots of them (a power of two); n_vox = distinct voxels, -1: never built.  Like the feature set it describes the
  // map as it was when it was built: inserts, carving and o3s_submap_transform leave it alone (overlap_impl.h)
  DevMem vox_tab;
  int64_t n_vox = -1;
  uint32_t vox_slots = 0;
  double vox_size = 0.0;
};

namespace {
int set_dev(const o3s_submap* m) { return hipSetDevice(m->device) == hipSuccess ? O3S_OK : O3S_ERR_HIP; }
int submap_settle(o3s_submap* m);  // completes a pending insert (defined with insert_dev below)
inline int submap_settle(const o3s_submap* m) { return submap_settle(const_cast<o3s_submap*>(m)); }

// Creating a HIP stream makes a hardware queue: 2.6 - 3.5 ms on the calling thread — the mapping thread, every time
// SubmapCollection::createNewSubmap runs (it was the largest part of a switch of submaps once the buffers changed hands instead of
// being freed and made again).  The submaps of a device therefore share a few streams, made on first use and kept for the life of
// the process, dealt round-robin: two submaps on one stream only ever order their work behind each other (the mapper works on one
// submap at a time), which no call's semantics depends on.  Snapshots made for a worker thread (o3s_submap_clone) get a stream of
// their own: they are there to run beside the mapper.
inline DeviceStreams<4>& submap_streams() {
  static DeviceStreams<4>* p = new DeviceStreams<4>;  // never destroyed (see DeviceStreams)
  return *p;
}
// all of a device's streams are made with its first submap (a collection's constructor), not one per switch of submaps later;
// a device that could not make all four deals what it got, and has no stream only if it got none
inline hipStream_t next_submap_stream(int device) {  // the device is current
  static std::mutex m;
  static std::vector<unsigned> next;  // [device]: the round-robin turn
  const auto set = submap_streams().get(device);
  std::lock_guard<std::mutex> g(m);
  if ((size_t)device >= next.size()) next.resize((size_t)device + 1, 0u);
  const unsigned k = next[(size_t)device]++ % 4u;
  return set.n ? set.s[k % (unsigned)set.n] : nullptr;
}

// work area of space carving on a map of nm points
struct CarveArea {
  static constexpr size_t kSlack = 8192;  // twice the usual page: what carving has always reserved
  uint32_t *inflag, *remove, *keep, *off;
  uint64_t *keys, *keys2;
  uint32_t *vals, *vals2;
  int32_t* d_mm;
  char* tmp;
  template <class A>
  void lay(A& a, size_t nm, size_t tb_scan, size_t tb_sort) {
    take(a, inflag, nm);
    take(a, remove, nm);
    take(a, keep, nm);
    take(a, off, nm + 1);
    take(a, keys, nm);
    take(a, keys2, nm);
    take(a, vals, nm);
    take(a, vals2, nm);
    take(a, d_mm, kExtSlots * 6);
    take(a, tmp, std::max(tb_scan, tb_sort));
  }
};
}  // namespace

extern "C" {

static int submap_create_impl(int device, double map_voxel_size, const o3s_cropper* map_builder_cropper, bool own_stream, o3s_submap** out) {
  if (!out || !map_builder_cropper) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  o3s_submap* m = new o3s_submap();
  m->device = device;
  m->voxel = map_voxel_size;
  m->cropper = *map_builder_cropper;
  m->owns_stream = own_stream;
  if (own_stream) {
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) m->stream = nullptr;
  } else {
    m->stream = next_submap_stream(device);
  }
  if (!m->stream || hipEventCreateWithFlags(&m->handover, hipEventDisableTiming) != hipSuccess) {
    if (m->stream && m->owns_stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return O3S_ERR_HIP;
  }
  *out = m;
  return O3S_OK;
}

int o3s_submap_create(int device, double map_voxel_size, const o3s_cropper* map_builder_cropper, o3s_submap** out) {
  return submap_create_impl(device, map_voxel_size, map_builder_cropper, /*own_stream=*/false, out);
}

void o3s_submap_destroy(o3s_submap* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  m->pend.active = false;  // nothing will look at the map again; the stream is drained below
  if (m->stream) {
    (void)hipStreamSynchronize(m->stream);
    if (m->owns_stream) (void)hipStreamDestroy(m->stream);
  }
  if (m->handover) (void)hipEventDestroy(m->handover);
  if (m->scan_read) (void)hipEventDestroy(m->scan_read);
  delete m;
}

int64_t o3s_submap_size(const o3s_submap* m) {
  (void)submap_settle(m);  // (an insert that fails while completing leaves the appended cloud: its size is what is reported)
  return m ? m->n : 0;
}
// the size without waiting for a pending insert: exact when none is pending, else [1, map before + scan] (voxelising never empties a cloud)
int o3s_submap_size_bounds(const o3s_submap* m, int64_t* at_least, int64_t* at_most) {
  if (!m || !at_least || !at_most) return O3S_ERR_BAD_ARGUMENT;
  if (m->pend.active) {
    *at_least = m->pend.n_tmp > 0 ? 1 : 0;
    *at_most = m->pend.n_tmp;
  } else {
    *at_least = *at_most = m->n;
  }
  return O3S_OK;
}

int o3s_submap_clone(const o3s_submap* src, int device, o3s_submap** out) {
  if (const int rs_ = submap_settle(src); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!src || !out) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  int rc = submap_create_impl(device, src->voxel, &src->cropper, /*own_stream=*/true, out);  // a snapshot runs beside the mapper
  if (rc != O3S_OK) return rc;
  o3s_submap* m = *out;
  auto fail = [&](int code) {
    o3s_submap_destroy(m);
    *out = nullptr;
    return code;
  };
  if (hipSetDevice(src->device) != hipSuccess || hipStreamSynchronize(src->stream) != hipSuccess) return fail(O3S_ERR_HIP);  // the source is complete
  if (hipSetDevice(m->device) != hipSuccess) return fail(O3S_ERR_HIP);
  const size_t bytes = (size_t)src->n * 24;
  hipStream_t s = m->stream;
  auto copy = [&](DevMem& dst, const DevMem& from) -> bool {
    if (dst.ensure(bytes, 0, s) != hipSuccess) return false;
    if (m->device == src->device) return hipMemcpyAsync(dst.p, from.p, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess;
    return hipMemcpyPeerAsync(dst.p, m->device, from.p, src->device, bytes, s) == hipSuccess;  // over xGMI when the devices are peers
  };
  if (src->n > 0) {
    if (!copy(m->pts[0], src->pts[src->cur])) return fail(O3S_ERR_HIP);
    if (src->has_normals == 1 && !copy(m->nrm[0], src->nrm[src->cur])) return fail(O3S_ERR_HIP);
    if (src->has_colors == 1 && !copy(m->col[0], src->col[src->cur])) return fail(O3S_ERR_HIP);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(O3S_ERR_HIP);
  }
  m->cur = 0;
  m->n = src->n;
  m->has_normals = src->has_normals;
  m->has_colors = src->has_colors;
  m->n_pt = src->n_pt;
  m->layout_valid = src->layout_valid;
  if (src->n_feat > 0) {  // the feature set travels with the snapshot
    const size_t nf = (size_t)src->n_feat;
    auto copy_n = [&](DevMem& dst, const DevMem& from, size_t b) -> bool {
      if (dst.ensure(b, 0, s) != hipSuccess) return false;
      if (m->device == src->device) return hipMemcpyAsync(dst.p, from.p, b, hipMemcpyDeviceToDevice, s) == hipSuccess;
      return hipMemcpyPeerAsync(dst.p, m->device, from.p, src->device, b, s) == hipSuccess;
    };
    if (!copy_n(m->feat_p, src->feat_p, nf * 24) || !copy_n(m->feat_n, src->feat_n, nf * 24) || !copy_n(m->feat_f, src->feat_f, nf * kFpfhDim * 8))
      return fail(O3S_ERR_HIP);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(O3S_ERR_HIP);
  }
  m->n_feat = src->n_feat;
  if (src->n_vox >= 0) {  // ... and so does the occupancy snapshot
    const size_t b = (size_t)src->vox_slots * 8;
    bool ok = m->vox_tab.ensure(b + 8, 0, s) == hipSuccess;  // (+ the counter word behind the slots)
    if (ok) ok = (m->device == src->device ? hipMemcpyAsync(m->vox_tab.p, src->vox_tab.p, b, hipMemcpyDeviceToDevice, s)
                                           : hipMemcpyPeerAsync(m->vox_tab.p, m->device, src->vox_tab.p, src->device, b, s)) == hipSuccess;
    if (!ok || hipStreamSynchronize(s) != hipSuccess) return fail(O3S_ERR_HIP);
    m->vox_slots = src->vox_slots;
    m->vox_size = src->vox_size;
  }
  m->n_vox = src->n_vox;
  return O3S_OK;
}

int o3s_submap_insert_stats(const o3s_submap* m, int64_t* merged, int64_t* sorted, int64_t* fell_back) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m) return O3S_ERR_BAD_ARGUMENT;
  if (merged) *merged = m->n_merged;
  if (sorted) *sorted = m->n_sorted;
  if (fell_back) *fell_back = m->n_fell_back;
  return O3S_OK;
}

int o3s_submap_reserve(o3s_submap* m, int64_t n_points) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || n_points < 0 || n_points > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const size_t bytes = (size_t)n_points * 24;
  for (int k = 0; k < 2; ++k) {
    CK(m->pts[k].ensure(bytes, k == m->cur ? (size_t)m->n * 24 : 0, s));
    CK(m->nrm[k].ensure(bytes, (k == m->cur && m->has_normals == 1) ? (size_t)m->n * 24 : 0, s));
  }
  // the work area of either insert pipeline at that size (the merge takes the map plus a scan of up to 2 x 64 x 2048 points)
  const size_t n = (size_t)n_points, n_s = std::min<size_t>(n, 262144);
  const size_t work = std::max(layout_bytes<VoxelArea>(n, scan_temp_bytes(n_points), sort_temp_bytes(n_points)),
                               layout_bytes<InsertMergeArea>(n, n, n_s, scan_temp_bytes(n_points), sort_temp_bytes((int64_t)n_s),
                                                             merge_temp_bytes(n_points, (int64_t)n_s)));
  if (m->arena.mem.cap < work) CK(m->arena.reserve(work));
  return O3S_OK;
}

int o3s_submap_trim(o3s_submap* m) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m) return O3S_ERR_BAD_ARGUMENT;
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(m->stream));
  // a submap that is no longer inserted into keeps its map cloud ([cur]) and nothing else: the spare ping-pong arrays, the
  // sort / scan work area and the scan staging go back to the allocator (they come back on the next reserve / insert); the patch
  // buffers stay: an ICP handle may still be indexing the last patch on its own stream
  const int spare = 1 - m->cur;
  for (DevMem* a : {&m->pts[spare], &m->nrm[spare], &m->col[spare], &m->scan_p, &m->scan_n, &m->scan_c, &m->carve_scan}) a->release();
  m->arena.release();
  // the feature set stays (a closed submap is what place recognition matches against); its work areas go
  m->feat_w.release();
  // shrink the map arrays themselves to what the map holds (a submap closed by radius at a fraction of the reserved size)
  const size_t need = (size_t)m->n * 24;
  auto shrink = [&](DevMem& a) -> hipError_t {
    if (!a.p || a.cap <= need + need / 8 + 4096) return hipSuccess;
    DevMem q;
    if (q.reset(need + 4096) != hipSuccess) return hipSuccess;  // no room for the copy: keep the large array
    hipError_t e = hipMemcpyAsync(q.p, a.p, need, hipMemcpyDeviceToDevice, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e == hipSuccess) a = std::move(q);
    return e;
  };
  CK(shrink(m->pts[m->cur]));
  // a map without normals / colours keeps none of the reserved room for them (the arrays come back with the next reserve / insert)
  if (m->has_normals == 1) CK(shrink(m->nrm[m->cur]));
  else m->nrm[m->cur].release();
  if (m->has_colors == 1) CK(shrink(m->col[m->cur]));
  else m->col[m->cur].release();
  return O3S_OK;
}

int o3s_submap_hand_over(o3s_submap* from, o3s_submap* to) {
  if (const int rs_ = submap_settle(from); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (const int rt_ = submap_settle(to); rt_ != O3S_OK) return rt_;  // a pending insert is completed first
  if (!from || !to || from == to || from->device != to->device || to->n != 0) return O3S_ERR_BAD_ARGUMENT;
  const int rc = set_dev(from);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(from->stream));
  CK(hipStreamSynchronize(to->stream));
  hipStream_t s = from->stream;
  const int c = from->cur;
  const size_t need = (size_t)from->n * 24;
  DevMem* ff[3] = {from->pts, from->nrm, from->col};
  DevMem* tf[3] = {to->pts, to->nrm, to->col};
  const bool used[3] = {true, from->has_normals == 1, from->has_colors == 1};
  // 1. the closed submap's map into arrays of its own size (the only allocations: a few MB each; nothing has moved if one fails)
  DevMem tight[3];  // (an early return frees them)
  hipError_t e = hipSuccess;
  for (int f = 0; f < 3 && e == hipSuccess; ++f)
    if (used[f] && need > 0 && ff[f][c].p) {
      e = tight[f].reset(need + 4096);
      if (e == hipSuccess) e = hipMemcpyAsync(tight[f].p, ff[f][c].p, need, hipMemcpyDeviceToDevice, s);
    }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return O3S_ERR_HIP;
  // 2. everything else changes hands (a fresh submap holds nothing; one that was reserved gives that back)
  for (int f = 0; f < 3; ++f) {
    tf[f][0] = std::move(ff[f][c]);
    tf[f][1] = std::move(ff[f][1 - c]);
    if (tight[f].p) ff[f][c] = std::move(tight[f]);
  }
  to->cur = 0;
  to->scan_p = std::move(from->scan_p);
  to->scan_n = std::move(from->scan_n);
  to->scan_c = std::move(from->scan_c);
  to->carve_scan = std::move(from->carve_scan);
  to->patch_xyzw = std::move(from->patch_xyzw);
  to->patch_n32 = std::move(from->patch_n32);
  to->d_post = std::move(from->d_post);
  to->arena.mem = std::move(from->arena.mem);
  to->arena.used = from->arena.used = 0;
  return O3S_OK;
}

int64_t o3s_submap_device_bytes(const o3s_submap* m) {
  (void)submap_settle(m);
  if (!m) return 0;
  size_t b = m->arena.mem.cap;
  for (int k = 0; k < 2; ++k) b += m->pts[k].cap + m->nrm[k].cap + m->col[k].cap;
  b += m->scan_p.cap + m->scan_n.cap + m->scan_c.cap + m->carve_scan.cap + m->d_T.cap + m->patch_xyzw.cap + m->patch_n32.cap;
  b += m->vox_tab.cap;
  b += m->feat_p.cap + m->feat_n.cap + m->feat_f.cap + m->feat_w.grid.arena.mem.cap + m->feat_w.grid.cells.cap + m->feat_w.idx.cap + m->feat_w.d2.cap +
       m->feat_w.spfh.cap;
  return (int64_t)b;
}

int o3s_submap_center(const o3s_submap* m, double center[3]) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !center) return O3S_ERR_BAD_ARGUMENT;
  center[0] = center[1] = center[2] = 0.0;
  if (m->n == 0) return O3S_OK;  // open3d ComputeCenter: zero for an empty cloud
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const int G = (int)std::min<int64_t>(256, (m->n + kB - 1) / kB);
  DevMem part;
  CK(part.alloc((size_t)G * 24));
  hipLaunchKernelGGL(k_center_part, dim3(G), dim3(kB), 0, s, (const double*)m->pts[m->cur].as<double>(), m->n, part.as<double>());
  CK(hipGetLastError());
  double h[256 * 3];
  CK(hipMemcpyAsync(h, part.p, (size_t)G * 24, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  for (int a = 0; a < 3; ++a) {
    double t = 0.0;
    for (int b = 0; b < G; ++b) t += h[b * 3 + a];
    center[a] = t / (double)m->n;
  }
  return O3S_OK;
}

int o3s_transform_cloud(int device, const double T[16], const double* pts, const double* normals, const double* covariances, int64_t N,
                        double* out_pts, double* out_normals, double* out_covariances, int64_t* n_out) {
  if (!T || !n_out || N < 0 || (N > 0 && (!pts || !out_pts)) || (normals && !out_normals) || (covariances && !out_covariances)) return O3S_ERR_BAD_ARGUMENT;
  *n_out = 0;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  double dev = 0.0;  // (T - Identity).array().abs().maxCoeff()
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) dev = std::max(dev, std::fabs(T[c * 4 + r] - (r == c ? 1.0 : 0.0)));
  const int64_t lead = dev < 1e-4 ? N : 0;  // "*out = cloud" first (helpers.cpp:285-288), the loop below appends regardless
  hipStream_t s = nullptr;
  DevMem a, b, c, d, e, f, t;
  CK(a.alloc((size_t)N * 24));
  CK(d.alloc((size_t)N * 24));
  CK(t.alloc(128));
  CK(hipMemcpyAsync(a.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(t.p, T, 128, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(b.alloc((size_t)N * 24));
    CK(e.alloc((size_t)N * 24));
    CK(hipMemcpyAsync(b.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_transform_append, dim3(nblk(N)), dim3(kB), 0, s, a.as<double>(), normals ? b.as<double>() : nullptr, N, t.as<double>(),
                     d.as<double>(), e.as<double>());
  if (covariances) {
    CK(c.alloc((size_t)N * 72));
    CK(f.alloc((size_t)N * 72));
    CK(hipMemcpyAsync(c.p, covariances, (size_t)N * 72, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_transform_cov, dim3(nblk(N)), dim3(kB), 0, s, c.as<double>(), N, t.as<double>(), f.as<double>());
  }
  CK(hipGetLastError());
  if (lead) {
    std::memcpy(out_pts, pts, (size_t)N * 24);
    if (normals) std::memcpy(out_normals, normals, (size_t)N * 24);
    if (covariances) std::memcpy(out_covariances, covariances, (size_t)N * 72);
  }
  CK(hipMemcpyAsync(out_pts + 3 * lead, d.p, (size_t)N * 24, hipMemcpyDeviceToHost, s));
  if (normals) CK(hipMemcpyAsync(out_normals + 3 * lead, e.p, (size_t)N * 24, hipMemcpyDeviceToHost, s));
  if (covariances) CK(hipMemcpyAsync(out_covariances + 9 * lead, f.p, (size_t)N * 72, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *n_out = lead + N;
  return O3S_OK;
}

int o3s_submap_upload(o3s_submap* m, const double* pts, const double* normals, int64_t N) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || N < 0 || (N > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  CK(m->pts[m->cur].ensure((size_t)N * 24, 0, s));
  if (N) CK(hipMemcpyAsync(m->pts[m->cur].p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(m->nrm[m->cur].ensure((size_t)N * 24, 0, s));
    if (N) CK(hipMemcpyAsync(m->nrm[m->cur].p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  CK(hipStreamSynchronize(s));
  m->n = N;
  m->layout_valid = false;
  m->has_normals = N == 0 ? -1 : (normals ? 1 : 0);
  m->has_colors = 0;  // an uploaded map comes without colours
  m->n_feat = -1;     // and without the features of the map it replaces
  return O3S_OK;
}

int o3s_submap_download(const o3s_submap* m, double* pts, double* normals) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || (m->n > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  if (m->n == 0) return O3S_OK;
  if (hipSetDevice(m->device) != hipSuccess) return O3S_ERR_HIP;
  CK(hipStreamSynchronize(m->stream));
  CK(hipMemcpy(pts, m->pts[m->cur].p, (size_t)m->n * 24, hipMemcpyDeviceToHost));
  if (normals) {
    if (m->has_normals != 1) return O3S_ERR_BAD_SHAPE;
    CK(hipMemcpy(normals, m->nrm[m->cur].p, (size_t)m->n * 24, hipMemcpyDeviceToHost));
  }
  return O3S_OK;
}

namespace {
// every word finite, and a last row that is not (0, 0, 0, 0) (v(3) would be zero for every point)
bool transform_valid(const double* T) {
  if (!T) return false;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(T[k])) return false;
  return !(T[3] == 0.0 && T[7] == 0.0 && T[11] == 0.0 && T[15] == 0.0);
}
// enqueues the in-place transform of a settled, non-empty submap on its own stream and drops what was derived from the coordinates
int submap_transform_enqueue(o3s_submap* m, const double* T) {
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  Pose4d Tv;
  for (int k = 0; k < 16; ++k) Tv.m[k] = T[k];
  const int c = m->cur;  // whichever ping-pong array is current (a closed submap's tight copy)
  const int64_t nf = m->n_feat > 0 ? m->n_feat : 0;
  hipLaunchKernelGGL(k_submap_transform, dim3(nblk(m->n + nf)), dim3(kB), 0, m->stream, m->pts[c].as<double>(), m->has_normals == 1 ? m->nrm[c].as<double>() : nullptr,
                     m->n, nf ? m->feat_p.as<double>() : nullptr, nf ? m->feat_n.as<double>() : nullptr, nf, Tv);
  CK(hipGetLastError());
  // The voxel order of the map array is the order of the OLD coordinates: the next insert sorts, and tries the merge right after
  // (a back-off counted revisits of the old frame).  The patch buffers and the feature work area (grid, lists, SPFH) carry no
  // validity state: o3s_submap_set_reference and o3s_submap_compute_features rebuild them from the map on every call.
  m->layout_valid = false;
  m->merge_backoff = 0;
  return O3S_OK;
}
}  // namespace

int o3s_submap_transform(o3s_submap* m, const double T[16]) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !transform_valid(T)) return O3S_ERR_BAD_ARGUMENT;
  if (m->n == 0) return O3S_OK;  // (a feature set of an empty map is empty)
  const int rc = submap_transform_enqueue(m, T);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(m->stream));  // registrations read the map from other streams
  return O3S_OK;
}

int o3s_submaps_transform(int32_t n, o3s_submap* const* maps, const double* T) {
  if (n < 0 || (n > 0 && (!maps || !T))) return O3S_ERR_BAD_ARGUMENT;
  // everything is checked before the first launch: a bad argument changes no submap
  for (int32_t i = 0; i < n; ++i) {
    if (!maps[i] || !transform_valid(T + 16 * (size_t)i)) return O3S_ERR_BAD_ARGUMENT;
    for (int32_t j = 0; j < i; ++j)
      if (maps[j] == maps[i]) return O3S_ERR_BAD_ARGUMENT;
  }
  for (int32_t i = 0; i < n; ++i)
    if (const int rs_ = submap_settle(maps[i]); rs_ != O3S_OK) return rs_;  // pending inserts are completed first
  int rc = O3S_OK;
  int32_t issued = 0;
  for (; issued < n && rc == O3S_OK; ++issued)
    if (maps[issued]->n > 0) rc = submap_transform_enqueue(maps[issued], T + 16 * (size_t)issued);
  // the one wait: each stream that was given work is drained, after the last launch (submaps share the streams of their device)
  for (int32_t i = 0; i < issued; ++i) {
    if (maps[i]->n == 0) continue;
    bool seen = false;
    for (int32_t j = 0; j < i && !seen; ++j) seen = maps[j]->n > 0 && maps[j]->stream == maps[i]->stream && maps[j]->device == maps[i]->device;
    if (seen) continue;
    if (hipSetDevice(maps[i]->device) != hipSuccess || hipStreamSynchronize(maps[i]->stream) != hipSuccess) rc = rc == O3S_OK ? O3S_ERR_HIP : rc;
  }
  return rc;
}

namespace {
// What is left of an insert once the merge path has answered (merged: its counts) or was not tried: the sort-based pipelines where
// needed, then the submap's new state.  The appended cloud [old map | scan] is in pts[c], the voxelised map goes to pts[1 - c].
int insert_finish(o3s_submap* m, int c, int64_t n_tmp, bool hn, bool have_vh, const VoxHint& vh, bool merged, const int64_t cnt_m[2]) {
  hipStream_t s = m->stream;
  Attrs at;
  if (m->has_colors == 1) {
    at.col = m->col[c].as<double>();
    at.out_col = m->col[1 - c].as<double>();
  }
  int rc = O3S_OK;
  bool hinted = merged;
  int64_t n_out = merged ? cnt_m[0] + cnt_m[1] : 0, n_pt_new = merged ? cnt_m[0] : 0;
  if (!hinted && have_vh) {
    int64_t cnt[3];
    rc = voxel_pipeline_hint_dev(m->arena, 0, &m->cropper, vh, m->voxel, m->pts[c].as<double>(), hn ? m->nrm[c].as<double>() : nullptr, n_tmp, m->pts[1 - c].as<double>(),
                                 m->nrm[1 - c].as<double>(), nullptr, &at, nullptr, nullptr, nullptr, cnt, &hinted, s);
    if (rc == O3S_OK && hinted) {
      n_out = cnt[0] + cnt[1];
      n_pt_new = cnt[0];
      ++m->n_sorted;
    }
  }
  m->layout_valid = false;
  if (rc == O3S_OK && !hinted)
    rc = voxel_pipeline_dev(m->arena, 0, &m->cropper, m->voxel, m->pts[c].as<double>(), hn ? m->nrm[c].as<double>() : nullptr, n_tmp, m->pts[1 - c].as<double>(),
                            m->nrm[1 - c].as<double>(), nullptr, &n_out, s, &at);
  if (rc != O3S_OK) {
    m->n = n_tmp;  // the appended cloud is still a valid map
    return rc;
  }
  CK(hipStreamSynchronize(s));
  m->cur = 1 - c;
  m->n = n_out;
  if (hinted) {  // the hinted pipelines emit [pass-through | voxels in key order] and say how many of each
    m->n_pt = n_pt_new;
    m->layout_valid = true;
  }
  return O3S_OK;
}

// Completes a pending insert (o3s_submap::PendingInsert); a no-op otherwise.  Every entry point that looks at or changes the map
// calls it first, so nothing outside ever sees the state in between.
int submap_settle(o3s_submap* m) {
  if (!m || !m->pend.active) return O3S_OK;
  const o3s_submap::PendingInsert p = m->pend;
  m->pend.active = false;
  if (hipSetDevice(m->device) != hipSuccess) return O3S_ERR_HIP;
  int64_t cnt[2];
  bool merged = false;
  const int rc = voxel_insert_merge_result(p.post, cnt, &merged);
  if (rc != O3S_OK) {
    m->n = p.n_tmp;
    return rc;
  }
  if (merged) ++m->n_merged;
  else {  // old pass-through points are back inside the volume (a revisit): that lasts for a while
    ++m->n_fell_back;
    m->merge_backoff = 4;
  }
  return insert_finish(m, p.c, p.n_tmp, p.hn, true, p.vh, merged, cnt);
}
// Submap::insertScan on a scan that already lives in HBM (d_pts / d_nrm: 3 x N doubles)
// lazy: the call may return with the insert enqueued and its completion pending (submap_settle)
// read_done (nullable): recorded on the submap's stream as soon as nothing enqueued here reads d_pts / d_nrm / d_col any more
int insert_dev(o3s_submap* m, const double* d_pts, const double* d_nrm, int64_t N, const double T_map_sensor[16], const double* d_col = nullptr,
               bool lazy = false, hipEvent_t read_done = nullptr) {
  hipStream_t s = m->stream;
  const bool hn = d_nrm != nullptr;
  // (T - Identity).array().abs().maxCoeff() < 1e-4: the reference copies the input cloud into the output and then
  // STILL appends the transformed points (helpers.cpp:285-288, 300-304) — the scan enters the map twice.  Kept as is.
  double dev = 0.0;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) dev = std::max(dev, std::fabs(T_map_sensor[c * 4 + r] - (r == c ? 1.0 : 0.0)));
  const bool doubled = dev < 1e-4;
  const int64_t add = doubled ? 2 * N : N;
  const int64_t n_tmp = m->n + add;
  if (n_tmp > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  Pose4d Tv;
  for (int k = 0; k < 16; ++k) Tv.m[k] = T_map_sensor[k];
  const int c = m->cur;
  CK(m->pts[c].ensure((size_t)n_tmp * 24, (size_t)m->n * 24, s));
  if (hn) CK(m->nrm[c].ensure((size_t)n_tmp * 24, (size_t)m->n * 24, s));
  // mapCloud_ += *transformedCloud (Submap.cpp:85)
  double* dst_p = m->pts[c].as<double>() + 3 * m->n;
  double* dst_n = hn ? m->nrm[c].as<double>() + 3 * m->n : nullptr;
  if (doubled) {
    CK(hipMemcpyAsync(dst_p, d_pts, (size_t)N * 24, hipMemcpyDeviceToDevice, s));
    if (hn) CK(hipMemcpyAsync(dst_n, d_nrm, (size_t)N * 24, hipMemcpyDeviceToDevice, s));
    dst_p += 3 * N;
    if (hn) dst_n += 3 * N;
  }
  hipLaunchKernelGGL(k_transform_append_v, dim3(nblk(N)), dim3(kB), 0, s, d_pts, d_nrm, N, Tv, dst_p, dst_n);
  CK(hipGetLastError());
  m->has_normals = hn ? 1 : 0;
  // Colours.  o3d_slam::transform copies them (out->colors_ = cloud.colors_, helpers.cpp:291) — N colours also when the
  // almost-identity quirk has doubled the points, so that cloud no longer "HasColors()" — and Open3D's
  // PointCloud::operator+= keeps the map's colours only if (map empty or map has colours) and the added cloud has them;
  // otherwise it clears them for good.
  {
    const bool scan_has = d_col != nullptr && !doubled;
    const bool keep_colors = (m->n == 0 || m->has_colors == 1) && scan_has;
    if (keep_colors) {
      CK(m->col[c].ensure((size_t)n_tmp * 24, (size_t)m->n * 24, s));
      CK(hipMemcpyAsync(m->col[c].as<double>() + 3 * m->n, d_col, (size_t)N * 24, hipMemcpyDeviceToDevice, s));
    }
    m->has_colors = keep_colors ? 1 : 0;
  }
  if (read_done) CK(hipEventRecord(read_done, s));  // the scan has been taken in: from here on only the map's own arrays are read
  // mapBuilderCropper_->setPose(mapToRangeSensor) (Submap.cpp:86)
  for (int d = 0; d < 3; ++d) m->cropper.centre[d] = T_map_sensor[12 + d];
  if (!(m->voxel > 0.0)) {  // "Map voxel size is zero. Not voxelizing the map." (Submap.cpp:164-166)
    m->n = n_tmp;
    m->layout_valid = false;
    CK(hipStreamSynchronize(s));
    return O3S_OK;
  }
  // voxelizeInsideCroppingVolume: *map = *voxelizeWithinCroppingVolume(voxel, cropper, *map) (Submap.cpp:159-163)
  CK(m->pts[1 - c].ensure((size_t)n_tmp * 24, 0, s));
  CK(m->nrm[1 - c].ensure((size_t)n_tmp * 24, 0, s));
  if (m->has_colors == 1) CK(m->col[1 - c].ensure((size_t)n_tmp * 24, 0, s));
  int rc = O3S_OK;
  bool merged = false;
  int64_t cnt_m[2] = {0, 0};
  const int64_t n_old = m->n;
  VoxHint vh{};
  bool have_vh = false;
  {  // a bounded map-builder volume bounds the voxel indices: no extrema, one read-back (cloud_dev.h, "hinted")
    double lo[3], hi[3];
    have_vh = hints_enabled() && cropper_aabb(m->cropper, lo, hi) && vox_hint(0, lo, hi, m->voxel, &vh);
    if (have_vh) {
      // the map is already in voxel order: merge the (sorted) scan into it instead of sorting everything again
      if (m->merge_backoff > 0) --m->merge_backoff;
      else if (m->layout_valid && m->has_colors != 1 && n_old > m->n_pt && O3S_HOOK_ENV("O3S_INSERT_SORT") == nullptr) {
        LazyPost lp;
        bool issued = false;
        bool can_lazy = lazy && O3S_HOOK_ENV("O3S_INSERT_EAGER") == nullptr;
        if (can_lazy) {
          CK(m->d_post.ensure(64, 0, s));
          can_lazy = lazy_post_open(pinned_area(), reinterpret_cast<uint32_t*>(m->d_post.as<double>()), s, &lp);
        }
        rc = voxel_insert_merge_dev(m->arena, m->cropper, vh, m->voxel, m->pts[c].as<double>(), hn ? m->nrm[c].as<double>() : nullptr, m->n_pt, n_old, n_tmp,
                                    m->pts[1 - c].as<double>(), m->nrm[1 - c].as<double>(), cnt_m, &merged, s, can_lazy ? &lp : nullptr, &issued);
        if (rc == O3S_OK && issued) {  // the answer is on its way: submap_settle() takes it from here
          m->layout_valid = false;
          m->pend.active = true;
          m->pend.post = lp;
          m->pend.c = c;
          m->pend.n_tmp = n_tmp;
          m->pend.hn = hn;
          m->pend.vh = vh;
          return O3S_OK;
        }
        if (rc == O3S_OK && merged) ++m->n_merged;
        else if (rc == O3S_OK) {  // old pass-through points are back inside the volume (a revisit): that lasts for a while
          ++m->n_fell_back;
          m->merge_backoff = 4;
        }
      }
    }
  }
  if (rc != O3S_OK) {
    m->layout_valid = false;
    m->n = n_tmp;  // the appended cloud is still a valid map
    return rc;
  }
  return insert_finish(m, c, n_tmp, hn, have_vh, vh, merged, cnt_m);
}
}  // namespace

int o3s_submap_insert_scan(o3s_submap* m, const double* pts, const double* normals, int64_t N, const double T_map_sensor[16]) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || N < 0 || !T_map_sensor || (N > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;  // "if (preProcessedScan.IsEmpty()) return true" (Submap.cpp:41-43)
  if (m->has_normals >= 0 && m->has_normals != (normals ? 1 : 0)) return O3S_ERR_BAD_SHAPE;
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  CK(m->scan_p.ensure((size_t)N * 24, 0, s));
  CK(hipMemcpyAsync(m->scan_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(m->scan_n.ensure((size_t)N * 24, 0, s));
    CK(hipMemcpyAsync(m->scan_n.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  return insert_dev(m, m->scan_p.as<double>(), normals ? m->scan_n.as<double>() : nullptr, N, T_map_sensor);
}

int o3s_submap_insert_scan_colored(o3s_submap* m, const double* pts, const double* normals, const double* colors, int64_t N,
                                   const double T_map_sensor[16]) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!colors) return o3s_submap_insert_scan(m, pts, normals, N, T_map_sensor);
  if (!m || N < 0 || !T_map_sensor || (N > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  if (m->has_normals >= 0 && m->has_normals != (normals ? 1 : 0)) return O3S_ERR_BAD_SHAPE;
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  CK(m->scan_p.ensure((size_t)N * 24, 0, s));
  CK(hipMemcpyAsync(m->scan_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(m->scan_n.ensure((size_t)N * 24, 0, s));
    CK(hipMemcpyAsync(m->scan_n.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  CK(m->scan_c.ensure((size_t)N * 24, 0, s));
  CK(hipMemcpyAsync(m->scan_c.p, colors, (size_t)N * 24, hipMemcpyHostToDevice, s));
  return insert_dev(m, m->scan_p.as<double>(), normals ? m->scan_n.as<double>() : nullptr, N, T_map_sensor, m->scan_c.as<double>());
}

int o3s_submap_has_colors(const o3s_submap* m) {
  (void)submap_settle(m);
  return m && m->n > 0 && m->has_colors == 1 ? 1 : 0;
}

int o3s_submap_download_colors(const o3s_submap* m, double* colors) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !colors) return O3S_ERR_BAD_ARGUMENT;
  if (m->n == 0) return O3S_OK;
  if (m->has_colors != 1) return O3S_ERR_BAD_SHAPE;
  if (hipSetDevice(m->device) != hipSuccess) return O3S_ERR_HIP;
  CK(hipStreamSynchronize(m->stream));
  CK(hipMemcpy(colors, m->col[m->cur].p, (size_t)m->n * 24, hipMemcpyDeviceToHost));
  return O3S_OK;
}

// removeByIds on a settled submap (space carving, the outlier filters): SelectByIndex(ids, invert) keeps the survivors in their
// order.  keep: one flag per map point, off: its exclusive scan, n_keep: the number set — on the submap's device, written on its
// stream.  The survivors go to the other half of the ping-pong, normals and colours with them; the call returns on a drained stream
static int submap_keep_flagged(o3s_submap* m, const uint32_t* keep, const uint32_t* off, int64_t n_keep) {
  const int64_t Nm = m->n;
  if (n_keep >= Nm) return O3S_OK;
  hipStream_t s = m->stream;
  const int c = m->cur;
  const bool hn = m->has_normals == 1;
  CK(m->pts[1 - c].ensure((size_t)Nm * 24, 0, s));
  CK(m->nrm[1 - c].ensure((size_t)Nm * 24, 0, s));
  hipLaunchKernelGGL(k_compact, dim3(nblk(Nm)), dim3(kB), 0, s, m->pts[c].as<double>(), hn ? m->nrm[c].as<double>() : nullptr, Nm, keep, off, m->pts[1 - c].as<double>(),
                     m->nrm[1 - c].as<double>(), (int32_t*)nullptr);
  if (m->has_colors == 1) {  // SelectByIndex carries the colours along
    CK(m->col[1 - c].ensure((size_t)Nm * 24, 0, s));
    hipLaunchKernelGGL(k_compact_attr, dim3(nblk(Nm)), dim3(kB), 0, s, (const double*)m->col[c].as<double>(), (const double*)nullptr, Nm, keep, off,
                       m->col[1 - c].as<double>(), (double*)nullptr);
  }
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s));
  m->cur = 1 - c;
  m->n = n_keep;
  m->layout_valid = false;  // order is kept, but how many pass-through points survived is not known here
  return O3S_OK;
}

int o3s_submap_carve(o3s_submap* m, const o3s_carving_params* cp, const double* raw_pts, int64_t N, const double T_map_sensor[16], int64_t* n_removed) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (n_removed) *n_removed = 0;
  if (!m || !cp || !T_map_sensor || N < 0 || (N > 0 && !raw_pts) || !(cp->voxel_size > 0.0)) return O3S_ERR_BAD_ARGUMENT;
  if (m->n == 0 || N == 0) return O3S_OK;  // "if (map->points_.empty() ...) return" (Submap.cpp:118-120)
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  const int64_t Nm = m->n;
  const bool hn = m->has_normals == 1;
  const int c = m->cur;
  // scan = transform(mapToRangeSensor, rawScan) (Submap.cpp:122)
  CK(m->scan_p.ensure((size_t)N * 24, 0, s));
  CK(m->carve_scan.ensure((size_t)N * 24, 0, s));
  CK(m->d_T.ensure(128, 0, s));
  CK(hipMemcpyAsync(m->scan_p.p, raw_pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(m->d_T.p, T_map_sensor, 128, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_transform_append, dim3(nblk(N)), dim3(kB), 0, s, m->scan_p.as<double>(), (const double*)nullptr, N, m->d_T.as<double>(), m->carve_scan.as<double>(),
                     (double*)nullptr);
  // wideCroppedIdxs = cropper.getIndicesWithinVolume(*map): the map-builder cropper at the pose of the previous insert
  const size_t nm = (size_t)Nm;
  const size_t tb_scan = scan_temp_bytes(Nm), tb_sort = sort_temp_bytes(Nm);
  CarveArea w;
  CK(lay_out(m->arena, w, nm, tb_scan, tb_sort));
  hipLaunchKernelGGL(k_mask, dim3(nblk(Nm)), dim3(kB), 0, s, m->cropper, m->pts[c].as<double>(), Nm, 1, w.inflag);
  int64_t n_in = 0;
  rc = scan_flags(w.inflag, w.off, Nm, w.tmp, tb_scan, &n_in, s);
  if (rc != O3S_OK) return rc;
  if (n_in == 0) return O3S_OK;
  const double inv = 1.0 / cp->voxel_size;
  rc = ext_i32_init(w.d_mm, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_carve_box, dim3(nblk(Nm)), dim3(kB), 0, s, m->pts[c].as<double>(), Nm, w.inflag, inv, w.d_mm);
  int32_t mm[6];
  rc = ext_i32_fetch(w.d_mm, mm, s);
  if (rc != O3S_OK) return rc;
  if (mm[0] > mm[3]) return O3S_OK;  // no point of the subset is in a voxel (all of them non-finite): nothing can be carved
  const int64_t ex = (int64_t)mm[3] - mm[0] + 1, ey = (int64_t)mm[4] - mm[1] + 1, ez = (int64_t)mm[5] - mm[2] + 1;
  if ((long double)ex * (long double)ey * (long double)ez >= 9.0e18L) return O3S_ERR_BAD_ARGUMENT;
  // sort bits: the packed range plus one bit for the key of the points outside the volume (the whole map is sorted: nine passes
  // with all 64 bits, three or four with the range that is known here)
  const int kb = key_bits((uint64_t)ex * (uint64_t)ey * (uint64_t)ez);
  const uint64_t out_key = kb < 63 ? (1ull << kb) : ~0ull;
  hipLaunchKernelGGL(k_carve_keys, dim3(nblk(Nm)), dim3(kB), 0, s, m->pts[c].as<double>(), Nm, w.inflag, inv, mm[0], mm[1], mm[2], (uint64_t)ex, (uint64_t)ey, out_key,
                     w.keys, w.vals);
  size_t tb = tb_sort;
  CK(sort_pairs(w.tmp, tb, w.keys, w.keys2, w.vals, w.vals2, nm, kb < 63 ? kb + 1 : 64, s));
  CK(hipMemsetAsync(w.remove, 0, nm * 4, s));
  hipLaunchKernelGGL(k_carve_rays, dim3(nblk(N)), dim3(kB), 0, s, m->carve_scan.as<double>(), N, T_map_sensor[12], T_map_sensor[13], T_map_sensor[14],
                     cp->voxel_size, inv, cp->max_raytracing_length, cp->truncation_distance, cp->min_dot_product_with_normal, w.keys2, w.vals2, n_in, mm[0],
                     mm[1], mm[2], ex, ey, ez, hn ? m->nrm[c].as<double>() : nullptr, w.remove);
  // removeByIds: SelectByIndex(ids, invert) keeps the survivors in their order
  hipLaunchKernelGGL(k_invert_flags, dim3(nblk(Nm)), dim3(kB), 0, s, w.remove, Nm, w.keep);
  int64_t n_keep = 0;
  rc = scan_flags(w.keep, w.off, Nm, w.tmp, tb_scan, &n_keep, s);
  if (rc != O3S_OK) return rc;
  rc = submap_keep_flagged(m, w.keep, w.off, n_keep);
  if (rc != O3S_OK) return rc;
  if (n_removed) *n_removed = Nm - n_keep;
  return O3S_OK;
}

int o3s_submap_patch_count(o3s_submap* m, const o3s_cropper* scan_matcher_cropper, const double T_map_sensor[16], int64_t* n_patch) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !scan_matcher_cropper || !T_map_sensor || !n_patch) return O3S_ERR_BAD_ARGUMENT;
  *n_patch = 0;
  if (m->n == 0) return O3S_OK;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  o3s_cropper c = *scan_matcher_cropper;  // scanMatcherCropper_->setPose(mapToRangeSensor)
  for (int d = 0; d < 3; ++d) c.centre[d] = T_map_sensor[12 + d];
  const int64_t N = m->n;
  const size_t tb = scan_temp_bytes(N);
  CropArea w;
  CK(lay_out(m->arena, w, (size_t)N, tb));
  uint32_t* blk = reinterpret_cast<uint32_t*>(w.tmp);
  hipLaunchKernelGGL(k_mask, dim3(nblk(N)), dim3(kB), 0, s, c, (const double*)m->pts[m->cur].as<double>(), N, 1, w.flag, (uint32_t*)nullptr, blk);
  return scan_flags(w.flag, w.off, N, w.tmp, tb, n_patch, s, blk);
}

int o3s_submap_set_reference(o3s_submap* m, const o3s_cropper* scan_matcher_cropper, const double T_map_sensor[16], o3s_icp* icp,
                             int64_t* n_patch) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (n_patch) *n_patch = 0;
  if (!m || !scan_matcher_cropper || !T_map_sensor || !icp) return O3S_ERR_BAD_ARGUMENT;
  if (m->n == 0) return O3S_ERR_EMPTY_REFERENCE;
  int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  // The previous patch may still be read by the handle's asynchronous index build when a compute failed before anything
  // waited for its stream (ERR_NOT_RIGID, an empty reading: the Mapper keeps the prior and goes on): the patch buffers are
  // rewritten below, so the handle's stream is drained first.  It is idle in the normal course of a scan.
  rc = o3s_icp_synchronize(icp);
  if (rc != O3S_OK) return rc;
  hipStream_t s = m->stream;
  o3s_cropper c = *scan_matcher_cropper;  // scanMatcherCropper_->setPose(mapToRangeSensor)
  for (int d = 0; d < 3; ++d) c.centre[d] = T_map_sensor[12 + d];
  const bool hn = m->has_normals == 1;
  // cropSubmap + open3dToPointmatcher in one compaction: mask, scan, then the kept points straight into fp32.  The COUNT stays on
  // the device: the compaction is launched for all N points into buffers that hold N, its last thread leaves the count behind the
  // offsets, and the index build reads it there — the host learns it from the post of the reference's statistics, which it waits
  // for anyway (round 4: a hand-over of the count first, then one of the statistics: two waits, ~15 us of every re-init)
  int64_t kept = 0;
  uint32_t* d_count = nullptr;
  const int64_t N = m->n;
  {
    const size_t tb = scan_temp_bytes(N);
    CropArea w;
    CK(lay_out(m->arena, w, (size_t)N, tb));
    uint32_t* blk = reinterpret_cast<uint32_t*>(w.tmp);  // the mask's per-block counts: the scan is one launch (cloud_dev.h k_scan_flags_blk)
    hipLaunchKernelGGL(k_mask, dim3(nblk(N)), dim3(kB), 0, s, c, (const double*)m->pts[m->cur].as<double>(), N, 1, w.flag, (uint32_t*)nullptr, blk);
    rc = scan_flags_dev(w.flag, w.off, N, w.tmp, tb, s, blk);
    if (rc != O3S_OK) return rc;
    CK(m->patch_xyzw.ensure((size_t)N * 16, 0, s));
    CK(m->patch_n32.ensure((size_t)N * 12, 0, s));
    d_count = w.off + N;
    hipLaunchKernelGGL(k_compact_pm, dim3(nblk(N)), dim3(kB), 0, s, (const double*)m->pts[m->cur].as<double>(), hn ? (const double*)m->nrm[m->cur].as<double>() : nullptr, N,
                       w.flag, w.off, reinterpret_cast<float4*>(m->patch_xyzw.p), reinterpret_cast<float*>(m->patch_n32.p), d_count);
    CK(hipGetLastError());
  }
  // the ICP handle works on its own stream: it waits for the patch on the device, and reads it asynchronously — the patch
  // buffers (and the count word in this submap's work area) are not touched again before the next call on this submap, which the
  // host only reaches after a compute has waited
  CK(hipEventRecord(m->handover, s));
  rc = o3s_icp_wait_event(icp, m->handover);
  if (rc != O3S_OK) return rc;
  rc = o3s_icp_init_reference_dev_counted_async(icp, m->patch_xyzw.p, hn ? m->patch_n32.p : nullptr, d_count, N, &kept);
  if (n_patch) *n_patch = kept;
  return rc;
}

// RegistrationICP between two resident submaps: nothing is uploaded; the source cloud is copied inside HBM (the
// iteration transforms it in place), the target and its normals are read where they lie
int o3s_o3d_registration_icp_submaps(const o3s_submap* source, const o3s_submap* target, double max_dist, const double init[16],
                                     const o3s_o3d_icp_criteria* criteria, o3s_o3d_icp_result* result, double* info36) {
  if (const int rs_ = submap_settle(source); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (const int rt_ = submap_settle(target); rt_ != O3S_OK) return rt_;  // a pending insert is completed first
  if (!source || !target || !init || !result || !(max_dist > 0.0)) return O3S_ERR_BAD_ARGUMENT;
  if (source->device != target->device) return O3S_ERR_BAD_ARGUMENT;
  if (source->n == 0 || target->n == 0) return O3S_ERR_EMPTY_REFERENCE;
  if (target->has_normals != 1) return O3S_ERR_BAD_SHAPE;  // "requires target pointcloud to have normals"
  int rc = set_dev(target);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(source->stream));
  CK(hipStreamSynchronize(target->stream));
  hipStream_t s = target->stream;
  o3s_cloud::RegLease area(target->device, s);
  rc = o3d_icp_run(area->reg, source->pts[source->cur].as<double>(), source->n, target->pts[target->cur].as<double>(), target->nrm[target->cur].as<double>(), target->n,
                   max_dist, init, criteria, result, s, /*on_device=*/true);
  if (rc == O3S_OK && info36) rc = o3d_info_after_icp(area->reg, max_dist, result->transformation, info36, s);
  return area.end(rc);
}

// ---- device-resident pre-processed scan (include/o3s_scan.h) ---------------------------------------------------------
}  // extern "C"

struct o3s_scan {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t handover = nullptr;  // recorded on `stream`, waited for by the ICP handle's stream
  DevMem raw_p, raw_n, tmp_p, tmp_n, wide_p, wide_n, narrow_p, narrow_n, xyzw, n32;
  int64_t n_wide = 0, n_narrow = 0, n_raw = 0;  // n_raw: the raw scan of the last preprocess, still in raw_p (/ raw_n)
  int raw_has_normals = 0;
  double normal_radius = 0.0;
  int32_t normal_knn = 0;
  bool voxel_ordered = false;  // the last preprocess down-sampled: merge / match clouds are in (z, y, x) voxel order
  bool pm_ready = false;       // ... and already wrote the match cloud in the PM layout (xyzw / n32)
  Arena arena;
  NormalsWork nwork;
};

// A raw scan staged in HBM ahead of the mapping call (include/o3s_scan.h: o3s_raw_scan)
struct o3s_raw_scan {
  int device = 0;
  hipStream_t stream = nullptr;
  DevMem p, n;
  int64_t N = 0;
  int has_normals = 0;
  DevMem dt, traj;      // per-point time offsets of this sweep (o3s_raw_scan_set_point_times); the table of the last trajectory de-skew
  int has_times = 0;  // dropped by the next upload
};

extern "C" {

int o3s_raw_scan_create(int device, o3s_raw_scan** out) {
  if (!out) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  o3s_raw_scan* r = new o3s_raw_scan();
  r->device = device;
  if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) {
    delete r;
    return O3S_ERR_HIP;
  }
  *out = r;
  return O3S_OK;
}

void o3s_raw_scan_destroy(o3s_raw_scan* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) {
    (void)hipStreamSynchronize(r->stream);
    (void)hipStreamDestroy(r->stream);
  }
  delete r;
}

int o3s_raw_scan_upload(o3s_raw_scan* r, const double* pts, const double* normals, int64_t N) {
  if (!r || N < 0 || (N > 0 && !pts) || N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  r->N = 0;
  r->has_times = 0;
  if (N == 0) return O3S_OK;
  if (hipSetDevice(r->device) != hipSuccess) return O3S_ERR_HIP;
  hipStream_t s = r->stream;
  CK(r->p.ensure((size_t)N * 24, 0, s));
  CK(hipMemcpyAsync(r->p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  if (normals) {
    CK(r->n.ensure((size_t)N * 24, 0, s));
    CK(hipMemcpyAsync(r->n.p, normals, (size_t)N * 24, hipMemcpyHostToDevice, s));
  }
  CK(hipStreamSynchronize(s));  // the caller's arrays are free again, the staged copy is complete
  r->N = N;
  r->has_normals = normals ? 1 : 0;
  return O3S_OK;
}

int64_t o3s_raw_scan_size(const o3s_raw_scan* r) { return r ? r->N : -1; }

// undistortInputPointCloud on the staged sweep, in place (undistort_dev.h): points only, the staged normals stay as they are
int o3s_raw_scan_undistort(o3s_raw_scan* r, const o3s_motion* m) {
  if (!r || !motion_valid(m)) return O3S_ERR_BAD_ARGUMENT;
  if (r->N == 0 || motion_is_zero(*m)) return O3S_OK;
  if (hipSetDevice(r->device) != hipSuccess) return O3S_ERR_HIP;
  const int rc = undistort_dev(r->p.as<double>(), r->N, *m, r->stream);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(r->stream));  // the pre-process reads the staged copy from another stream
  return O3S_OK;
}

// include/trajectory/o3s_trajectory.h: the driver's per-point time offsets of the staged sweep
int o3s_raw_scan_set_point_times(o3s_raw_scan* r, const double* dt, int64_t N) {
  if (!r || N != r->N || (N > 0 && !dt)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  if (hipSetDevice(r->device) != hipSuccess) return O3S_ERR_HIP;
  r->has_times = 0;
  CK(r->dt.ensure((size_t)N * 8, 0, r->stream));
  CK(hipMemcpyAsync(r->dt.p, dt, (size_t)N * 8, hipMemcpyHostToDevice, r->stream));
  CK(hipStreamSynchronize(r->stream));
  r->has_times = 1;
  return O3S_OK;
}

// the de-skew along a trajectory on the staged sweep, in place (trajectory_dev.h): points only, the staged normals stay as they are
int o3s_raw_scan_undistort_trajectory(o3s_raw_scan* r, const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew* params) {
  if (!r || !trajectory_call_valid(poses, K, params, r->N > 0 && r->has_times)) return O3S_ERR_BAD_ARGUMENT;
  if (r->N == 0 || K == 1) return O3S_OK;
  TrajectoryArgs a;
  std::vector<double> tab;
  int rc = trajectory_prepare(poses, K, *params, &a, &tab);
  if (rc != O3S_OK) return rc;
  if (hipSetDevice(r->device) != hipSuccess) return O3S_ERR_HIP;
  CK(r->traj.ensure(tab.size() * 8, 0, r->stream));
  CK(hipMemcpyAsync(r->traj.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, r->stream));
  rc = undistort_trajectory_dev(r->p.as<double>(), r->has_times ? r->dt.as<double>() : nullptr, r->N, r->traj.as<double>(), a, r->stream);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(r->stream));  // the pre-process reads the staged copy from another stream; `tab` is free again
  return O3S_OK;
}

int o3s_host_alloc_pinned(size_t bytes, void** out) {
  if (!out || bytes == 0) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  return hipHostMalloc(out, bytes, hipHostMallocPortable) == hipSuccess ? O3S_OK : O3S_ERR_HIP;
}

void o3s_host_free_pinned(void* p) {
  if (p) (void)hipHostFree(p);
}

int o3s_scan_create(int device, o3s_scan** out) {
  if (!out) return O3S_ERR_BAD_ARGUMENT;
  *out = nullptr;
  const int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  o3s_scan* sc = new o3s_scan();
  sc->device = device;
  if (hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&sc->handover, hipEventDisableTiming) != hipSuccess) {
    if (sc->stream) (void)hipStreamDestroy(sc->stream);
    delete sc;
    return O3S_ERR_HIP;
  }
  *out = sc;
  return O3S_OK;
}

void o3s_scan_destroy(o3s_scan* sc) {
  if (!sc) return;
  (void)hipSetDevice(sc->device);
  if (sc->stream) {
    (void)hipStreamSynchronize(sc->stream);
    (void)hipStreamDestroy(sc->stream);
  }
  if (sc->handover) (void)hipEventDestroy(sc->handover);
  delete sc;
}

int o3s_scan_set_normal_estimation(o3s_scan* sc, double max_radius, int32_t knn) {
  if (!sc) return O3S_ERR_BAD_ARGUMENT;
  if (knn <= 0) {
    sc->normal_knn = 0;
    return O3S_OK;
  }
  if (knn > kNnMax || !(max_radius > 0.0)) return O3S_ERR_BAD_ARGUMENT;
  sc->normal_radius = max_radius;
  sc->normal_knn = knn;
  return O3S_OK;
}

}  // extern "C"

// pts / normals: host arrays, or (on_device) arrays already in HBM on the scan's device
static int scan_preprocess_impl(o3s_scan* sc, const o3s_cropper* map_builder_cropper, double voxel_size, const o3s_cropper* scan_matcher_cropper,
                                const double* pts, const double* normals, int64_t N, int64_t* n_merge, int64_t* n_match, bool on_device) {
  if (n_merge) *n_merge = 0;
  if (n_match) *n_match = 0;
  if (!sc || !map_builder_cropper || !scan_matcher_cropper || N < 0 || (N > 0 && !pts)) return O3S_ERR_BAD_ARGUMENT;
  const bool estimate = normals == nullptr;
  if (N > 0 && estimate && sc->normal_knn <= 0) return O3S_ERR_BAD_SHAPE;  // no normals and no estimation parameters
  if (N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  sc->n_wide = sc->n_narrow = sc->n_raw = 0;
  sc->pm_ready = false;
  if (N == 0) return O3S_OK;
  if (hipSetDevice(sc->device) != hipSuccess) return O3S_ERR_HIP;
  hipStream_t s = sc->stream;
  CK(sc->raw_p.ensure((size_t)N * 24, 0, s));
  CK(sc->raw_n.ensure((size_t)N * 24, 0, s));
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  CK(hipMemcpyAsync(sc->raw_p.p, pts, (size_t)N * 24, kind, s));
  if (!estimate) CK(hipMemcpyAsync(sc->raw_n.p, normals, (size_t)N * 24, kind, s));
  for (DevMem* a : {&sc->tmp_p, &sc->tmp_n, &sc->wide_p, &sc->wide_n, &sc->narrow_p, &sc->narrow_n}) CK(a->ensure((size_t)N * 24, 0, s));
  int rc = O3S_OK;
  {  // bounded wide volume: crop, down-sample and narrow crop as one pipeline with a single read-back (cloud_dev.h, "hinted")
    double lo[3], hi[3];
    VoxHint vh;
    if (hints_enabled() && voxel_size > 0.0 && cropper_aabb(*map_builder_cropper, lo, hi) && vox_hint(1, lo, hi, voxel_size, &vh)) {
      int64_t cnt[3];
      bool ok = false;
      if (!estimate) {  // the narrow crop writes the reading for the ICP as well: no conversion pass in o3s_scan_set_reading
        CK(sc->xyzw.ensure((size_t)N * 16, 0, s));
        CK(sc->n32.ensure((size_t)N * 12, 0, s));
      }
      rc = voxel_pipeline_hint_dev(sc->arena, 1, map_builder_cropper, vh, voxel_size, sc->raw_p.as<double>(), estimate ? nullptr : sc->raw_n.as<double>(), N,
                                   sc->wide_p.as<double>(), sc->wide_n.as<double>(), nullptr, nullptr, estimate ? nullptr : scan_matcher_cropper, sc->narrow_p.as<double>(),
                                   sc->narrow_n.as<double>(), cnt, &ok, s, estimate ? nullptr : reinterpret_cast<float4*>(sc->xyzw.p),
                                   estimate ? nullptr : reinterpret_cast<float*>(sc->n32.p));
      if (rc != O3S_OK) return rc;
      if (ok) {
        int64_t n_wide = cnt[1], n_narrow = cnt[2];
        if (estimate) {
          if (n_wide > 0) {
            rc = estimate_normals_dev(sc->nwork, sc->wide_p.as<double>(), n_wide, sc->normal_radius, sc->normal_knn, sc->wide_n.as<double>(), nullptr, s);
            if (rc != O3S_OK) return rc;
          }
          rc = crop_dev(sc->arena, *scan_matcher_cropper, sc->wide_p.as<double>(), sc->wide_n.as<double>(), n_wide, sc->narrow_p.as<double>(), sc->narrow_n.as<double>(), &n_narrow, s);
          if (rc != O3S_OK) return rc;
        }
        CK(hipStreamSynchronize(s));
        sc->n_wide = n_wide;
        sc->n_narrow = n_narrow;
        sc->n_raw = N;
        sc->raw_has_normals = estimate ? 0 : 1;
        sc->voxel_ordered = true;
        sc->pm_ready = !estimate;
        if (n_merge) *n_merge = n_wide;
        if (n_match) *n_match = n_narrow;
        return O3S_OK;
      }
    }
  }
  // preprocess(): croppedCloud = mapBuilderCropper_->crop(in)
  int64_t n_crop = 0;
  rc = crop_dev(sc->arena, *map_builder_cropper, sc->raw_p.as<double>(), estimate ? nullptr : sc->raw_n.as<double>(), N, sc->tmp_p.as<double>(), sc->tmp_n.as<double>(), &n_crop, s);
  if (rc != O3S_OK) return rc;
  // o3d_slam::voxelize(voxelSize, croppedCloud): Open3D VoxelDownSample, or nothing for voxelSize <= 0
  int64_t n_wide = 0;
  if (voxel_size > 0.0 && n_crop > 0) {
    rc = voxel_pipeline_dev(sc->arena, 1, nullptr, voxel_size, sc->tmp_p.as<double>(), estimate ? nullptr : sc->tmp_n.as<double>(), n_crop, sc->wide_p.as<double>(), sc->wide_n.as<double>(),
                            nullptr, &n_wide, s);
    if (rc != O3S_OK) return rc;
  } else {
    n_wide = n_crop;
    if (n_crop) {
      CK(hipMemcpyAsync(sc->wide_p.p, sc->tmp_p.p, (size_t)n_crop * 24, hipMemcpyDeviceToDevice, s));
      if (!estimate) CK(hipMemcpyAsync(sc->wide_n.p, sc->tmp_n.p, (size_t)n_crop * 24, hipMemcpyDeviceToDevice, s));
    }
  }
  // cloudRegistration->estimateNormalsOrCovariancesIfNeeded(croppedCloud): only for clouds that came without normals
  if (estimate && n_wide > 0) {
    rc = estimate_normals_dev(sc->nwork, sc->wide_p.as<double>(), n_wide, sc->normal_radius, sc->normal_knn, sc->wide_n.as<double>(), nullptr, s);
    if (rc != O3S_OK) return rc;
  }
  // narrowCropped = scanMatcherCropper_->crop(*wideCropped)
  int64_t n_narrow = 0;
  rc = crop_dev(sc->arena, *scan_matcher_cropper, sc->wide_p.as<double>(), sc->wide_n.as<double>(), n_wide, sc->narrow_p.as<double>(), sc->narrow_n.as<double>(), &n_narrow, s);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(s));
  sc->n_wide = n_wide;
  sc->n_narrow = n_narrow;
  sc->n_raw = N;
  sc->raw_has_normals = estimate ? 0 : 1;
  sc->voxel_ordered = voxel_size > 0.0;
  sc->pm_ready = false;
  if (n_merge) *n_merge = n_wide;
  if (n_match) *n_match = n_narrow;
  return O3S_OK;
}

extern "C" {

int o3s_scan_preprocess(o3s_scan* sc, const o3s_cropper* map_builder_cropper, double voxel_size, const o3s_cropper* scan_matcher_cropper,
                        const double* pts, const double* normals, int64_t N, int64_t* n_merge, int64_t* n_match) {
  return scan_preprocess_impl(sc, map_builder_cropper, voxel_size, scan_matcher_cropper, pts, normals, N, n_merge, n_match, false);
}

int o3s_scan_preprocess_staged(o3s_scan* sc, const o3s_cropper* map_builder_cropper, double voxel_size, const o3s_cropper* scan_matcher_cropper,
                               const o3s_raw_scan* raw, int64_t* n_merge, int64_t* n_match) {
  if (!raw || !sc || raw->device != sc->device) return O3S_ERR_BAD_ARGUMENT;
  return scan_preprocess_impl(sc, map_builder_cropper, voxel_size, scan_matcher_cropper, raw->p.as<double>(), raw->has_normals ? raw->n.as<double>() : nullptr, raw->N,
                              n_merge, n_match, true);
}

int64_t o3s_scan_get(const o3s_scan* sc, int which, double* pts, double* normals) {
  if (!sc || (which != 0 && which != 1)) return -1;
  const int64_t n = which == 0 ? sc->n_wide : sc->n_narrow;
  if (!pts || n == 0) return n;
  if (hipSetDevice(sc->device) != hipSuccess) return -1;
  const DevMem& p = which == 0 ? sc->wide_p : sc->narrow_p;
  const DevMem& q = which == 0 ? sc->wide_n : sc->narrow_n;
  if (hipStreamSynchronize(sc->stream) != hipSuccess) return -1;
  if (hipMemcpy(pts, p.p, (size_t)n * 24, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (normals && hipMemcpy(normals, q.p, (size_t)n * 24, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}

// CloudRegistration::registerClouds between two resident pre-processed scans: nothing is downloaded; the work area's stream (the
// target's) is ordered behind the source's by an event, and the call returns on a drained stream, so either scan may be refilled
int o3s_scan_registration_icp(const o3s_scan* source, int source_which, const o3s_scan* target, int target_which, double max_dist,
                              const double init[16], const o3s_o3d_estimation* est, const o3s_o3d_icp_criteria* criteria,
                              o3s_o3d_icp_result* result) {
  if (!o3d_est_valid(est) || !source || !target || !init || !result || !(max_dist > 0.0) || (source_which != 0 && source_which != 1) ||
      (target_which != 0 && target_which != 1))
    return O3S_ERR_BAD_ARGUMENT;
  if (source->device != target->device) return O3S_ERR_BAD_ARGUMENT;
  const int64_t Ns = source_which == 0 ? source->n_wide : source->n_narrow;
  const int64_t Nt = target_which == 0 ? target->n_wide : target->n_narrow;
  if (Ns == 0 || Nt == 0) return O3S_ERR_EMPTY_REFERENCE;
  if (hipSetDevice(target->device) != hipSuccess) return O3S_ERR_HIP;
  const double* sp = (source_which == 0 ? source->wide_p : source->narrow_p).as<double>();
  const double* sn = (source_which == 0 ? source->wide_n : source->narrow_n).as<double>();
  const double* tp = (target_which == 0 ? target->wide_p : target->narrow_p).as<double>();
  const double* tn = (target_which == 0 ? target->wide_n : target->narrow_n).as<double>();
  hipStream_t s = target->stream;
  if (source->stream != s) {
    CK(hipEventRecord(source->handover, source->stream));
    CK(hipStreamWaitEvent(s, source->handover, 0));
  }
  O3dEstIn e;
  e.type = est->type;
  e.eps = est->gicp_epsilon;
  e.src_n = sn;
  o3s_cloud::RegLease area(target->device, s);
  return area.end(o3d_icp_run(area->reg, sp, Ns, tp, tn, Nt, max_dist, init, criteria, result, s, /*on_device=*/true, nullptr, &e));
}

int o3s_scan_set_reading(o3s_scan* sc, o3s_icp* icp) {
  if (!sc || !icp) return O3S_ERR_BAD_ARGUMENT;
  if (sc->n_narrow == 0) return O3S_ERR_EMPTY_READING;  // "narrow cropped size is zero" (ScanToMapRegistration.cpp:66)
  if (hipSetDevice(sc->device) != hipSuccess) return O3S_ERR_HIP;
  hipStream_t s = sc->stream;
  const int64_t n = sc->n_narrow;
  if (!sc->pm_ready) {
    CK(sc->xyzw.ensure((size_t)n * 16, 0, s));
    CK(sc->n32.ensure((size_t)n * 12, 0, s));
    hipLaunchKernelGGL(k_o3d_to_pm, dim3(nblk(n)), dim3(kB), 0, s, sc->narrow_p.as<double>(), sc->narrow_n.as<double>(), n, reinterpret_cast<float4*>(sc->xyzw.p),
                       reinterpret_cast<float*>(sc->n32.p));
    CK(hipGetLastError());
  }
  CK(hipEventRecord(sc->handover, s));  // the ICP handle's stream waits for the conversion on the device
  const int rc = o3s_icp_wait_event(icp, sc->handover);
  if (rc != O3S_OK) return rc;
  const int rc2 = o3s_icp_set_reading_dev(icp, sc->xyzw.p, sc->n32.p, n);
  if (rc2 != O3S_OK) return rc2;
  return o3s_icp_reading_is_spatially_sorted(icp, sc->voxel_ordered ? 1 : 0);  // voxel order is spatial order: no re-sort per compute
}

int o3s_submap_insert_processed(o3s_submap* m, const o3s_scan* sc, const double T_map_sensor[16]) {
  if (const int rs_ = submap_settle(m); rs_ != O3S_OK) return rs_;  // a pending insert is completed first
  if (!m || !sc || !T_map_sensor) return O3S_ERR_BAD_ARGUMENT;
  if (sc->n_wide == 0) return O3S_OK;
  if (m->device != sc->device) return O3S_ERR_BAD_ARGUMENT;
  if (m->has_normals == 0) return O3S_ERR_BAD_SHAPE;
  const int rc = set_dev(m);
  if (rc != O3S_OK) return rc;
  CK(hipStreamSynchronize(sc->stream));
  // the insert may come back with its completion pending (submap_settle): every later call on the submap completes it first.  The
  // scan object may be refilled as soon as this returns, so its stream is ordered behind the kernels that read it here.
  if (!m->scan_read) CK(hipEventCreateWithFlags(&m->scan_read, hipEventDisableTiming));
  const int ri = insert_dev(m, sc->wide_p.as<double>(), sc->wide_n.as<double>(), sc->n_wide, T_map_sensor, nullptr, /*lazy=*/true, m->scan_read);
  if (m->pend.active) CK(hipStreamWaitEvent(sc->stream, m->scan_read, 0));
  return ri;
}

int o3s_estimate_normals(int device, const double* pts, int64_t N, double radius, int32_t max_nn, double* out_normals, int32_t* out_nn_idx) {
  if (!pts || !out_normals || N < 0 || max_nn < 1 || max_nn > kNnMax || !(radius > 0.0)) return O3S_ERR_BAD_ARGUMENT;
  if (N == 0) return O3S_OK;
  int rc = pick_device(device);
  if (rc != O3S_OK) return rc;
  hipStream_t s = nullptr;
  DevMem d_p, d_n, d_i;
  NormalsWork w;
  CK(d_p.alloc((size_t)N * 24));
  CK(d_n.alloc((size_t)N * 24));
  if (out_nn_idx) CK(d_i.alloc((size_t)N * (size_t)max_nn * 4));
  CK(hipMemcpyAsync(d_p.p, pts, (size_t)N * 24, hipMemcpyHostToDevice, s));
  rc = estimate_normals_dev(w, d_p.as<double>(), N, radius, max_nn, d_n.as<double>(), out_nn_idx ? d_i.as<int32_t>() : nullptr, s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(out_normals, d_n.p, (size_t)N * 24, hipMemcpyDeviceToHost, s));
  if (out_nn_idx) CK(hipMemcpyAsync(out_nn_idx, d_i.p, (size_t)N * (size_t)max_nn * 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return O3S_OK;
}

}  // extern "C"
