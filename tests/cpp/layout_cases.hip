// Every work-area layout of csrc against the size its hand-written formula gave before the layouts existed.  The formulas below
// are that record: copied verbatim from the commit before, with the sizes rocPRIM reports (scan_temp_bytes, sort_temp_bytes,
// merge_temp_bytes) turned into arguments, as they are arguments of the layouts.  A capacity decides when the device stalls in
// hipFree / hipMalloc and is visible through *_device_bytes, so layout_bytes must give the same number for every input.
// Host functions only: the program includes the implementation the way the library does, has its own main, needs no GPU, and is
// built and run by tests/test_ownership_cpp.py; it exits 0 and prints "ok" when all hold.
#include "cloud_ops.hip"

#include <cstdio>

using o3s::measure;

static int failed = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      if (failed < 20) std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
      ++failed;                                                    \
    }                                                              \
  } while (0)

namespace was {  // the formulas of the commit before
size_t crop(int64_t N, size_t tb_scan) { return Arena::pad((size_t)N * 4) + Arena::pad((size_t)(N + 1) * 4) + Arena::pad(tb_scan) + 1024; }
size_t voxel(int64_t N, size_t tb_scan, size_t tb_sort) {
  const size_t n = (size_t)N;
  return Arena::pad(n * 4) + Arena::pad((n + 1) * 4)                 // flag, off
         + Arena::pad(n * 12) + Arena::pad(kExtSlots * 6 * 4) + Arena::pad(kBoundsWords * 8)  // vidx, mm, bounds block
         + 2 * Arena::pad(n * 8) + 2 * Arena::pad(n * 4)             // keys x2, vals x2
         + Arena::pad(n * 4) + Arena::pad((n + 1) * 4)               // head, ord
         + Arena::pad(std::max(tb_scan, tb_sort)) + 4096;
}
size_t insert_merge(int64_t n_tmp, int64_t n_v, int64_t n_s, size_t tb_scan, size_t tb_sort, size_t tb_merge) {
  const size_t nt = (size_t)n_tmp, nv = (size_t)std::max<int64_t>(n_v, 1), ns = (size_t)std::max<int64_t>(n_s, 1), nm = nv + ns;
  return Arena::pad(nt * 4) + Arena::pad((nt + 1) * 4) + Arena::pad(256)                      // flag, off, status
         + Arena::pad(nv * 8) + Arena::pad(nv * 4) + 2 * Arena::pad(ns * 8) + 2 * Arena::pad(ns * 4)  // A, U, U sorted
         + Arena::pad(nm * 8) + Arena::pad(nm * 4) + Arena::pad(nm * 4) + Arena::pad((nm + 1) * 4)   // merged keys / vals, head, ord
         + Arena::pad(std::max(std::max(tb_scan, tb_sort), tb_merge)) + 4096;
}
size_t carve(int64_t Nm, size_t tb_scan, size_t tb_sort) {
  const size_t nm = (size_t)Nm;
  return 3 * Arena::pad(nm * 4) + Arena::pad((nm + 1) * 4) + 2 * Arena::pad(nm * 8) + 2 * Arena::pad(nm * 4) + Arena::pad(kExtSlots * 6 * 4) +
         Arena::pad(std::max(tb_scan, tb_sort)) + 8192;
}
size_t overlap(int64_t Ns, int64_t Nt, uint32_t slots, size_t tb_scan) {
  const size_t ns = (size_t)Ns, nt = (size_t)Nt;
  return Arena::pad(ns * 8) + Arena::pad(nt * 8) + Arena::pad(ns * 4) + Arena::pad(nt * 4) + Arena::pad((ns + 1) * 4) + Arena::pad((nt + 1) * 4) +
         Arena::pad(tb_scan) + Arena::pad((size_t)slots * sizeof(OvSlot)) + Arena::pad(64) + Arena::pad(128) +
         Arena::pad(kBoundsReplicaWords * 8) + 4096;
}
size_t grid_index(int64_t N, size_t tb_scan, size_t tb_sort) {
  const size_t n = (size_t)N;
  return Arena::pad(kBoundsWords * 8) + 2 * Arena::pad(n * 8) + 2 * Arena::pad(n * 4) + Arena::pad(n * 4) + Arena::pad((n + 1) * 4) +
         Arena::pad(n * 24) + Arena::pad(std::max(tb_scan, tb_sort)) + 8192;
}
size_t assemble(int64_t N, size_t tb_scan, size_t tb_sort) {
  const size_t n = (size_t)N;
  return Arena::pad(kBoundsWords * 8)                              // bounds block
         + 2 * Arena::pad(n * 8) + 2 * Arena::pad(n * 4)           // keys x2, vals x2
         + Arena::pad(n * 4) + Arena::pad((n + 1) * 4)             // head, ord
         + Arena::pad(std::max(tb_scan, tb_sort)) + 4096;
}
size_t oc_chunk(int m, uint32_t slots, uint32_t n_buckets, uint32_t blocks_all, uint32_t blocks_src, int64_t G, int64_t Mt, size_t tb_sort) {
  return Arena::pad((size_t)m * sizeof(OcPair)) + Arena::pad((size_t)slots * sizeof(OvSlot)) + 2 * Arena::pad((size_t)G * 4) +
         Arena::pad((size_t)(3 * m + 1) * 4) + Arena::pad((size_t)blocks_all * 4) + 2 * Arena::pad((size_t)Mt * 8) + 2 * Arena::pad((size_t)Mt * 4) + Arena::pad(tb_sort) +
         Arena::pad((size_t)n_buckets * 8) + Arena::pad((size_t)Mt * sizeof(OcRec)) + Arena::pad((size_t)kOcComps * blocks_src * 8) +
         Arena::pad((size_t)m * kOcComps * 8) + 4096;
}
size_t sorted(size_t n, size_t tb, size_t extra_bytes) {  // the registration sort area (extra 0), and dm_sorted_keys
  return 2 * Arena::pad(n * 8) + 2 * Arena::pad(n * 4) + Arena::pad(tb) + extra_bytes + 4096;
}
size_t dm_carve_extra(size_t n, size_t cap, int64_t nwords) {
  return 2 * Arena::pad(n * 4) + Arena::pad((n + 1) * 4) + Arena::pad(cap) + Arena::pad((size_t)nwords * 16);
}
size_t dm_export(size_t cap, size_t v, size_t tb, bool colors) {
  return Arena::pad(cap * 4) + Arena::pad((cap + 1) * 4) + 2 * Arena::pad(v * 8) + 2 * Arena::pad(v * 4) + Arena::pad(tb) +
         (colors ? 3 : 2) * Arena::pad(v * 24) + Arena::pad(v * 12) + Arena::pad(v * 4) + 4096;
}
}  // namespace was

static const int64_t kCounts[] = {0, 1, 255, 256, 257, 65537, 3000001};  // 0 only where the pipeline admits it
static const size_t kTemps[] = {0, 1, 256, 257, 1000000};                // each branch of every max(...) is hit
constexpr int kNc = 7;

static void one_size() {
  for (int i = 0; i < kNc; ++i) {
    const int64_t N = kCounts[i];
    const size_t n = (size_t)N;
    for (size_t ta : kTemps) {
      if (N > 0) CHECK(layout_bytes<CropArea>(n, ta) == was::crop(N, ta));  // every crop returns before its work area for N = 0
      CHECK(layout_bytes<O3dSortArea>(n, ta) == was::sorted(n, ta, 0));     // o3s_registration_reserve(0, 0)
      if (N > 0) CHECK(layout_bytes<DmSortArea>(n, ta) == was::sorted(n, ta, 0));
      for (size_t tb : kTemps) {
        CHECK(layout_bytes<VoxelArea>(n, ta, tb) == was::voxel(N, ta, tb));  // o3s_submap_reserve(0)
        // the hinted voxelisers live in a reservation of the measuring one's size
        CHECK(measure<VoxelHintArea>(n, ta, tb) <= measure<VoxelArea>(n, ta, tb));
        CHECK(layout_bytes<GridIndexArea>(n, ta, tb) == was::grid_index(N, ta, tb));  // o3s_registration_reserve(0, 0)
        if (N > 0) CHECK(layout_bytes<CarveArea>(n, ta, tb) == was::carve(N, ta, tb));
        if (N > 0) CHECK(layout_bytes<AssembleArea>(n, ta, tb) == was::assemble(N, ta, tb));
      }
    }
  }
}

static void two_sizes() {
  for (int i = 0; i < kNc; ++i)
    for (int j = 0; j < kNc; ++j) {
      if (i == j) continue;  // unequal pairs
      const int64_t A = kCounts[i], B = kCounts[j];
      const size_t a = (size_t)A, b = (size_t)B;
      for (size_t ta : kTemps) {
        // overlap: source A, target B; the first table and the full one
        for (uint32_t slots : {std::min(kOvFirstSlots, ov_slots_for(A + B)), ov_slots_for(A + B)})
          CHECK(layout_bytes<OverlapArea>(a, b, (size_t)slots, ta) == was::overlap(A, B, slots, ta));
        // dense-map carving: A scan points into a table of B slots (a power of two >= 1024 in the map: any size here)
        if (A > 0)
          for (int64_t nwords : {(int64_t)4096, (int64_t)1 << 20})
            CHECK(layout_bytes<DmCarveArea>(a, ta, b, (size_t)nwords) == was::sorted(a, ta, was::dm_carve_extra(a, b, nwords)));
        // dense-map export: a table of A slots with B live voxels
        if (A > 0 && B > 0)
          for (bool colors : {false, true}) CHECK(layout_bytes<DmExportArea>(a, b, ta, colors) == was::dm_export(a, b, ta, colors));
        // insert by merge: A old voxel points, B scan points, and a few pass-through points in front (0 / 0: o3s_submap_reserve(0))
        for (size_t tb : kTemps)
          for (size_t tc : kTemps)
            for (int64_t n_pt : {(int64_t)0, (int64_t)77}) {
              const int64_t n_tmp = n_pt + A + B;
              CHECK(layout_bytes<InsertMergeArea>((size_t)n_tmp, a, b, ta, tb, tc) == was::insert_merge(n_tmp, A, B, ta, tb, tc));
            }
      }
    }
  CHECK(layout_bytes<InsertMergeArea>((size_t)0, (size_t)0, (size_t)0, (size_t)0, (size_t)0, (size_t)0) == was::insert_merge(0, 0, 0, 0, 0, 0));
}

static void constraint_chunks() {  // m pairs of unequal clouds, sized as oc_run_chunk sizes them
  for (int m : {1, 5})
    for (int first : {0, 1})  // the first table slices, then the full ones
      for (int i = 1; i < kNc; ++i)
        for (size_t ta : kTemps) {
          OcSizes L;
          for (int k = 0; k < m; ++k) {
            const int64_t ns = kCounts[i], nt = kCounts[1 + (i + k) % (kNc - 1)] + (k == 0 ? 3 : 0);
            const uint32_t full = ov_slots_for(ns + nt);
            L.slots += first ? std::min(kOvFirstSlots, full) : full;
            L.blocks_all += nblk(ns) + nblk(nt);
            L.blocks_src += nblk(ns);
            L.G += ns + nt;
            L.Mt += nt;
          }
          L.n_buckets = 1u << 10;
          while ((int64_t)L.n_buckets < L.Mt && L.n_buckets < (1u << 31)) L.n_buckets <<= 1;
          L.tb_sort = ta;
          CHECK(layout_bytes<OcArea>(m, L) == was::oc_chunk(m, L.slots, L.n_buckets, L.blocks_all, L.blocks_src, L.G, L.Mt, L.tb_sort));
        }
}

int main() {
  one_size();
  two_sizes();
  constraint_chunks();
  // the two reservations that name a layout from outside its pipeline
  CHECK(grid_index_arena_bytes(257) == was::grid_index(257, scan_temp_bytes(257), sort_temp_bytes(257)));
  CHECK(reg_overlap_arena_bytes(257, 65537) == was::overlap(257, 65537, ov_slots_for(257 + 65537), scan_temp_bytes(65537)));
  if (failed) {
    std::printf("%d checks failed\n", failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
