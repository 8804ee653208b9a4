// o3s_icp.hip — host side of libo3dslam_icp_hip.so (C ABI declared in include/o3s_icp.h).
//
// Build (gfx950 only, no other targets, no CPU fallback):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared -Iinclude o3s_icp.hip -o libo3dslam_icp_hip.so
#include "../../include/o3s_icp.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dev_mem.h"
#include "icp_kernels.h"
#include "icp_shard_kernels.h"
#include "icp_types.h"
#include "localizability_dev.h"
#include "degeneracy_dev.h"
#include "../../include/degeneracy/o3s_degeneracy.h"

#pragma clang fp contract(off)

using namespace o3s;

namespace {

thread_local std::string g_create_error;

struct HostStage {  // pinned staging block for small H2D / D2H transfers
  IcpState state;
  IcpState eval_state;  // o3s_icp_evaluate_resident's own: `state` keeps what the last compute left (o3s_icp_host_split reads it)
  float T0[16];
  double ref_part[1024 * 3];  // init_reference: per-block sums and bounds of k_ref_stats (a pageable landing area costs a
  float ref_bb[1024 * 6];     // staged round trip per copy)
  uint32_t n_occ;
};

constexpr int kNumKernels = 5;
constexpr size_t kCovBufBytes = ((size_t)kMaxPartialBlocks * kCovComps + kCovComps + 3) * sizeof(double);  // k_cov's partials [42][blocks], the 42 totals + 2 stamps, k_cov's start
static_assert(kCovBufBytes >= (2 * (size_t)kern::kFitMaxBlocks + 4) * sizeof(double), "k_fit's block partials and its four totals fit the covariance pass's area");
constexpr size_t kHistWords = (size_t)kHistReplicas * kHistBins + 1024;  // level-1 replicas + the level-2 histogram right behind them
// hooks build: per-iteration traces behind the speculative histograms — the depth k_classify resolved, then the matcher's two
// counters of settled queries (certificate held | the wave skipped its search) in kHistReplicas copies: one atomic per wave onto
// one word made the hooks build's converged launch 39 us
constexpr size_t kHookTraceWords = (1 + 2 * (size_t)kHistReplicas) * kSpecTrace;

// Lanes per open query of k_match2's settle front.  Four whatever the reading's size: the open queries' search is what the launch
// ends on, and four lanes take their candidates in one round (converged k_match2, hooks build, us: C2 without the front 8.58, two
// lanes 8.13, four 7.50;  C4 24.1, 18.4, 17.0: profiles/r10/NOTES.md)
constexpr int kFrontLanes = 4;

struct ChainArgs {
  int N;
  int match_g;  // lanes per query of k_match2
  int front_g;  // lanes per open query of k_match2's settle front (launches 2.. of a chain that keeps certificates); 0: no front
  int nb_match, nb_part, nb_cls;
  int nb_fused;  // blocks of the fused selection + normal-equation kernel (0: the two kernels are launched separately)
  bool has_n;
  uint32_t* spec;  // the speculative digit histograms and bin counters of the trim selection (k_match2 -> k_classify); null: level 1 only
  int no_bin_counters;  // hooks build (O3S_NO_BIN_COUNTERS=1): k_classify sums the level-1 replicas in every iteration
  float* cert;     // the matcher's certificates (k_match2 -> the next k_match2); null: every query is searched in every iteration
  float *rx, *ry, *rz, *rnx, *rny, *rnz;
  ChainParams cp;
  GridParams g;
};

// One compute() from compute_launch to compute_finish: the plan compute_launch builds once (what the chain computes, how its
// iterations go onto the stream, how many go out before each look at its post) and how far the call has got.
struct Call {
  bool live = false;  // compute_launch succeeded and compute_finish has not run yet
  ChainArgs a{};      // launch arguments; a.cp: the chain's parameters
  bool stats = false;
  float Tc[16], T0[16];  // T_refIn_refMean and the initial guess in the <refMean> frame
  int iters_cap = 0;     // max_iters, or 4096 without a Counter checker
  enum Issue { kEager, kReplay, kProfiled } issue = kEager;  // launch by launch, replays of the captured graph, launch by launch between events
  int first = 0, step = 0;  // iterations issued before the first look at the post, and before each later one
  int issued = 0;
  // the chain is certain to end inside what was issued: a Counter checker and all of max_iters out
  bool ends_inside() const { return a.cp.max_iters > 0 && issued >= a.cp.max_iters; }
};

}  // namespace

struct o3s_icp {
  o3s_icp_config cfg;
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::string err;
  // Every DevBuf of the handle but d_loc (which has loc_gen, below) reports its moves here; the graph key carries the value, so a
  // graph is never replayed after ANY buffer a captured kernel points at has moved (the key's pointer list alone missed d_cand & co.).
  uint64_t alloc_gen = 0;

  // reference (matcher index)
  bool ref_ready = false;
  bool ref_has_normals = false;
  int64_t M = 0;
  float mean[3] = {0, 0, 0};
  GridParams grid{};
  size_t ncells = 0;
  int qf = 1, qnx = 1, qny = 1, qnz = 1;  // coarsened grid the reading is sorted on
  size_t qcells = 1;
  DevBuf d_ref_in{&alloc_gen}, d_refn_in{&alloc_gen};  // staging for host-supplied references
  DevBuf d_ref{&alloc_gen}, d_refn{&alloc_gen}, d_cell_start{&alloc_gen}, d_cell_tmp{&alloc_gen}, d_qstart{&alloc_gen}, d_orig_to_sorted{&alloc_gen},
      d_cell_of{&alloc_gen}, d_scan_sums{&alloc_gen}, d_ref_part{&alloc_gen}, d_ref_bb{&alloc_gen};
  // the first-iteration index (dense maps only, init_reference_impl step 4): the same points sorted on a grid of 1.5 x the cell edge
  bool have_grid1 = false;
  GridParams grid1{};
  DevBuf d_ref1{&alloc_gen}, d_refn1{&alloc_gen}, d_cell_start1{&alloc_gen};
  bool far_rows = false;  // the matcher's far search is the row-disc search (finite maxDist), else the ring search

  // reading
  bool reading_ready = false;
  bool read_has_normals = false;
  bool reading_presorted = false;  // o3s_icp_reading_is_spatially_sorted: the per-call counting sort of the reading is skipped
  int N = 0;
  int prepared_N = 0;  // points of the last prepare_reading (d_perm holds their processing order)
  const void* ext_xyzw = nullptr;  // device pointers supplied by set_reading_dev (not owned)
  const void* ext_n = nullptr;
  DevBuf d_in_xyzw{&alloc_gen}, d_in_n{&alloc_gen}, d_t{&alloc_gen}, d_r{&alloc_gen}, d_perm{&alloc_gen}, d_qcell{&alloc_gen};
  DevBuf d_qcount{&alloc_gen};  // per-bin counts of the reading's sort [qcells] + tile totals behind them: ALL ZEROS between calls
  size_t qcount_words = 0;

  // iteration chain
  DevBuf d_mn{&alloc_gen};  // matched reference normal of every query (written by k_classify, streamed by k_normal_eq)
  DevBuf d_mq{&alloc_gen};  // matched reference point of every query (k_match2: this iteration's output, the next one's pruning bound)
  DevBuf d_cert{&alloc_gen};  // ... and its certificate: a lower bound of the squared distance to every OTHER reference point (0: none)
  DevBuf d_cand_cnt{&alloc_gen};
  DevBuf d_sel_part2{&alloc_gen}, d_park{&alloc_gen};  // k_sel_partial (large readings): block partials [7][blocks]; parked records [kParkRecs] + their order keys
  DevBuf d_pos{&alloc_gen}, d_d2{&alloc_gen}, d_hist{&alloc_gen}, d_cand{&alloc_gen}, d_sel{&alloc_gen}, d_cent{&alloc_gen}, d_ne{&alloc_gen},
      d_state{&alloc_gen}, d_T0{&alloc_gen}, d_trace_T{&alloc_gen}, d_trace_limit{&alloc_gen}, d_trace_kept{&alloc_gen};
  DevBuf d_mod_a{&alloc_gen}, d_mod_b{&alloc_gen}, d_mod_c{&alloc_gen}, d_mod_d{&alloc_gen};  // module-level scratch
  // pose covariance (error_minimizer 1, o3s_icp_estimate_covariance): k_cov's block partials [42][blocks] with the 42 totals behind
  // them, and the mailbox k_cov_post posts the totals to
  DevBuf d_cov{&alloc_gen};
  host_post::PostBlock<> cov_mb;
  double cov[36] = {0};
  bool cov_valid = false;       // the last compute succeeded: o3s_icp_get_covariance has something to return
  bool elements_valid = false;  // ... and nothing has touched the chain's buffers since: o3s_icp_get_error_elements can rebuild its pairs
  float last_max_out_r2 = 0.f;  // the kept-pair predicate's MaxDist bound of that compute
  float last_step[16] = {0};    // ... and its last iteration's step (IcpState::dT)
  unsigned long long cov_t_start = 0, cov_t_end = 0;  // wall_clock64 stamps of the last covariance pass (k_cov's start, k_cov_post's end)
  // localizability analysis (localizability_impl.h): the work area of its four kernels, allocated by the first call or when the
  // degeneracy mode ANALYSE is set.  Only that mode's captured kernels point into it, so its moves are counted apart and the graph
  // key carries the count in that mode alone: a first analysis behind an unconstrained compute leaves the chain's graph alone
  uint64_t loc_gen = 0;
  DevBuf d_loc{&loc_gen};
  // degeneracy-aware step (degeneracy_impl.h): the mode of the later computes; the device area (the set the last constrained
  // iteration used, then one mask per iteration) exists only once a mode other than OFF has been set
  o3s_degeneracy_config deg{};          // (mode 0 = OFF)
  kern::DegFixed deg_fixed{};           // FIXED: the caller's set as k_constrain takes it
  uint64_t deg_gen = 0;                 // moves with every change of mode, set or parameters: part of the graph key
  bool deg_trace_valid = false;         // the last successful compute ran with a mode other than OFF
  DevBuf d_deg{&alloc_gen};
  // values for the partially localizable directions (degeneracy_partial_impl.h): the flag of the later computes; the device area
  // (the strong-pair partials, the last record, one trace record per iteration) exists only once the flag has been set
  bool deg_partial = false;
  bool deg_partial_valid = false;       // the last successful compute ran in ANALYSE mode with the flag set
  DevBuf d_degp{&alloc_gen};
  // registration fitness (o3s_icp_evaluate_resident): where the last successful compute left the reading.  pose_valid: that compute's
  // T_iter is in last_T_iter and nothing has replaced the reading or the reference since; r_is_call: d_r still holds the reading as
  // that compute prepared it (T0 . p in its processing order) — an evaluation at an explicit pose prepares it anew
  bool pose_valid = false, r_is_call = false;
  float last_T_iter[16] = {0};
  HostStage* stage = nullptr;                // pinned
  // mailbox (host_post.h): init_reference's two read-backs without a copy or a stream synchronisation
  host_post::PostBlock<> mb;
  // the chain's own mailbox (icp_types.h, HostPost): the kernel that closes an iteration posts the progress word and, when the
  // chain is done, the whole state — compute() polls it; no copy command, no stream synchronisation on the per-call path
  host_post::PostBlock<HostPost> post;
  uint32_t call_seq = 0;     // sequence number of the compute() in flight (k_read_prep writes it into the state)
  double wall_clock_khz = 100000.0;  // wall_clock64 rate (hipDeviceAttributeWallClockRate)
  // host-side split of the last compute(): microseconds spent issuing (either half) and waiting (wait_post), stream queries made
  double host_issue_us = 0.0, host_wait_us = 0.0;
  int host_queries = 0;
  // what ended the waits of the last compute(): the chain's post, the `drained` event, the 2 ms stream guard; and how the chain was
  // issued (0 eager, 1 captured in this call and replayed, 2 replayed from the cached graph) — o3s_icp_host_split_ex
  int wait_by_post = 0, wait_by_event = 0, wait_by_guard = 0, issue_mode = 0;
  // set by o3s_icp_compute_batch while several chains share the GPU: the fused k_sel_ne trades redundant work and most of a
  // CU's LDS for one chain's latency, which costs throughput when the CUs are wanted by other chains (64 pairs of config 3:
  // 9.7 ms with the two kernels apart, 10.8 ms fused)
  bool many_in_flight = false;
  int trace_cap = 0;
  int last_iters = 0;

  Call call;  // the compute() in flight between compute_launch and compute_finish
#ifdef O3S_TEST_HOOKS
  std::vector<int> looks;  // hooks build (O3S_PRINT_CHAIN): iterations issued at each look at the post of the call in flight
#endif

  // graph cache
  hipGraphExec_t graph_exec = nullptr;
  struct GraphKey {
    int N = -1, iters = -1, nb = -1, has_n = -1;
    uint64_t gen = 0;
    uint64_t deg = 0;  // 0: the degeneracy mode is OFF; else deg_gen
    uint64_t loc = 0;  // mode ANALYSE: loc_gen (the captured analysis kernels point into d_loc); else 0
    const void* ptrs[8] = {nullptr};
    ChainParams cp{};
    GridParams g{};
    bool have_grid1 = false;  // a captured iteration 0 bakes the first-iteration grid in by value (chain_index)
    GridParams g1{};
  } graph_key, graph_candidate;
  bool graph_candidate_valid = false;

  // one-pair-sharded mode (o3s_icp_shard_configure): this handle holds one slice of the reading
  struct Shard {
    bool active = false;
    int rank = 0, world = 1;
    int64_t n_total = 0;
    o3s_allreduce_fn fn = nullptr;
    void* user = nullptr;
    bool capturable = false;  // fn only enqueues stream work (ncclAllReduce): the sharded chain may be captured in a hipGraph
    uint8_t* xbuf = nullptr;  // exchange buffer (kXchgBytes), caller's or `own`
    DevBuf own;
    explicit Shard(uint64_t* gen) : own(gen) {}
  } shard{&alloc_gen};

  int eager_hint = 4;  // iterations the last call needed: where the eager (un-graphed) chain first looks at the `done` flag

  // profiling
  bool profiling = false;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  std::vector<hipEvent_t> prof_events;
  float kernel_ms[kNumKernels] = {0, 0, 0, 0, 0};
  int kernel_launches[kNumKernels] = {0, 0, 0, 0, 0};
};

namespace {

#define HIP_TRY(h, expr)                                                                      \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                           \
      return O3S_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

int fail(o3s_icp* h, int code, const char* msg) {
  h->err = msg;
  return code;
}

inline int nblocks(int64_t n, int per = kern::kBlock) { return (int)((n + per - 1) / per); }
inline int round_up8(int v) { return (v + 7) & ~7; }

// ---- fp32 4x4 helpers on the host (frame algebra of LPM/ICP.cpp:373-374, 462-465) ----------------------------
#define HM4(m, r, c) (m)[(c)*4 + (r)]
void hmul4(const float* A, const float* B, float* C) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      float s = HM4(A, r, 0) * HM4(B, 0, c);
      s = s + HM4(A, r, 1) * HM4(B, 1, c);
      s = s + HM4(A, r, 2) * HM4(B, 2, c);
      s = s + HM4(A, r, 3) * HM4(B, 3, c);
      HM4(C, r, c) = s;
    }
}
void hidentity(float* T) {
  for (int i = 0; i < 16; ++i) T[i] = 0.f;
  T[0] = T[5] = T[10] = T[15] = 1.f;
}
bool hrigid(const float* T) {  // RigidTransformation::checkParameters (LPM/TransformationsImpl.cpp:98-113)
  const float d0 = HM4(T, 0, 0) * (HM4(T, 1, 1) * HM4(T, 2, 2) - HM4(T, 1, 2) * HM4(T, 2, 1));
  const float d1 = HM4(T, 0, 1) * (HM4(T, 1, 0) * HM4(T, 2, 2) - HM4(T, 1, 2) * HM4(T, 2, 0));
  const float d2 = HM4(T, 0, 2) * (HM4(T, 1, 0) * HM4(T, 2, 1) - HM4(T, 1, 1) * HM4(T, 2, 0));
  const float det = d0 - d1 + d2;
  return !(std::fabs(1.f - det) > 0.001f);
}

ChainParams make_chain(const o3s_icp* h, bool reading_normals) {
  const o3s_icp_config& c = h->cfg;
  ChainParams cp{};
  cp.has_trim = c.trim_ratio >= 0.f;
  cp.trim_ratio = c.trim_ratio;
  cp.has_normal_gate = (c.max_normal_angle >= 0.f) && reading_normals && h->ref_has_normals;
  cp.cos_max_angle = std::cos(c.max_normal_angle);  // fp32 cos, as eps(cos(maxAngle)) at LPM/OutlierFiltersImpl.cpp:229
  cp.max_out_r2 = c.max_dist_outlier >= 0.f ? (float)std::pow((double)c.max_dist_outlier, 2)
                                            : std::numeric_limits<float>::infinity();
  cp.use_differential = c.use_differential;
  cp.min_diff_rot = c.min_diff_rot;
  cp.min_diff_trans = c.min_diff_trans;
  cp.smooth_length = c.smooth_length;
  cp.max_iters = c.max_iters;
  cp.counter_first = c.counter_first;
  cp.mirror = c.matcher == 1;
#ifdef O3S_TEST_HOOKS
  if (const char* e = O3S_HOOK_ENV("O3S_DBG")) cp.dbg = std::atoi(e);
#endif
  return cp;
}

int validate_config(const o3s_icp_config& c, std::string& why) {
  if (c.matcher != 0 && c.matcher != 1) return why = "matcher must be 0 (KDTreeMatcher) or 1 (MirrorMatcher)", O3S_ERR_BAD_CONFIG;
  if (!(c.max_dist > 0.f)) return why = "max_dist must be > 0", O3S_ERR_BAD_CONFIG;
  if (c.trim_ratio > 1.0f) return why = "trim_ratio must be <= 1", O3S_ERR_BAD_CONFIG;
  if (c.use_differential && (c.smooth_length < 0 || c.smooth_length > kMaxSmooth))
    return why = "smooth_length must be in [0, 15]", O3S_ERR_BAD_CONFIG;
  if (c.max_iters <= 0 && !c.use_differential) return why = "no transformation checker configured", O3S_ERR_BAD_CONFIG;
  if (c.grid_cell < 0.f) return why = "grid_cell must be >= 0", O3S_ERR_BAD_CONFIG;
  if (c.error_minimizer != 0 && c.error_minimizer != 1)
    return why = "error_minimizer must be 0 (PointToPlaneErrorMinimizer) or 1 (PointToPlaneWithCovErrorMinimizer)", O3S_ERR_BAD_CONFIG;
  if (c.error_minimizer == 1 && !(c.sensor_std_dev >= 0.f)) return why = "sensor_std_dev must be >= 0", O3S_ERR_BAD_CONFIG;
  return O3S_OK;
}

// exclusive scan of n uint32 counts into out[n+1] on the handle's stream
// zero_in: the input array is cleared once read (it becomes the per-cell cursor array of the scatter that follows).
// post_nonzero: the number of non-zero inputs is posted to the mailbox; *seq_out is the sequence number to wait for.
int device_scan(o3s_icp* h, uint32_t* in, int64_t n, uint32_t* out, bool zero_in = false, bool post_nonzero = false, uint32_t* seq_out = nullptr) {
  const int64_t nb = (n + kern::kScanTile - 1) / kern::kScanTile;
  HIP_TRY(h, h->d_scan_sums.ensure((size_t)nb * 8));
  uint32_t* sums = h->d_scan_sums.as<uint32_t>();
  uint32_t* nonzero = post_nonzero ? sums + nb : nullptr;
  uint32_t seq = 0;
  if (post_nonzero) {
    seq = h->mb.next();
    if (seq_out) *seq_out = seq;
  }
  hipLaunchKernelGGL(kern::k_scan_block_sums, dim3((unsigned)nb), dim3(kern::kBlock), 0, h->stream, in, n, sums, nonzero);
  hipLaunchKernelGGL(kern::k_scan_sums, dim3(1), dim3(1024), 0, h->stream, sums, nb, nonzero, h->mb.dev, seq);
  hipLaunchKernelGGL(kern::k_scan_apply, dim3((unsigned)nb), dim3(kern::kBlock), 0, h->stream, in, n, sums, out, zero_in ? in : nullptr);
  HIP_TRY(h, hipGetLastError());
  return O3S_OK;
}

// `drained` (nullable): an event recorded behind the last launch issued so far — how the host learns that everything issued has
// run WITHOUT ending the chain (kernels post once, when the chain is done).  Chains that are certain to end inside what was
// issued (a Counter checker and all of max_iters issued) pass none.  1 = the post is there (*done) or everything issued has run,
// 0 = the stream drained without the post and there was no event, < 0 = a HIP error.
int wait_post(o3s_icp* h, uint32_t seq, hipEvent_t drained, bool* done) {
#ifdef O3S_TEST_HOOKS
  if (h->looks.empty() || h->looks.back() != h->call.issued) h->looks.push_back(h->call.issued);
#endif
  const double t0 = host_post::now_us();
  host_post::PollTrace tr;
  const int w = host_post::poll_until(
      [&] {  // the final post of THIS call
        const unsigned long long word = __atomic_load_n(&h->post.host->word, __ATOMIC_ACQUIRE);
        return (uint32_t)(word >> 32) == seq && (word & 1ull);
      },
      h->stream, host_post::kChainCadence, drained, &tr);
  h->host_wait_us += host_post::now_us() - t0;
  h->host_queries += tr.queries;
  *done = w == host_post::kPollPosted;
  if (w == host_post::kPollError) return -1;
  (tr.tier == host_post::kTierSpin ? h->wait_by_post : tr.tier == host_post::kTierEvent ? h->wait_by_event : h->wait_by_guard) += 1;
  return *done || drained ? 1 : 0;
}

// ---- initReference on device-resident input --------------------------------------------------------------------
// center = false: Matcher::init semantics (LPM/MatchersImpl.cpp:108-114) — the cloud is indexed as given; x - 0.0f is exact,
// so the index kernels run unchanged with a zero mean
// d_count (nullable): the number of points is a word on the device (o3s_icp_init_reference_dev_counted_async): M is then an upper
// bound that sizes the statistics launch, and the count arrives with the statistics — one hand-over for both; *M_out receives it
int init_reference_impl(o3s_icp* h, const float4* d_xyzw, const float* d_normals, int64_t M, bool wait_end = true, bool center = true,
                        const uint32_t* d_count = nullptr, int64_t* M_out = nullptr) {
  h->ref_ready = false;
  // what a compute left speaks of the reference this call replaces: the reading in d_r and T_iter are centred on ITS mean, the
  // incumbents in d_mq are ITS points (no bound of anything in the new index)
  h->elements_valid = h->pose_valid = h->r_is_call = false;
  if (M_out) *M_out = 0;
  if (M <= 0) return fail(h, O3S_ERR_EMPTY_REFERENCE, "reference cloud is empty");
  if (M > (int64_t)0x7fffffff) return fail(h, O3S_ERR_BAD_ARGUMENT, "reference larger than 2^31-1 points");
  HIP_TRY(h, hipSetDevice(h->device));
  // 1. mean (fp64 accumulate, rounded once: rowwise().mean() at LPM/ICP.cpp:313) and bounds: per-block partials, folded
  //    by one block that posts the nine numbers to the mailbox
  const int G = std::min(1024, nblocks(M));
  HIP_TRY(h, h->d_ref_part.ensure((size_t)G * 3 * sizeof(double)));
  HIP_TRY(h, h->d_ref_bb.ensure((size_t)G * 6 * sizeof(float)));
  hipLaunchKernelGGL(kern::k_ref_stats, dim3(G), dim3(kern::kBlock), 0, h->stream, d_xyzw, M, d_count, h->d_ref_part.as<double>(),
                     h->d_ref_bb.as<float>());
  const uint32_t stats_seq = h->mb.next();
  hipLaunchKernelGGL(kern::k_ref_stats_post, dim3(1), dim3(kern::kBlock), 0, h->stream, h->d_ref_part.as<double>(), h->d_ref_bb.as<float>(), G, M,
                     d_count, h->mb.dev, stats_seq);
  HIP_TRY(h, hipGetLastError());
  {
    const int w = host_post::mailbox_wait(h->mb.host, stats_seq, h->stream);
    if (w < 0) return fail(h, O3S_ERR_HIP, "init_reference: the statistics kernels failed");
    if (w == 0) return fail(h, O3S_ERR_HIP, "init_reference: the statistics were not posted");
  }
  if (d_count) {  // the count the device formed
    M = (int64_t)host_post::post_get(h->mb.host, kern::RefStatsPost::kCount);
    if (M_out) *M_out = M;
    if (M <= 0) return fail(h, O3S_ERR_EMPTY_REFERENCE, "reference cloud is empty");
  }
  float lo[3], hi[3];
  for (int c = 0; c < 3; ++c) {
    h->mean[c] = host_post::post_get<float>(h->mb.host, kern::RefStatsPost::kMean + c);
    lo[c] = host_post::post_get<float>(h->mb.host, kern::RefStatsPost::kLo + c);
    hi[c] = host_post::post_get<float>(h->mb.host, kern::RefStatsPost::kHi + c);
    if (!center) h->mean[c] = 0.f;
  }
  for (int c = 0; c < 3; ++c) {
    lo[c] = lo[c] - h->mean[c];  // x - mean is monotone in x, so the centred bounds are the bounds of the centred cloud
    hi[c] = hi[c] - h->mean[c];
    if (!(std::isfinite(lo[c]) && std::isfinite(hi[c]))) return fail(h, O3S_ERR_BAD_ARGUMENT, "reference contains non-finite coordinates");
  }
  // 2. grid geometry.  Start from maxDist/3 (the 3x3x3 block then covers maxDist/3 around any query and rings 2-3 the
  //    rest up to maxDist; measured on C2: k_match 18.9 us vs 23.0 us at maxDist/2, 28.2 us at 0.6 maxDist); if the map
  //    is much denser than that (mean points per occupied cell > 8) shrink the cell so that it holds ~4 points — the
  //    ring expansion keeps the search exact for any cell size.  A user-supplied grid_cell is taken as is.
  const float ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
  float cell = h->cfg.grid_cell;
  const bool adaptive = !(cell > 0.f);
  if (adaptive) {
    if (std::isfinite(h->cfg.max_dist)) {
      cell = h->cfg.max_dist * (1.0f / 3.0f);
    } else {
      const double vol = std::max((double)ext[0], 1e-3) * std::max((double)ext[1], 1e-3) * std::max((double)ext[2], 1e-3);
      cell = (float)(2.0 * std::cbrt(vol / (double)M));
    }
  }
  const float maxext = std::max(ext[0], std::max(ext[1], ext[2]));
  const float min_cell = std::max(maxext * 1e-6f, 1e-6f);
  cell = std::max(cell, min_cell);
  const double kMaxCells = (double)(1u << 28);
  float maxabs = 0.f;
  for (int c = 0; c < 3; ++c) maxabs = std::max(maxabs, std::max(std::fabs(lo[c]), std::fabs(hi[c])));
  HIP_TRY(h, h->d_cell_of.ensure((size_t)M * 4));
  HIP_TRY(h, h->d_ref.ensure((size_t)M * sizeof(float4)));
  HIP_TRY(h, h->d_refn.ensure((size_t)M * sizeof(float4)));
  HIP_TRY(h, h->d_orig_to_sorted.ensure((size_t)M * 4));
  const int gb = nblocks(M);
  GridParams g{};
  int64_t dims[3];
  // grid geometry for a cell edge (enlarged until the grid has at most 2^28 cells); returns the number of cells
  auto geometry = [&](float& edge, GridParams& gp, int64_t d[3]) -> size_t {
    for (;;) {
      double total = 1;
      for (int c = 0; c < 3; ++c) {
        d[c] = (int64_t)std::floor((double)ext[c] / (double)edge) + 1;
        total *= (double)d[c];
      }
      if (total <= kMaxCells) break;
      edge *= 1.26f;
    }
    gp.ox = lo[0];
    gp.oy = lo[1];
    gp.oz = lo[2];
    gp.cell = edge;
    gp.inv_cell = 1.0f / edge;
    gp.nx = (int)d[0];
    gp.ny = (int)d[1];
    gp.nz = (int)d[2];
    gp.margin = std::max(edge * 1e-3f, 16.f * maxabs * 1.1920929e-7f);
    gp.max_r2 = h->cfg.max_dist * h->cfg.max_dist;  // libnabo: maxRadius2 = maxRadius * maxRadius
    return (size_t)d[0] * (size_t)d[1] * (size_t)d[2];
  };
  for (int attempt = 0;; ++attempt) {
    h->ncells = geometry(cell, g, dims);
    // 3. counting sort of the reference into cell order: per-cell populations, scan (which also counts the occupied
    //    cells and clears the populations: they become the scatter's cursors), scatter.  The density probe is
    //    speculative: the sort is enqueued for this cell size right away and only repeated, with a smaller cell, when
    //    the occupied-cell count — posted by the scan, long there by the time it is looked at — says the map is dense.
    HIP_TRY(h, h->d_cell_tmp.ensure(h->ncells * 4));
    HIP_TRY(h, h->d_cell_start.ensure((h->ncells + 1 + 4) * 4));  // +4: headers are fetched as 4-word groups
    HIP_TRY(h, hipMemsetAsync(h->d_cell_tmp.p, 0, h->ncells * 4, h->stream));
    hipLaunchKernelGGL(kern::k_ref_assign, dim3(gb), dim3(kern::kBlock), 0, h->stream, d_xyzw, M, h->mean[0], h->mean[1], h->mean[2], g,
                       h->d_cell_of.as<uint32_t>(), h->d_cell_tmp.as<uint32_t>());
    HIP_TRY(h, hipGetLastError());
    const bool probe = adaptive && attempt < 2;
    uint32_t seq = 0;
    int rc = device_scan(h, h->d_cell_tmp.as<uint32_t>(), (int64_t)h->ncells, h->d_cell_start.as<uint32_t>(), /*zero_in=*/true, probe, &seq);
    if (rc != O3S_OK) return rc;
    hipLaunchKernelGGL(kern::k_ref_scatter, dim3(gb), dim3(kern::kBlock), 0, h->stream, d_xyzw, d_normals, M, h->mean[0], h->mean[1], h->mean[2],
                       h->d_cell_of.as<uint32_t>(), h->d_cell_start.as<uint32_t>(), h->d_cell_tmp.as<uint32_t>(), h->d_ref.as<float4>(),
                       h->d_refn.as<float4>(), h->d_orig_to_sorted.as<int32_t>());
    HIP_TRY(h, hipGetLastError());
    if (!probe) break;
    const int w = host_post::mailbox_wait(h->mb.host, seq, h->stream);
    if (w < 0) return fail(h, O3S_ERR_HIP, "init_reference: the index kernels failed");
    if (w == 0) return fail(h, O3S_ERR_HIP, "init_reference: the occupied-cell count was not posted");
    const uint32_t n_occ = host_post::post_get(h->mb.host, host_post::kPostCount);
    const double rho = (double)M / (double)std::max(1u, n_occ);
    if (rho <= 8.0) break;
    const float next = std::max(min_cell, cell * (float)std::sqrt(4.0 / rho));  // points per cell ~ cell^2 on surfaces
    if (next > 0.9f * cell) break;
    cell = next;
  }
  h->grid = g;
  // 4. dense maps only: a second index of the same points for the FIRST iteration of a call.  The cell above was shrunk to ~4 points
  //    per occupied cell, which is what a converged iteration wants (few candidates; the incumbent bounds the search to a cell or two).
  //    A first iteration has no incumbents: under the initial guess the neighbour is several such cells away and the far search has
  //    to verify every row of the (y, z) disc of that radius — at C4 (cell 0.0445 m) 52 row windows per query, 0.93 ms.  How far away
  //    the neighbour is depends on the misalignment, not on the density, so the edge that suits this search is an absolute one:
  //    maxDist / 6 — the largest that still has the seed probe along the normal on (k_match2: reach >= 5 cells) — measured best or
  //    near best on maps of 0.02 and 0.03 m voxels (0.93 -> 0.64 .. 0.70 ms, 0.37 -> 0.30 ms), while every edge beyond maxDist / 5
  //    LOSES against the fine grid (tools/r05_first_grid.py, profiles/LAB_NOTES_r05.md 6).  Built when the main cell is at most 0.85
  //    of it.  Results do not depend on the grid (exact search, ties by original index).  Costs a second counting sort in
  //    init_reference and 32 bytes per reference point; maps at the nominal cell (maxDist / 3: C2, the per-scan loop) do not build it.
  h->have_grid1 = false;
  {
    const char* fg = O3S_HOOK_ENV("O3S_FIRST_GRID");  // hooks build: 0 = off, else the cell edge in metres
    const float nominal = std::isfinite(h->cfg.max_dist) ? h->cfg.max_dist * (1.0f / 3.0f) : 0.f;
    const float want = fg ? (float)std::atof(fg) : 0.5f * nominal;
    if (adaptive && nominal > 0.f && want > 0.f && g.cell <= 0.85f * want) {
      float cell1 = std::min(want, nominal);
      GridParams g1{};
      int64_t d1[3];
      const size_t nc1 = geometry(cell1, g1, d1);
      HIP_TRY(h, h->d_ref1.ensure((size_t)M * sizeof(float4)));
      if (d_normals) HIP_TRY(h, h->d_refn1.ensure((size_t)M * sizeof(float4)));
      HIP_TRY(h, h->d_cell_tmp.ensure(nc1 * 4));
      HIP_TRY(h, h->d_cell_start1.ensure((nc1 + 1 + 4) * 4));
      HIP_TRY(h, hipMemsetAsync(h->d_cell_tmp.p, 0, nc1 * 4, h->stream));
      hipLaunchKernelGGL(kern::k_ref_assign, dim3(gb), dim3(kern::kBlock), 0, h->stream, d_xyzw, M, h->mean[0], h->mean[1], h->mean[2], g1,
                         h->d_cell_of.as<uint32_t>(), h->d_cell_tmp.as<uint32_t>());
      HIP_TRY(h, hipGetLastError());
      const int rc1 = device_scan(h, h->d_cell_tmp.as<uint32_t>(), (int64_t)nc1, h->d_cell_start1.as<uint32_t>(), /*zero_in=*/true);
      if (rc1 != O3S_OK) return rc1;
      hipLaunchKernelGGL(kern::k_ref_scatter, dim3(gb), dim3(kern::kBlock), 0, h->stream, d_xyzw, d_normals, M, h->mean[0], h->mean[1], h->mean[2],
                         h->d_cell_of.as<uint32_t>(), h->d_cell_start1.as<uint32_t>(), h->d_cell_tmp.as<uint32_t>(), h->d_ref1.as<float4>(),
                         h->d_refn1.as<float4>(), (int32_t*)nullptr);
      HIP_TRY(h, hipGetLastError());
      h->grid1 = g1;
      h->have_grid1 = true;
    }
  }
  if (O3S_HOOK_ENV("O3S_PRINT_GRID"))  // hooks build: the cell edges the two indexes ended up with (tools/r05_first_grid.py)
    std::fprintf(stderr, "o3s grid: M %lld cell %.4f (%d x %d x %d) first-iteration cell %.4f\n", (long long)M, (double)g.cell, g.nx, g.ny, g.nz,
                 h->have_grid1 ? (double)h->grid1.cell : 0.0);
  {
    // the row-disc far search needs a finite bound to end; an unbounded maxDist (or one that reaches across more cells than an
    // int comfortably indexes) keeps the ring search, which expands until something is found.
    const double reach = std::isfinite(h->cfg.max_dist) ? (double)h->cfg.max_dist / (double)g.cell : 1e30;
    h->far_rows = reach <= (double)kern::kFarMaxCells;
  }
  // the reading is sorted on a coarsened grid of at most 2^22 bins
  {
    int qf = 1;
    while ((double)((dims[0] + qf - 1) / qf) * (double)((dims[1] + qf - 1) / qf) * (double)((dims[2] + qf - 1) / qf) > (double)(1 << 22)) ++qf;
    h->qf = qf;
    h->qnx = (int)((dims[0] + qf - 1) / qf);
    h->qny = (int)((dims[1] + qf - 1) / qf);
    h->qnz = (int)((dims[2] + qf - 1) / qf);
    h->qcells = (size_t)h->qnx * (size_t)h->qny * (size_t)h->qnz;
  }
  HIP_TRY(h, h->d_qstart.ensure((h->qcells + 1) * 4));
  // wait_end = false (o3s_icp_init_reference_dev_async): the scatter may still be reading the caller's arrays when this
  // returns; everything later on this handle is ordered behind it on the stream
  if (wait_end) HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->M = M;
  h->ref_has_normals = d_normals != nullptr;
  h->ref_ready = true;
  h->reading_ready = false;  // a resident reading was prepared against the previous grid
  if (h->graph_exec) {
    (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
  }
  return O3S_OK;
}

int ensure_iteration_buffers(o3s_icp* h, int N) {
  HIP_TRY(h, h->d_t.ensure((size_t)N * 6 * 4));
  HIP_TRY(h, h->d_r.ensure((size_t)N * 6 * 4));
  HIP_TRY(h, h->d_perm.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_qcell.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_pos.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_d2.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_mq.ensure((size_t)N * sizeof(float4)));
  HIP_TRY(h, h->d_cert.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_mn.ensure((size_t)N * sizeof(float4)));
  HIP_TRY(h, h->d_hist.ensure((kHistWords + kSpecWords + kHookTraceWords) * 4));  // + the speculative digit histograms (+ the hooks build's traces)
  HIP_TRY(h, h->d_cand.ensure((size_t)nblocks(N, kern::kClsBlock) * kern::kClsBlock * sizeof(CandRec)));  // one region per classify block
  HIP_TRY(h, h->d_cand_cnt.ensure(((size_t)nblocks(N, kern::kClsBlock) * 2 + 2) * 4));  // counts [nb] + bases [nb + 1]
  HIP_TRY(h, h->d_sel.ensure(sizeof(SelScratch)));
  HIP_TRY(h, h->d_sel_part2.ensure((size_t)kCentComps * kern::kSelPartMaxBlocks * sizeof(double)));
  HIP_TRY(h, h->d_park.ensure((size_t)kern::kParkRecs * (sizeof(CandRec) + 4)));
  HIP_TRY(h, h->d_cent.ensure((size_t)nblocks(N) * kCentComps * sizeof(double)));
  HIP_TRY(h, h->d_ne.ensure((size_t)kMaxPartialBlocks * kNeComps * sizeof(double)));
  HIP_TRY(h, h->d_state.ensure(sizeof(IcpState)));
  HIP_TRY(h, h->d_T0.ensure(16 * 4));
  // the configured covariance's partials, here rather than at their first use behind the chain: an allocation moves alloc_gen, and
  // one made after a call's graph key was formed would put the capture off by a call
  if (h->cfg.error_minimizer == 1) HIP_TRY(h, h->d_cov.ensure(kCovBufBytes));
  return O3S_OK;
}

// the reading sort's count arrays: zeroed when (re)allocated or when the grid changes the split between bins and tiles; the
// kernels of prepare_reading leave them zeroed
int ensure_qcount(o3s_icp* h) {
  // whole tiles (the counts of a tile are kept transposed inside it: kern::qcount_slot), then the tile totals
  const size_t words = ((h->qcells + kern::kScanTile - 1) / kern::kScanTile) * kern::kScanTile + (size_t)kern::kMaxQTiles * kern::kTileReplicas;
  const size_t cap_before = h->d_qcount.cap;
  HIP_TRY(h, h->d_qcount.ensure(words * 4));
  if (h->d_qcount.cap != cap_before) HIP_TRY(h, hipMemsetAsync(h->d_qcount.p, 0, h->d_qcount.cap, h->stream));
  return O3S_OK;
}

int ensure_trace(o3s_icp* h, int cap) {
  cap = std::max(cap, 1);
  HIP_TRY(h, h->d_trace_T.ensure((size_t)cap * 16 * 4));
  HIP_TRY(h, h->d_trace_limit.ensure((size_t)cap * 4));
  HIP_TRY(h, h->d_trace_kept.ensure((size_t)cap * 8));
  h->trace_cap = cap;
  return O3S_OK;
}

ChainArgs chain_args(o3s_icp* h, const ChainParams& cp) {
  ChainArgs a{};
  a.N = h->N;
  // k_match2: lanes per query, by reading size (kernels)
  //   measured (converged pose, us): C2 100k: G=4 10.6, G=2 8.9, G=1 9.4;  C4 500k: 37.2 / 27.8 / 33.1.  Two lanes halve the
  //   per-query set-up every lane of a group repeats; below ~32k queries four lanes are needed to fill 1024 SIMDs.  Between 32k and
  //   64k the two are equal on the synthetic pairs (50k: 30.6 k it/s either way) and four lanes win on ray-cast sweeps against a
  //   voxel map (47k queries, 17 candidates per query: registration stage 0.267 -> 0.239 ms); from 65k up two lanes win (-1..3 %).
  a.match_g = h->N < 65536 ? 4 : 2;
  a.nb_match = round_up8(nblocks(h->N, kern::kBlock / a.match_g));  // one tile per block (steady state; the launch sizes its own grid)
  a.nb_cls = nblocks(h->N, kern::kClsBlock);
  a.nb_part = std::min(kMaxPartialBlocks, nblocks(h->N, kern::kBlock * kern::kNePPT));
  if (h->shard.active) {
    // sharded: the block partials of the normal equations are all-reduced AS THEY ARE ([27][blocks]), so the number of blocks must be
    // the same on every rank — derived from the whole reading and the world size, not from this rank's slice (slices differ by
    // one point: 2 * 512 * k + 1 points over two ranks gave 4 blocks here and 3 there, i.e. collectives of different lengths)
    const int64_t per_rank = (h->shard.n_total + h->shard.world - 1) / h->shard.world;
    a.nb_part = std::min(kMaxPartialBlocks, nblocks(per_rank, kern::kBlock * kern::kNePPT));
  }
  {  // fused selection + normal equations while the blocks fit one generation (O3S_FUSE=0 keeps the two kernels apart)
    const char* fe = O3S_HOOK_ENV("O3S_FUSE");  // read per call: the tests run both chains in one process
    const bool fuse = !(fe && std::atoi(fe) == 0);
    const int nbf = nblocks(h->N, kern::kBlock * kern::kNePPT);  // the blocks k_normal_eq would use: same partials, same bits
    a.nb_fused = (fuse && !h->shard.active && !h->many_in_flight && nbf <= kern::kFusedMaxBlocks && nbf == a.nb_part) ? nbf : 0;
  }
  a.has_n = h->read_has_normals;
  {  // the previous limit's prefix resolves the limit in k_classify: single-GPU chains with a Trimmed filter (O3S_NO_SPEC_SELECT=1: level 1 only)
    const char* ne = O3S_HOOK_ENV("O3S_NO_SPEC_SELECT");  // read per call: the tests run both in one process
    const bool spec = cp.has_trim && !cp.mirror && !h->shard.active && !(ne && std::atoi(ne) != 0);
    a.spec = spec ? h->d_hist.as<uint32_t>() + kHistWords : nullptr;
    const char* nb = O3S_HOOK_ENV("O3S_NO_BIN_COUNTERS");
    a.no_bin_counters = (nb && std::atoi(nb) != 0) ? 1 : 0;
  }
  {  // certificates: single-GPU KDTree chains (O3S_NO_CERT=1: none; a work-skipping switch of O3S_DBG would falsify them)
    const char* nc = O3S_HOOK_ENV("O3S_NO_CERT");  // read per call: the tests run both in one process
    const bool on = !cp.mirror && !h->shard.active && !(nc && std::atoi(nc) != 0) && !O3S_CP_DBG(cp, ~0);
    a.cert = on ? h->d_cert.as<float>() : nullptr;
    // the settle front of launches 2.. (O3S_NO_SETTLE_FRONT=1: the kernel of launch 1 everywhere)
    const char* nf = O3S_HOOK_ENV("O3S_NO_SETTLE_FRONT");  // read per call: the tests run both in one process
    a.front_g = (on && !(nf && std::atoi(nf) != 0)) ? kFrontLanes : 0;
  }
  float* r = h->d_r.as<float>();
  a.rx = r;
  a.ry = r + (size_t)h->N;
  a.rz = r + 2 * (size_t)h->N;
  a.rnx = r + 3 * (size_t)h->N;
  a.rny = r + 4 * (size_t)h->N;
  a.rnz = r + 5 * (size_t)h->N;
  a.cp = cp;
  a.g = h->grid;
  return a;
}

// the level-1 replicas (+ level-2 histogram right behind the 16-replica area) the chain works on: in the sharded mode they live
// inside the exchange buffer, so that the all-reduces act on them in place
uint32_t* chain_hist(o3s_icp* h) {
  return h->shard.active ? reinterpret_cast<uint32_t*>(h->shard.xbuf + kXchgI32Off) : h->d_hist.as<uint32_t>();
}
// level-1 replicas the matcher spreads its flushes over: 16; in the sharded mode max(1, 16 / world) — they travel
int chain_replicas(const o3s_icp* h) { return h->shard.active ? shard_replicas(h->shard.world) : kHistReplicas; }

// RCB = candidates per round trip of the far search: 4 for the row-disc search (C2 first iteration 50.6 -> 43.2 us), 2 for the
// ring search (the kernel stays at <= 72 VGPRs; 8 was measured there in round 2 and bought nothing)
// From 200 k queries up k_match2 also fetches the matched normal (one more gather at the end of a launch with thousands of waves
// to hide it) and k_classify streams it instead of gathering it as an exposed round trip: C4 k_classify 17.9 -> 14.8 us,
// k_match2 54.3 -> 56.9 us, 9.41 -> 9.69 k it/s.  Below, the two cancel (C2: 26.7 k either way) and k_classify keeps the gather.
inline bool normals_from_matcher(const ChainArgs& a) { return a.N >= 200000 && !a.cp.mirror; }
// the index an iteration of the chain searches: the first-iteration index (init_reference_impl step 4) for iteration 0 of a KDTree
// chain when the map has one, else the main one.  Slots (d_pos) are positions in THAT index's order: the kernels of the same iteration
// that gather by slot (k_match2's own normal fetch, k_classify) get the same index; nothing carries a slot from one iteration to the
// next (the incumbent is the matched POINT, d_mq).  A mirror chain always searches the main index: k_match_mirror writes slots in
// the main index's order (d_orig_to_sorted).  The module entry points (find_closests & co.) always use the main index.
struct RefIndex {
  const float4* ref;
  const float4* refn;
  const uint32_t* cell_start;
  GridParams g;
};
inline bool first_index_used(const o3s_icp* h, const ChainParams& cp) { return !cp.mirror && h->have_grid1 && h->far_rows; }
inline RefIndex main_index(o3s_icp* h) { return RefIndex{h->d_ref.as<float4>(), h->d_refn.as<float4>(), h->d_cell_start.as<uint32_t>(), h->grid}; }
inline RefIndex chain_index(o3s_icp* h, const ChainParams& cp, int it) {
  if (it == 0 && first_index_used(h, cp))
    return RefIndex{h->d_ref1.as<float4>(), h->ref_has_normals ? h->d_refn1.as<float4>() : h->d_refn.as<float4>(), h->d_cell_start1.as<uint32_t>(), h->grid1};
  return main_index(h);
}
// the entry point of k_match2 for a launch: the overload with the seventh template argument is the settle front
template <bool STATS, int G, int UN, int RCB, bool FAR, bool CERT, bool FRONT>
constexpr auto match2_kernel() {
  if constexpr (FRONT) return &kern::k_match2<STATS, G, UN, RCB, FAR, CERT, true>;
  else return &kern::k_match2<STATS, G, UN, RCB, FAR, CERT>;
}
// FRONT: the settle front (kernels: k_match2) — one lane per query up to the settle decision, G lanes per open query behind it
template <bool STATS, int G, bool CERT, bool FRONT = false>
void launch_match2(o3s_icp* h, const ChainArgs& a, const ChainParams& cp, const RefIndex& ix, uint32_t* spec, float* cert, hipStream_t s) {
#ifdef O3S_TEST_HOOKS
  uint32_t* const settled = CERT ? h->d_hist.as<uint32_t>() + kHistWords + kSpecWords + kSpecTrace : nullptr;
#endif
  const int nb = round_up8(nblocks(a.N, kern::kBlock / (FRONT ? 1 : G)));  // one tile of kBlock / G queries per block (FRONT: kBlock)
  // (O3S_MATCH2_PARAMS: the reading and its normals go in as one base each)
  if (h->far_rows)
    hipLaunchKernelGGL((match2_kernel<STATS, G, 2, 4, true, CERT, FRONT>()), dim3(nb), dim3(kern::kBlock), 0, s, a.rx, h->d_state.as<IcpState>(),
                       h->d_mq.as<float4>(), CERT ? cert : (float*)nullptr, h->d_pos.as<int32_t>(), a.N, chain_replicas(h) - 1, ix.ref, ix.cell_start,
                       h->d_d2.as<float>(), chain_hist(h), ix.refn, normals_from_matcher(a) ? h->d_mn.as<float4>() : (float4*)nullptr,
                       a.has_n ? a.rnx : (const float*)nullptr, spec, ix.g O3S_DBG_ARG(cp.dbg) O3S_DBG_ARG(settled));
  else
    hipLaunchKernelGGL((match2_kernel<STATS, G, 2, 2, false, CERT, FRONT>()), dim3(nb), dim3(kern::kBlock), 0, s, a.rx, h->d_state.as<IcpState>(),
                       h->d_mq.as<float4>(), CERT ? cert : (float*)nullptr, h->d_pos.as<int32_t>(), a.N, chain_replicas(h) - 1, ix.ref, ix.cell_start,
                       h->d_d2.as<float>(), chain_hist(h), ix.refn, normals_from_matcher(a) ? h->d_mn.as<float4>() : (float4*)nullptr,
                       a.has_n ? a.rnx : (const float*)nullptr, spec, ix.g O3S_DBG_ARG(cp.dbg) O3S_DBG_ARG(settled));
}
// `first`: the first iteration of a call — no incumbents yet, half the queries go through the far search.  Up to 200 k points
// it runs with FOUR lanes per query whatever the steady-state choice: the far search is a chain of dependent round trips per lane,
// and twice the lanes halve the rows and candidates each has to walk (C2: 50 -> 39.5 us; at C4 the launch is candidate-bound and
// gains nothing).  Results do not depend on the lanes per query (exact search, integer histogram).
inline int match_lanes(const o3s_icp* h, const ChainArgs& a, bool first) {
  return (first && h->far_rows && a.N < 200000) ? 4 : a.match_g;
}
void launch_match2_any(o3s_icp* h, const ChainArgs& a, const ChainParams& cp, bool stats, bool first, const RefIndex& ix, uint32_t* spec, float* cert,
                       hipStream_t s, int front_g = 0 /*lanes per open query of the settle front; 0: the launch has none*/) {
  if (cp.mirror) {
    hipLaunchKernelGGL(kern::k_match_mirror, dim3(nblocks(a.N)), dim3(kern::kBlock), 0, s, a.N, h->d_ref.as<float4>(), h->d_orig_to_sorted.as<int32_t>(),
                       h->d_perm.as<int32_t>(), h->d_state.as<IcpState>(), h->d_pos.as<int32_t>(), h->d_d2.as<float>(), h->d_mq.as<float4>(),
                       chain_hist(h));
    return;
  }
  const bool front = cert != nullptr && front_g != 0;
  const int G = match_lanes(h, a, first);
  auto go = [&](auto st_, auto g_) {
    if (front) launch_match2<decltype(st_)::value, kFrontLanes, true, true>(h, a, cp, ix, spec, cert, s);
    else if (cert) launch_match2<decltype(st_)::value, decltype(g_)::value, true>(h, a, cp, ix, spec, cert, s);
    else launch_match2<decltype(st_)::value, decltype(g_)::value, false>(h, a, cp, ix, spec, cert, s);
  };
  using std::integral_constant;
  if (stats) {
    if (G == 2) go(std::true_type{}, integral_constant<int, 2>{});
    else go(std::true_type{}, integral_constant<int, 4>{});
  } else {
    if (G == 2) go(std::false_type{}, integral_constant<int, 2>{});
    else go(std::false_type{}, integral_constant<int, 4>{});
  }
}
void launch_match_any(o3s_icp* h, const ChainArgs& a, const ChainParams& cp, bool stats, hipStream_t s, bool first = false) {
  launch_match2_any(h, a, cp, stats, first, main_index(h), nullptr, nullptr, s);  // module-level entry points: no speculation, no certificates
}
// the matcher launch of iteration `it` of a chain, on the index chain_index() picks for it
void launch_match_chain(o3s_icp* h, const ChainArgs& a, bool stats, hipStream_t s, int it, const RefIndex& ix) {
  // the first iteration of a call keeps no certificates: its far search is bound by instruction issue (their book-keeping cost it
  // 6 us at C2), the pose still moves by millimetres behind it, and on the first-iteration index its slots are in THAT index's
  // order, which nothing may carry on.  They stay 0, as k_read_prep left them: iteration 1 searches every query and leaves them.
  float* const cert = it == 0 ? nullptr : a.cert;
  // from the third launch of an issued chain or replayed chunk on, most queries settle: the settle front.
  // Launch 1 meets certificates that are all zero or stale and searches every query: it keeps the lanes it has.
  launch_match2_any(h, a, a.cp, stats, it == 0, ix, a.spec, cert, s, it >= 2 ? a.front_g : 0);
}

// large readings (more classify blocks than the finishing block has threads): the candidate sweep of the two-kernel chain runs on many
// blocks first
inline bool sel_partial(const ChainArgs& a) {
  const char* pe = O3S_HOOK_ENV("O3S_SEL_PARTIAL");  // read per call (A/B runs, tests of both paths): 0 keeps the single-block sweep
  return a.nb_cls > kern::kFinThreads && !(pe && std::atoi(pe) == 0);
}

// the degeneracy-aware step's launches between the normal equations and k_solve (degeneracy_dev.h): k_constrain, in ANALYSE mode
// behind the three analysis kernels on this iteration's kept pairs.  `set`: the module-level minimiser's own set (no trace)
constexpr int kDegMaskCap = 4096;  // ensure_trace's bound
constexpr size_t kDegBufBytes = sizeof(kern::DegLast) + (size_t)kDegMaskCap * 4;
// the area of the values (o3s_degeneracy_partial.h), in bytes: the strong-pair partials [12][blocks], the last record, the trace
// (one partial mask and six values per iteration)
constexpr size_t kDegpOffLast = (size_t)kMaxPartialBlocks * kern::kLocSums * sizeof(double);
constexpr size_t kDegpOffMasks = kDegpOffLast + sizeof(kern::DegPartialLast);
constexpr size_t kDegpOffValues = kDegpOffMasks + (size_t)kDegMaskCap * 4;
constexpr size_t kDegpBufBytes = kDegpOffValues + (size_t)kDegMaskCap * 6 * sizeof(double);
static_assert(kDegpOffLast % 8 == 0 && kDegpOffValues % 8 == 0, "doubles on 8-byte boundaries");
inline bool deg_partial_live(const o3s_icp* h) { return h->deg_partial && h->deg.mode == O3S_DEGENERACY_ANALYSE; }
// `vals`: the module-level minimiser's values for the rows of `set`, in the mask's order (k_constrain_values)
void launch_constrain(o3s_icp* h, const ChainArgs& a, int nb, hipStream_t s, const kern::DegFixed* set = nullptr, const double* vals = nullptr) {
  IcpState* st = h->d_state.as<IcpState>();
  kern::DegLast* last = h->d_deg.as<kern::DegLast>();
  uint32_t* masks = set ? nullptr : reinterpret_cast<uint32_t*>(h->d_deg.as<char>() + sizeof(kern::DegLast));
  kern::LocThresholds th{};
  if (set && vals) {
    kern::DegValuesIo io{};
    for (int j = 0; j < 6; ++j) io.fixed_vals[j] = vals[j];
    hipLaunchKernelGGL(kern::k_constrain_values, dim3(1), dim3(kern::kBlock), 0, s, h->d_ne.as<double>(), nb, st, *set, (const double*)nullptr, 0,
                       (const double*)nullptr, th, 0, last, masks, kDegMaskCap, io);
    return;
  }
  if (set || h->deg.mode == O3S_DEGENERACY_FIXED) {
    hipLaunchKernelGGL(kern::k_constrain, dim3(1), dim3(kern::kBlock), 0, s, h->d_ne.as<double>(), nb, st, set ? *set : h->deg_fixed,
                       (const double*)nullptr, 0, (const double*)nullptr, th, 0, last, masks, kDegMaskCap);
    return;
  }
  const o3s_localizability_params& p = h->deg.loc_params;
  th = kern::LocThresholds{p.filter_min, p.strong_min, p.sum_all_min, p.sum_strong_min, p.sum_partial_min};
  const int nbl = loc_blocks(a.N);
  double* base = h->d_loc.as<double>();
  double *part1 = base, *dirs = base + kLocOffDirs, *part2 = base + kLocOffPart2;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base + kLocOffCnt);
  unsigned long long* t_start = reinterpret_cast<unsigned long long*>(base + kLocOffStart);
  hipLaunchKernelGGL(kern::k_loc_hessian, dim3(nbl), dim3(kern::kBlock), 0, s, a.rx, a.ry, a.rz, a.N, h->d_mn.as<float4>(), h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), a.cp.max_out_r2, st, (const float*)nullptr, (const float*)nullptr, part1, t_start, 1);
  hipLaunchKernelGGL(kern::k_loc_eig, dim3(1), dim3(kern::kBlock), 0, s, part1, nbl, dirs, (const IcpState*)st);
  if (h->deg_partial) {  // the same launches, the flagged instantiations: the strong-pair sums ride on pass 2, k_constrain_values applies them
    char* pb = h->d_degp.as<char>();
    double* pp = reinterpret_cast<double*>(pb);
    const kern::LocPartialIo pio{h->d_mq.as<float4>(), nullptr, pp};
    hipLaunchKernelGGL(kern::k_loc_contrib_partial, dim3(nbl), dim3(kern::kBlock), 0, s, a.rx, a.ry, a.rz, a.N, h->d_mn.as<float4>(),
                       h->d_pos.as<int32_t>(), h->d_d2.as<float>(), a.cp.max_out_r2, st, (const float*)nullptr, (const float*)nullptr, dirs, p.filter_min,
                       p.strong_min, part2, cnt, 1, pio);
    kern::DegValuesIo io{};
    io.pp_part = pp;
    io.last = reinterpret_cast<kern::DegPartialLast*>(pb + kDegpOffLast);
    io.pmasks = reinterpret_cast<uint32_t*>(pb + kDegpOffMasks);
    io.values = reinterpret_cast<double*>(pb + kDegpOffValues);
    hipLaunchKernelGGL(kern::k_constrain_values, dim3(1), dim3(kern::kBlock), 0, s, h->d_ne.as<double>(), nb, st, kern::DegFixed{}, part2, nbl, dirs, th,
                       (int)h->deg.min_category, last, masks, kDegMaskCap, io);
    return;
  }
  hipLaunchKernelGGL(kern::k_loc_contrib, dim3(nbl), dim3(kern::kBlock), 0, s, a.rx, a.ry, a.rz, a.N, h->d_mn.as<float4>(), h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), a.cp.max_out_r2, st, (const float*)nullptr, (const float*)nullptr, dirs, p.filter_min, p.strong_min, part2, cnt, 1);
  hipLaunchKernelGGL(kern::k_constrain, dim3(1), dim3(kern::kBlock), 0, s, h->d_ne.as<double>(), nb, st, kern::DegFixed{}, part2, nbl, dirs, th,
                     (int)h->deg.min_category, last, masks, kDegMaskCap);
}

void launch_iteration(o3s_icp* h, const ChainArgs& a, bool stats, hipEvent_t* ev /*6 events or null*/, int it) {
  IcpState* st = h->d_state.as<IcpState>();
  hipStream_t s = h->stream;
  const int mode = kern::kModeCentroid | (a.cp.has_normal_gate ? kern::kModeGate : 0) | (normals_from_matcher(a) ? kern::kModeNormalReady : 0);
  if (ev) (void)hipEventRecord(ev[0], s);
  const RefIndex ix = chain_index(h, a.cp, it);
  launch_match_chain(h, a, stats, s, it, ix);
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(kern::k_classify, dim3(a.nb_cls), dim3(kern::kClsBlock), 0, s, a.rx, st, h->d_pos.as<int32_t>(), h->d_d2.as<float>(),
                     h->d_mq.as<float4>(), a.spec, a.N, mode, h->d_mn.as<float4>(), ix.ref, ix.refn, h->d_hist.as<uint32_t>(),
                     h->d_sel.as<SelScratch>(), h->d_cand.as<CandRec>(), h->d_cand_cnt.as<uint32_t>(),
                     h->d_hist.as<uint32_t>() + (size_t)kHistReplicas * kHistBins, h->d_cent.as<double>(), kHistReplicas, 10, 1023u,
                     a.cp.mirror ? kern::kInfF : ix.g.max_r2, a.cp O3S_DBG_ARG(a.no_bin_counters));
  if (ev) (void)hipEventRecord(ev[2], s);
  uint32_t* hist2 = h->d_hist.as<uint32_t>() + (size_t)kHistReplicas * kHistBins;
  if (a.nb_fused > 0) {  // selection + normal equations in one launch (kern::k_sel_ne); timed under "sel_finish"
    hipLaunchKernelGGL(kern::k_sel_ne, dim3(a.nb_fused), dim3(kern::kFinThreads), kern::kSelCap * 4, s, st, a.rx, h->d_pos.as<int32_t>(),
                       h->d_d2.as<float>(), h->d_mq.as<float4>(), h->d_mn.as<float4>(), a.N, a.nb_cls, mode, h->d_sel.as<SelScratch>(),
                       h->d_cand_cnt.as<uint32_t>(), h->d_hist.as<uint32_t>(), h->d_cent.as<double>(), h->d_cand.as<CandRec>(),
                       h->d_ne.as<double>(), a.cp);
    if (ev) (void)hipEventRecord(ev[3], s);
    if (ev) (void)hipEventRecord(ev[4], s);
    if (h->deg.mode != O3S_DEGENERACY_OFF) launch_constrain(h, a, a.nb_fused, s);  // (a profiled call times it with k_solve)
    hipLaunchKernelGGL(kern::k_solve, dim3(1), dim3(kern::kBlock), 0, s, h->d_ne.as<double>(), a.nb_fused, a.N, st, h->d_trace_T.as<float>(),
                       h->d_trace_limit.as<float>(), h->d_trace_kept.as<int64_t>(), h->trace_cap, 1, h->post.dev, a.cp);
    if (ev) (void)hipEventRecord(ev[5], s);
    return;
  }
  {
    const bool partial = sel_partial(a);
    const int nbp = partial ? std::min(kern::kSelPartMaxBlocks, nblocks(a.nb_cls, 4)) : 0;
    CandRec* park_rec = h->d_park.as<CandRec>();
    uint32_t* park_key = reinterpret_cast<uint32_t*>(h->d_park.as<char>() + (size_t)kern::kParkRecs * sizeof(CandRec));
    if (partial)
      hipLaunchKernelGGL(kern::k_sel_partial, dim3(nbp), dim3(kern::kFinThreads), 0, s, st, h->d_sel.as<SelScratch>(), h->d_cand.as<CandRec>(),
                         h->d_cand_cnt.as<uint32_t>(), hist2, a.nb_cls, mode, h->d_sel_part2.as<double>(), park_rec, park_key);
    hipLaunchKernelGGL(kern::k_sel_finish, dim3(1), dim3(kern::kFinThreads), kern::kSelCap * 4, s, (uint32_t*)nullptr, st,
                       h->d_sel.as<SelScratch>(), h->d_cand_cnt.as<uint32_t>(), hist2, h->d_cent.as<double>(), a.nb_cls, mode,
                       h->d_cand_cnt.as<uint32_t>() + a.nb_cls, h->d_cand.as<CandRec>(),
                       partial ? h->d_sel_part2.as<double>() : (const double*)nullptr, nbp, park_rec, park_key, a.cp);
  }
  if (ev) (void)hipEventRecord(ev[3], s);
  hipLaunchKernelGGL(kern::k_normal_eq, dim3(a.nb_part), dim3(kern::kBlock), 0, s, a.rx, (const IcpState*)st, h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), h->d_mq.as<float4>(), h->d_mn.as<float4>(), a.N, h->d_ne.as<double>(), h->d_hist.as<uint32_t>(), a.cp);
  if (ev) (void)hipEventRecord(ev[4], s);
  if (h->deg.mode != O3S_DEGENERACY_OFF) launch_constrain(h, a, a.nb_part, s);
  hipLaunchKernelGGL(kern::k_solve, dim3(1), dim3(kern::kBlock), 0, s, h->d_ne.as<double>(), a.nb_part, a.N, st, h->d_trace_T.as<float>(),
                     h->d_trace_limit.as<float>(), h->d_trace_kept.as<int64_t>(), h->trace_cap, 1, h->post.dev, a.cp);
  if (ev) (void)hipEventRecord(ev[5], s);
}

// One iteration of the one-pair-sharded mode: four kernels with the three global quantities formed by three all-reduces of
// regions of the exchange buffer between them (csrc/icp_shard_kernels.h).  Everything is enqueued on the handle's
// stream; the callback enqueues the collective on (or ordered after) the same stream.
int launch_iteration_sharded(o3s_icp* h, const ChainArgs& a, bool stats, int it) {
  IcpState* st = h->d_state.as<IcpState>();
  hipStream_t s = h->stream;
  // no centroid partials from k_classify here: the raw moments of k_shard_moments carry the sums of p and q themselves
  const int mode = (a.cp.has_normal_gate ? kern::kModeGate : 0) | (normals_from_matcher(a) ? kern::kModeNormalReady : 0);
  uint8_t* xb = h->shard.xbuf;
  double* xm = reinterpret_cast<double*>(xb + kXchgMOff);
  uint32_t* l1 = reinterpret_cast<uint32_t*>(xb + kXchgI32Off);
  uint32_t* l2 = l1 + kXchgL1Words;
  auto exchange = [&](int64_t byte_off, int64_t count, int32_t dtype) -> int {
    const int rc = h->shard.fn(h->shard.user, xb + byte_off, byte_off, count, dtype, (void*)s);
    if (rc != 0) {
      h->err = "shard exchange callback failed (rc " + std::to_string(rc) + ")";
      return O3S_ERR_HIP;
    }
    return O3S_OK;
  };
  int rc;
  const int R = chain_replicas(h);
  const RefIndex ix = chain_index(h, a.cp, it);  // (every rank holds the same reference, so every rank picks the same index)
  launch_match_chain(h, a, stats, s, it, ix);  // level-1 replicas = region I of the exchange buffer (chain_hist), R of them
  if ((rc = exchange(kXchgI32Off, (int64_t)R * kHistBins, O3S_XCHG_INT32)) != O3S_OK) return rc;
  hipLaunchKernelGGL(kern::k_classify, dim3(a.nb_cls), dim3(kern::kClsBlock), 0, s, a.rx, st, h->d_pos.as<int32_t>(), h->d_d2.as<float>(),
                     h->d_mq.as<float4>(), (const uint32_t*)nullptr, a.N, mode, h->d_mn.as<float4>(), ix.ref, ix.refn, l1, h->d_sel.as<SelScratch>(),
                     h->d_cand.as<CandRec>(), h->d_cand_cnt.as<uint32_t>(), l2, h->d_cent.as<double>(), R, 20 - kShardL2Bits,
                     (uint32_t)(kShardL2Bins - 1), kern::kInfF, a.cp);
  if (a.cp.has_trim && (rc = exchange(kXchgI32Off + (int64_t)kXchgL1Words * 4, kShardL2Bins, O3S_XCHG_INT32)) != O3S_OK) return rc;
  hipLaunchKernelGGL(kern::k_shard_moments, dim3(a.nb_part + 1), dim3(kern::kBlock), 0, s, a.cp, st, h->d_sel.as<SelScratch>(), l2, a.rx, a.ry, a.rz, a.N,
                     h->d_mq.as<float4>(), h->d_mn.as<float4>(), h->d_pos.as<int32_t>(), h->d_d2.as<float>(), xm, a.nb_part, l1, R,
                     h->d_cand.as<CandRec>(), h->d_cand_cnt.as<uint32_t>(), a.nb_cls, h->d_cand_cnt.as<uint32_t>() + a.nb_cls);
  if ((rc = exchange(kXchgMOff, shard_moment_doubles(a.nb_part), O3S_XCHG_FLOAT64)) != O3S_OK) return rc;
  hipLaunchKernelGGL(kern::k_solve_shard, dim3(1), dim3(kern::kBlock), 0, s, a.cp, st, h->d_sel.as<SelScratch>(), l2, xm, a.nb_part,
                     (int)std::min<int64_t>(h->shard.n_total, 0x7fffffff), h->d_trace_T.as<float>(), h->d_trace_limit.as<float>(),
                     h->d_trace_kept.as<int64_t>(), h->trace_cap, h->post.dev);
  return O3S_OK;
}

void init_state(IcpState& st) {
  std::memset(&st, 0, sizeof(st));
  hidentity(st.T_iter);
  st.limit = std::numeric_limits<float>::infinity();
}

bool graph_key_equal(const o3s_icp::GraphKey& a, const o3s_icp::GraphKey& b) {
  return a.N == b.N && a.iters == b.iters && a.nb == b.nb && a.has_n == b.has_n && a.gen == b.gen && a.deg == b.deg && a.loc == b.loc && std::memcmp(a.ptrs, b.ptrs, sizeof(a.ptrs)) == 0 &&
         std::memcmp(&a.cp, &b.cp, sizeof(ChainParams)) == 0 && std::memcmp(&a.g, &b.g, sizeof(GridParams)) == 0 && a.have_grid1 == b.have_grid1 &&
         std::memcmp(&a.g1, &b.g1, sizeof(GridParams)) == 0;
}

// transform + spatial sort of the reading; with reset_chain the first kernel also resets what a chain starts from
// (histograms, selection hand-off, incumbents, state — kern::PrepInit): no separate fill / copy commands
int prepare_reading(o3s_icp* h, const float* T0, bool sort, bool reset_chain, bool seed_differential) {
  const int N = h->N;
  const float4* in = reinterpret_cast<const float4*>(h->ext_xyzw ? h->ext_xyzw : h->d_in_xyzw.p);
  const float* in_n = h->read_has_normals ? reinterpret_cast<const float*>(h->ext_n ? h->ext_n : h->d_in_n.p) : nullptr;
  kern::Mat16 T0v;
  std::memcpy(T0v.v, T0, 16 * sizeof(float));
  kern::PrepInit init{};
  if (reset_chain) {
    init.hist = chain_hist(h);
    init.hist_words = h->shard.active ? (int)(kXchgL1Words + kShardL2Bins) : (int)kHistWords;  // level-1 replicas + the level-2 histogram behind them
#ifdef O3S_TEST_HOOKS
    if (!h->shard.active) init.hist_words += (int)(kSpecWords + kHookTraceWords);  // hooks build: the traces start empty every call
#endif
    init.sel = h->d_sel.as<uint32_t>();
    init.sel_words = (int)(sizeof(SelScratch) / 4);
    init.mq = h->d_mq.as<float4>();
    init.cert = h->d_cert.as<float>();
    init.state = h->d_state.as<IcpState>();
    init.seed_differential = seed_differential ? 1 : 0;
    init.seq = h->call_seq;
  }
  float* t = h->d_t.as<float>();
  float* r = h->d_r.as<float>();
  const size_t n = (size_t)N;
  const int nb = nblocks(N);
  if (sort) {
    // 4 launches: transform + bin counts + arrival ranks | bin starts | who sits where | stable placement.  The count arrays are
    // all zeros between calls (zeroed when allocated, cleared by the kernels that read them): no per-call memset.
    const int n_tiles = (int)((h->qcells + kern::kScanTile - 1) / kern::kScanTile);
    int rc = ensure_qcount(h);
    if (rc != O3S_OK) return rc;
    uint32_t* counts = h->d_qcount.as<uint32_t>();
    uint32_t* tile_cnt = counts + (size_t)n_tiles * kern::kScanTile;
    uint32_t* ticket = h->d_d2.as<uint32_t>();  // free until the first matcher launch, like d_pos below
    hipLaunchKernelGGL(kern::k_read_prep, dim3(nb), dim3(kern::kBlock), 0, h->stream, in, in_n, N, T0v, h->grid, t, t + n,
                       t + 2 * n, t + 3 * n, t + 4 * n, t + 5 * n, h->d_qcell.as<uint32_t>(), counts, h->qf, h->qnx,
                       h->qny, init, ticket, tile_cnt, (int32_t*)nullptr);
    hipLaunchKernelGGL(kern::k_read_starts, dim3(n_tiles), dim3(kern::kBlock), 0, h->stream, counts, (int64_t)h->qcells, tile_cnt,
                       h->d_qstart.as<uint32_t>());
    // stable counting sort: every point is placed by the rank of its input index inside its bin.
    // d_pos is free until the first matcher launch and holds the slot -> index table in between.
    const char* so = O3S_HOOK_ENV("O3S_SCATTER_ORDER");  // test hook: reversed arrival order, same placed reading
    int32_t* who = h->d_pos.as<int32_t>();
    hipLaunchKernelGGL(kern::k_read_scatter, dim3(nb), dim3(kern::kBlock), 0, h->stream, N, h->d_qcell.as<uint32_t>(), h->d_qstart.as<uint32_t>(),
                       ticket, who, tile_cnt, n_tiles, (so && std::atoi(so) == 1) ? 1 : 0);
    hipLaunchKernelGGL(kern::k_read_place, dim3(nb), dim3(kern::kBlock), 0, h->stream, N, h->d_qcell.as<uint32_t>(), h->d_qstart.as<uint32_t>(), who, t,
                       t + n, t + 2 * n, t + 3 * n, t + 4 * n, t + 5 * n, h->read_has_normals ? 1 : 0, r, r + n, r + 2 * n, r + 3 * n, r + 4 * n,
                       r + 5 * n, h->d_perm.as<int32_t>());
  } else {
    hipLaunchKernelGGL(kern::k_read_prep, dim3(nb), dim3(kern::kBlock), 0, h->stream, in, in_n, N, T0v, h->grid, r, r + n,
                       r + 2 * n, r + 3 * n, r + 4 * n, r + 5 * n, (uint32_t*)nullptr, (uint32_t*)nullptr, 1, 1, 1, init, (uint32_t*)nullptr,
                       (uint32_t*)nullptr, h->d_perm.as<int32_t>());
  }
  HIP_TRY(h, hipGetLastError());
  h->prepared_N = N;
  return O3S_OK;
}

int push_state(o3s_icp* h, const IcpState& st) {
  h->stage->state = st;
  HIP_TRY(h, hipMemcpyAsync(h->d_state.p, &h->stage->state, sizeof(IcpState), hipMemcpyHostToDevice, h->stream));
  return O3S_OK;
}
int pull_state(o3s_icp* h) {
  HIP_TRY(h, hipMemcpyAsync(&h->stage->state, h->d_state.p, sizeof(IcpState), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return O3S_OK;
}

// Issues the call's next segment and counts it: one replay of the captured graph (`step` iterations; past max_iters they are
// no-ops), or the next iterations launch by launch up to iters_cap, each between its six events when profiling.  Unless the chain
// is certain to end inside what is now issued, ev_end is recorded right behind the segment's last launch: the look that follows
// learns from it that everything issued has run without ending the chain.  The capture window (`capturing`) records the first
// segment of an eager plan: no event, and a failed launch fails the capture without a message.  A failed exchange callback ends
// the segment with its error.
int issue_segment(o3s_icp* h, Call& c, bool capturing = false) {
  const int n = c.issued ? c.step : c.first;
  if (c.issue == Call::kReplay) {
    HIP_TRY(h, hipGraphLaunch(h->graph_exec, h->stream));
    c.issued += n;
  } else {
    for (const int end = std::min(c.issued + n, c.iters_cap); c.issued < end; ++c.issued) {
      if (!h->shard.active) {
        launch_iteration(h, c.a, c.stats, c.issue == Call::kProfiled ? &h->prof_events[(size_t)c.issued * 6] : nullptr, c.issued);
        continue;
      }
      const int rc = launch_iteration_sharded(h, c.a, c.stats, c.issued);
      if (rc != O3S_OK) return rc;
    }
    if (capturing) return hipGetLastError() == hipSuccess ? O3S_OK : O3S_ERR_HIP;
    HIP_TRY(h, hipGetLastError());
  }
  if (!c.ends_inside()) HIP_TRY(h, hipEventRecord(h->ev_end, h->stream));
  return O3S_OK;
}

// Plans one compute() (Call) and enqueues its first part on the handle's stream: the reading's preparation and the first segment
// of the iteration chain.  Never looks at the chain's post: compute_finish does, so several handles can be in flight at once.
int start_call(o3s_icp* h, const float* T_init) {
  Call& c = h->call;
  c.live = false;
  h->cov_valid = h->elements_valid = h->pose_valid = false;
  h->deg_trace_valid = h->deg_partial_valid = false;
#ifdef O3S_TEST_HOOKS
  h->looks.clear();
#endif
  if (h->shard.active && h->deg.mode != O3S_DEGENERACY_OFF)
    return fail(h, O3S_ERR_BAD_CONFIG, "the degeneracy-aware step is not available in the sharded mode");
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "compute before a successful init_reference");
  if (!h->reading_ready || h->N <= 0) return fail(h, O3S_ERR_EMPTY_READING, "the reading point cloud is empty");
  if (!h->ref_has_normals) return fail(h, O3S_ERR_BAD_SHAPE, "point-to-plane needs reference normals");
  if (h->cfg.matcher == 1 && (int64_t)h->N > h->M) return fail(h, O3S_ERR_BAD_SHAPE, "MirrorMatcher needs reading size <= reference size");
  HIP_TRY(h, hipSetDevice(h->device));
  const int N = h->N;
  int rc = ensure_iteration_buffers(h, N);
  if (rc != O3S_OK) return rc;
  const ChainParams cp = make_chain(h, h->read_has_normals);
  c.iters_cap = cp.max_iters > 0 ? cp.max_iters : 4096;
  rc = ensure_trace(h, std::min(c.iters_cap, 4096));
  if (rc != O3S_OK) return rc;

  // T_refMean_readMean = T_refIn_refMean^-1 * T_refIn_readIn  (LPM/ICP.cpp:373-374; reading mean forced to 0 at :364)
  float TcInv[16];
  hidentity(c.Tc);
  hidentity(TcInv);
  for (int d = 0; d < 3; ++d) {
    HM4(c.Tc, d, 3) = h->mean[d];
    HM4(TcInv, d, 3) = -h->mean[d];
  }
  hmul4(TcInv, T_init, c.T0);
  if (!hrigid(c.T0)) return fail(h, O3S_ERR_NOT_RIGID, "RigidTransformation: rotation matrix is not orthogonal (initial guess)");

  if (++h->call_seq == 0) ++h->call_seq;  // what this call's posts carry (k_read_prep writes it into the state)
  c.issued = 0;
  // the degeneracy area starts a call empty: no set used yet, every mask 0 (o3s_icp_set_degeneracy allocated it)
  if (h->deg.mode != O3S_DEGENERACY_OFF) HIP_TRY(h, hipMemsetAsync(h->d_deg.p, 0, kDegBufBytes, h->stream));
  if (deg_partial_live(h)) {  // ... and so does the area of the values: the last record and the records this call's iterations can reach
    const size_t n = (size_t)std::min(c.iters_cap, kDegMaskCap);
    HIP_TRY(h, hipMemsetAsync(h->d_degp.as<char>() + kDegpOffLast, 0, sizeof(kern::DegPartialLast) + n * 4, h->stream));  // (the masks follow the record)
    HIP_TRY(h, hipMemsetAsync(h->d_degp.as<char>() + kDegpOffValues, 0, n * 6 * sizeof(double), h->stream));
  }
  rc = prepare_reading(h, c.T0, h->cfg.sort_queries != 0 && h->cfg.matcher == 0 && !h->reading_presorted, /*reset_chain=*/true, cp.use_differential != 0);
  if (rc != O3S_OK) return rc;
  c.a = chain_args(h, cp);
  c.stats = h->cfg.match_stats != 0;
  c.issue = Call::kEager;
  if (h->shard.active && h->cfg.matcher != 0) return fail(h, O3S_ERR_BAD_CONFIG, "the sharded mode supports KDTreeMatcher only");

  // A chain that can stop by itself (a Differential checker and more than 7 iterations, or no Counter checker) is looked at every
  // kChunk iterations; a fixed-length one goes out whole.  Sharded chains keep to that on every path: each iteration carries
  // collectives the other ranks have to match, so the schedule may depend on the config only — never on this handle's history
  // (eager_hint) nor on whether THIS rank's graph capture succeeded.
  constexpr int kChunk = 5;
  const bool chunked = cp.max_iters <= 0 || (cp.use_differential && cp.max_iters > kChunk + 2);
  const int chunk = chunked ? kChunk : cp.max_iters;
  // Replay policy.  A hipGraph of the chain pays off when the same shapes come back: it is captured the SECOND time a key is seen
  // in a row and replayed from then on.  With a Differential checker the chain usually stops long before max_iters, and a graph of
  // all max_iters iterations would still issue 5 no-op launches (~1.8 us each) for every iteration after convergence: the graph
  // holds `chunk` iterations and is replayed until the post says done; the first replay's look is the one every call needs anyway.
  // Fixed-length chains (no Differential checker: the bench configurations) keep one graph of max_iters iterations.  Sharded
  // chains replay only with a capturable exchange (its collectives are graph nodes too); a profiled call is never replayed.
  const bool graph_ok = !h->profiling && h->cfg.use_graph && cp.max_iters > 0 && (!h->shard.active || h->shard.capturable);
  bool replay = false;
  if (!h->profiling && (graph_ok || !h->shard.active)) {
    o3s_icp::GraphKey key;
    key.N = N;
    key.iters = chunk;
    key.nb = c.a.nb_fused > 0 ? -c.a.nb_fused : c.a.nb_part;  // the fused and the two-kernel chain are different graphs
    key.has_n = c.a.has_n ? 1 : 0;
    key.deg = h->deg.mode != O3S_DEGENERACY_OFF ? h->deg_gen : 0;
    key.loc = h->deg.mode == O3S_DEGENERACY_ANALYSE ? h->loc_gen : 0;
    key.gen = h->alloc_gen;  // every ensure() of this call has already run (ensure_iteration_buffers / ensure_trace / prepare)
    key.ptrs[0] = h->d_r.p;
    key.ptrs[1] = h->d_pos.p;
    key.ptrs[2] = h->d_d2.p;
    key.ptrs[3] = h->d_ref.p;
    key.ptrs[4] = h->have_grid1 ? h->d_cell_start1.p : h->d_cell_start.p;  // (any re-allocation moves key.gen as well; this tells the two kinds of chain apart)
    key.ptrs[5] = h->d_trace_T.p;
    key.ptrs[6] = (const void*)(uintptr_t)((c.stats ? 1 : 0) | (h->shard.active ? 2 : 0) | (c.a.spec ? 8 : 0) | (h->cfg.error_minimizer == 1 ? 16 : 0) | (c.a.cert ? 32 : 0) | ((uintptr_t)(h->shard.active ? h->shard.world : 0) << 8));
    key.ptrs[7] = h->d_perm.p;
    key.cp = cp;
    key.g = h->grid;
    key.have_grid1 = h->have_grid1;
    if (h->have_grid1) key.g1 = h->grid1;
    const bool have = graph_ok && h->graph_exec && graph_key_equal(key, h->graph_key);
    const bool seen_before = graph_ok && h->graph_candidate_valid && graph_key_equal(key, h->graph_candidate);
    bool capture_failed = false;
    if (graph_ok && !have && seen_before) {
      if (h->graph_exec) {
        (void)hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr;
      }
      // Capture window: whatever fails inside it, the stream (possibly the caller's, o3s_icp_set_stream) must leave
      // capture mode again and the partial graph must go; the call is then issued eagerly.
      hipGraph_t graph = nullptr;
      hipError_t ge = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
      if (ge == hipSuccess) {
        c.first = chunk;
        const int src = issue_segment(h, c, /*capturing=*/true);
        c.issued = 0;
        ge = hipStreamEndCapture(h->stream, &graph);  // always: ends the capture even after a failed launch
        if (ge == hipSuccess && src != O3S_OK) ge = hipErrorUnknown;
      }
      if (ge == hipSuccess) ge = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
      if (ge != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky error: the eager chain reports its own
        h->graph_exec = nullptr;
        capture_failed = true;
      } else {
        h->graph_key = key;
        h->issue_mode = 1;
      }
    }
    h->graph_candidate = key;
    h->graph_candidate_valid = !capture_failed;
    replay = graph_ok && h->graph_exec && graph_key_equal(key, h->graph_key);
  }
  if (replay) {
    c.issue = Call::kReplay;
    c.first = c.step = chunk;
    if (h->issue_mode != 1) h->issue_mode = 2;
  } else if (h->profiling && !h->shard.active) {  // the whole chain between events, or 16 iterations at a time without a Counter checker
    c.issue = Call::kProfiled;
    c.first = c.step = cp.max_iters > 0 ? c.iters_cap : 16;
    for (int k = 0; k < kNumKernels; ++k) {
      h->kernel_ms[k] = 0.f;
      h->kernel_launches[k] = 0;
    }
    while (h->prof_events.size() < (size_t)c.iters_cap * 6) {
      hipEvent_t e;
      HIP_TRY(h, hipEventCreate(&e));
      h->prof_events.push_back(e);
    }
  } else if (h->shard.active) {
    c.first = c.step = chunk;
  } else {
    // An eager chain (a reading of a new size) is first looked at after as many iterations as the LAST call on this handle needed
    // (a mapping loop's registrations take the same three or four iterations sweep after sweep, and every iteration issued beyond
    // the last one is four launches that return at once: ~20 us of launch time per sweep), then after every second one.  The
    // iterations themselves, and so the result, do not depend on where the host looks.
    c.first = std::min(std::max(h->eager_hint, 2), 8);
    c.step = 2;
  }
  rc = issue_segment(h, c);
  if (rc != O3S_OK) return rc;
  c.live = true;
  return O3S_OK;
}

// ---- pose covariance (include/o3s_icp.h, "pose covariance"): the host's share -------------------------------------------------
// beta, alpha, gamma of the step: fp64 on the promoted fp32 entries, each rounded once
kern::CovAngles cov_angles(const float* T /*column-major step*/) {
  kern::CovAngles g{};
  g.beta = (float)(-std::asin((double)HM4(T, 2, 0)));
  g.alpha = (float)std::atan2((double)HM4(T, 2, 1), (double)HM4(T, 2, 2));
  const double cb = std::cos((double)g.beta);
  g.gamma = (float)std::atan2((double)HM4(T, 1, 0) / cb, (double)HM4(T, 0, 0) / cb);
  g.tx = HM4(T, 0, 3);
  g.ty = HM4(T, 1, 3);
  g.tz = HM4(T, 2, 3);
  return g;
}
// cov = sigma2 * H^-1 * M * H^-1 from the 42 sums; 36 NaN when H has a zero or non-finite pivot
void cov_finish(const double* sums /*H upper triangle (21), M upper triangle (21)*/, float sensor_std_dev, double* cov36) {
  double H[6][6], M[6][6], Hi[6][6], X[6][6];
  int t = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c, ++t) {
      H[a][c] = H[c][a] = sums[t];
      M[a][c] = M[c][a] = sums[kCovTri + t];
    }
  for (int a = 0; a < 6; ++a)
    for (int c = 0; c < 6; ++c) Hi[a][c] = a == c ? 1.0 : 0.0;
  bool ok = true;
  for (int k = 0; k < 6 && ok; ++k) {  // partial-pivot LU, carried out on [H | I]
    int piv = k;
    for (int r = k + 1; r < 6; ++r)
      if (std::fabs(H[r][k]) > std::fabs(H[piv][k])) piv = r;
    if (!(std::isfinite(H[piv][k]) && H[piv][k] != 0.0)) {
      ok = false;
      break;
    }
    if (piv != k)
      for (int c = 0; c < 6; ++c) {
        std::swap(H[k][c], H[piv][c]);
        std::swap(Hi[k][c], Hi[piv][c]);
      }
    for (int r = k + 1; r < 6; ++r) {
      const double f = H[r][k] / H[k][k];
      for (int c = k; c < 6; ++c) H[r][c] -= f * H[k][c];
      for (int c = 0; c < 6; ++c) Hi[r][c] -= f * Hi[k][c];
    }
  }
  if (ok)
    for (int k = 5; k >= 0; --k)  // back substitution
      for (int c = 0; c < 6; ++c) {
        double v = Hi[k][c];
        for (int j = k + 1; j < 6; ++j) v -= H[k][j] * Hi[j][c];
        Hi[k][c] = v / H[k][k];
      }
  if (!ok) {
    for (int k = 0; k < 36; ++k) cov36[k] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  const double sigma2 = (double)(sensor_std_dev * sensor_std_dev);
  for (int a = 0; a < 6; ++a)
    for (int c = 0; c < 6; ++c) {
      double v = 0.0;
      for (int j = 0; j < 6; ++j) v += Hi[a][j] * M[j][c];
      X[a][c] = v;
    }
  for (int a = 0; a < 6; ++a)
    for (int c = 0; c < 6; ++c) {
      double v = 0.0;
      for (int j = 0; j < 6; ++j) v += X[a][j] * Hi[j][c];
      cov36[c * 6 + a] = sigma2 * v;
    }
}
// k_cov + k_cov_post on the handle's stream and the wait for the 42 totals.  ext_*: the module-level source (device, 3 x n AoS).
int cov_run(o3s_icp* h, int n, const float* rx, const float* ry, const float* rz, float max_out_r2, const float* ext_p, const float* ext_q,
            const float* ext_n, const float* T_step, float sensor_std_dev, double* cov36) {
  const int nb = std::min(kMaxPartialBlocks, nblocks(n, kern::kBlock * kern::kNePPT));  // k_normal_eq's blocks: the same for every way a chain is issued
  HIP_TRY(h, h->d_cov.ensure(kCovBufBytes));
  double* part = h->d_cov.as<double>();
  double* sums = part + (size_t)kMaxPartialBlocks * kCovComps;
  unsigned long long* t_start = reinterpret_cast<unsigned long long*>(sums + kCovComps + 2);
  const kern::CovAngles ang = cov_angles(T_step);
  hipLaunchKernelGGL(kern::k_cov, dim3(nb), dim3(kern::kBlock), 0, h->stream, rx, ry, rz, n, h->d_mq.as<float4>(), h->d_mn.as<float4>(),
                     h->d_pos.as<int32_t>(), h->d_d2.as<float>(), max_out_r2, h->d_state.as<IcpState>(), ext_p, ext_q, ext_n, ang, part, t_start);
  const uint32_t seq = h->cov_mb.next();
  hipLaunchKernelGGL(kern::k_cov_post, dim3(1), dim3(kern::kBlock), 0, h->stream, part, nb, sums, t_start, h->cov_mb.dev, seq);
  HIP_TRY(h, hipGetLastError());
  double s[kCovComps + 2];
  const double t0 = host_post::now_us();
  const int w = host_post::fetch_post(h->cov_mb, seq, h->stream, reinterpret_cast<uint32_t*>(s), 2 * (kCovComps + 2), host_post::kPostVals, sums);
  h->host_wait_us += host_post::now_us() - t0;
  if (w == host_post::kPollError) return fail(h, O3S_ERR_HIP, "covariance: the kernels failed");
  std::memcpy(&h->cov_t_start, &s[kCovComps], 8);
  std::memcpy(&h->cov_t_end, &s[kCovComps + 1], 8);
  cov_finish(s, sensor_std_dev, cov36);
  return O3S_OK;
}
int cov_chain(o3s_icp* h, const ChainArgs& a, const float* dT, float sensor_std_dev, double* cov36) {
  return cov_run(h, a.N, a.rx, a.ry, a.rz, a.cp.max_out_r2, nullptr, nullptr, nullptr, dT, sensor_std_dev, cov36);
}

// the per-call diagnostics of o3s_icp_host_split_ex
void reset_call_diagnostics(o3s_icp* h) {
  h->host_issue_us = h->host_wait_us = 0.0;
  h->host_queries = 0;
  h->wait_by_post = h->wait_by_event = h->wait_by_guard = h->issue_mode = 0;
}

int compute_launch(o3s_icp* h, const float* T_init) {
  reset_call_diagnostics(h);
  const double t0 = host_post::now_us();
  const int rc = start_call(h, T_init);
  h->host_issue_us += host_post::now_us() - t0;
  return rc;
}

#ifdef O3S_TEST_HOOKS
// hooks build: the side of every dispatch switch the call took (tests/test_gpu_dispatch_boundaries.py) and the iterations issued at
// each look at the post, e.g. "looks 4,6"
void print_chain(o3s_icp* h) {
  if (!O3S_HOOK_ENV("O3S_PRINT_CHAIN")) return;
  static const char* issued[] = {"eager", "captured", "replayed"};
  const ChainArgs& a = h->call.a;
  const ChainParams& cp = a.cp;
  std::string looks;
  for (int n : h->looks) looks += (looks.empty() ? "" : ",") + std::to_string(n);
  std::fprintf(stderr,
               "o3s chain: N %d matcher %s far %s it0_index %s match_g %d first_g %d front_g %d normals_from_matcher %d nb_fused %d partial %d "
               "spec %d has_n %d issued %s looks %s\n",
               a.N, cp.mirror ? "mirror" : "kdtree", h->far_rows ? "rows" : "ring", first_index_used(h, cp) ? "first" : "main",
               cp.mirror ? 0 : a.match_g, cp.mirror ? 0 : match_lanes(h, a, true), a.cert ? a.front_g : 0, normals_from_matcher(a) ? 1 : 0, a.nb_fused,
               (!h->shard.active && a.nb_fused == 0 && sel_partial(a)) ? 1 : 0, a.spec ? 1 : 0, a.has_n ? 1 : 0,
               h->profiling ? "profiled" : issued[h->issue_mode], looks.c_str());
}
#endif

// The only look at the chain's post: waits, and issues the next segment while the chain is not done and iterations are left; then
// composes the pose.
int compute_finish(o3s_icp* h, float* T_out, o3s_icp_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  Call& c = h->call;
  if (!c.live) return fail(h, O3S_ERR_BAD_ARGUMENT, "compute_finish without a successful compute_launch");
  c.live = false;
#ifdef O3S_TEST_HOOKS
  struct PrintAtExit {  // once per call, failed chains included
    o3s_icp* h;
    ~PrintAtExit() { print_chain(h); }
  } print_at_exit{h};
#endif
  HIP_TRY(h, hipSetDevice(h->device));  // compute_batch finishes handles in turn: the current device is the last launch's
  const ChainParams& cp = c.a.cp;
  bool done = false;
  for (;;) {
    const int w = wait_post(h, h->call_seq, c.ends_inside() ? (hipEvent_t) nullptr : h->ev_end, &done);  // (issue_segment recorded ev_end)
    if (w < 0) return fail(h, O3S_ERR_HIP, "compute: a kernel of the iteration chain failed");
    if (w == 0) return fail(h, O3S_ERR_HIP, "compute: the iteration chain ended without posting its state");
    if (done || c.issued >= c.iters_cap) break;
    const double t0 = host_post::now_us();
    const int rc = issue_segment(h, c);
    h->host_issue_us += host_post::now_us() - t0;
    if (rc != O3S_OK) return rc;
  }
  // every issued iteration ran and the chain is not done (no Counter checker and the cap reached): fetch the state the slow way;
  // a profiled call waits for the stream anyway (its events have to be complete before they are read)
  if (!done || c.issue == Call::kProfiled) {
    const int rc = pull_state(h);
    if (rc != O3S_OK) return rc;
  }
  if (c.issue == Call::kProfiled) {
    const int ran = std::min(c.issued, h->stage->state.iter + (h->stage->state.status ? 1 : 0));
    for (int it = 0; it < ran; ++it)
      for (int k = 0; k < kNumKernels; ++k) {
        if (k == 3 && c.a.nb_fused > 0) continue;  // fused chain: k_sel_ne (timed as k = 2) holds the selection and the normal equations
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->prof_events[(size_t)it * 6 + k], h->prof_events[(size_t)it * 6 + k + 1]) == hipSuccess) {
          h->kernel_ms[k] += ms;
          h->kernel_launches[k] += 1;
        }
      }
  }
  if (done) std::memcpy(&h->stage->state, &h->post.host->state, sizeof(IcpState));  // posted in front of the progress word (system-scope release)
  const IcpState& st = h->stage->state;
  h->last_iters = std::min(st.iter, h->trace_cap);  // the trace stays on the device until o3s_icp_get_trace asks for it
  h->eager_hint = st.iter;
  if (stats) {
    stats->iterations = st.iter;
    stats->max_iters_reached = st.max_iters_reached;
    stats->kept_pairs = st.kept;
    stats->matched_pairs = st.n_finite;
    stats->point_used_ratio = st.point_used_ratio;
    stats->weighted_point_used_ratio = st.weighted_ratio;
    stats->last_trim_limit = cp.has_trim ? st.limit : std::numeric_limits<float>::quiet_NaN();
    // the chain's own clock: first matcher launch -> the launch that posted the final state (wall_clock64 stamps in the state)
    if (st.t_end > st.t_begin) stats->gpu_ms = (float)((double)(st.t_end - st.t_begin) / h->wall_clock_khz);
    stats->candidates_examined = (double)st.cand_count;
    stats->cells_probed = (double)st.row_count;
  }
  if (st.status != 0) {
    static const char* msgs[] = {"", "", "", "", "", "No matches available for computing distance quantiles",
                                 "ErrorMinimizer: no point to minimize", "abs rotation/translation norm not a number",
                                 "RigidTransformation: rotation matrix is not orthogonal"};
    h->err = (st.status >= 5 && st.status <= 8) ? msgs[st.status] : "device-side failure";
    return st.status;
  }
  if (!st.done && cp.max_iters <= 0) return fail(h, O3S_ERR_BAD_CONFIG, "iteration cap reached without a Counter checker");
  // icpCorrected_T_refIn_readIn = T_refIn_refMean * (T_iter * T_refMean_readMean)   (LPM/ICP.cpp:462-465)
  float tmp[16], out[16];
  hmul4(st.T_iter, c.T0, tmp);
  hmul4(c.Tc, tmp, out);
  h->last_max_out_r2 = cp.max_out_r2;
  std::memcpy(h->last_step, st.dT, sizeof(st.dT));
  if (h->cfg.error_minimizer == 1) {  // the one extra pass and round trip of the configured covariance
    const int rc = cov_chain(h, c.a, st.dT, h->cfg.sensor_std_dev, h->cov);
    if (rc != O3S_OK) return rc;
  } else {
    std::memset(h->cov, 0, sizeof(h->cov));  // ErrorMinimizer::getCovariance of the base class (LPM/ErrorMinimizer.cpp:266-270)
  }
  h->cov_valid = h->elements_valid = true;
  h->deg_trace_valid = h->deg.mode != O3S_DEGENERACY_OFF;
  h->deg_partial_valid = deg_partial_live(h);
  std::memcpy(h->last_T_iter, st.T_iter, sizeof(st.T_iter));
  h->pose_valid = h->r_is_call = true;
  std::memcpy(T_out, out, sizeof(out));
  return O3S_OK;
}

int compute_impl(o3s_icp* h, const float* T_init, float* T_out, o3s_icp_stats* stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const int rc = compute_launch(h, T_init);
  return rc != O3S_OK ? rc : compute_finish(h, T_out, stats);
}

int upload_reading(o3s_icp* h, const float* xyzw, const float* normals, int64_t N) {
  h->reading_ready = false;
  h->elements_valid = h->pose_valid = false;
  h->ext_xyzw = h->ext_n = nullptr;
  if (N <= 0) {
    h->N = 0;
    return fail(h, O3S_ERR_EMPTY_READING, "the reading point cloud is empty");
  }
  if (N > (int64_t)(1 << 30)) return fail(h, O3S_ERR_BAD_ARGUMENT, "reading larger than 2^30 points");
  if (!xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "xyzw is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, h->d_in_xyzw.ensure((size_t)N * 16));
  // compute() returns when the chain has POSTED its result, a moment before its last kernel retires: a copy from pageable memory
  // issued into a stream that is still busy takes the runtime's slow path (measured: 9.5 ms instead of 2.5 ms per call with host
  // buffers) — drain the stream first (a spin of a few microseconds), as the synchronising compute of round 3 did implicitly
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_in_xyzw.p, xyzw, (size_t)N * 16, hipMemcpyHostToDevice, h->stream));
  if (normals) {
    HIP_TRY(h, h->d_in_n.ensure((size_t)N * 12));
    HIP_TRY(h, hipMemcpyAsync(h->d_in_n.p, normals, (size_t)N * 12, hipMemcpyHostToDevice, h->stream));
  }
  h->N = (int)N;
  h->read_has_normals = normals != nullptr;
  h->reading_ready = true;
  h->reading_presorted = false;
  return O3S_OK;
}

}  // namespace

// =====================================================================================================================
// C ABI
// =====================================================================================================================
extern "C" {

int o3s_abi_version(void) { return O3S_ABI_VERSION; }

void o3s_icp_default_config(o3s_icp_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->matcher = 0;
  c->max_dist = 0.5f;
  c->epsilon = 0.01f;
  c->trim_ratio = 0.90f;
  c->max_normal_angle = 1.57f;
  c->max_dist_outlier = -1.f;
  c->use_differential = 1;
  c->min_diff_rot = 0.001f;
  c->min_diff_trans = 0.01f;
  c->smooth_length = 3;
  c->max_iters = 15;
  c->counter_first = 0;
  c->grid_cell = 0.f;
  c->sort_queries = 1;
  c->use_graph = 1;
  c->error_minimizer = 0;
  c->sensor_std_dev = 0.01f;
}

int o3s_icp_create(const o3s_icp_config* cfg, int device, o3s_icp** out) {
  if (!cfg || !out) {
    g_create_error = "NULL argument";
    return O3S_ERR_BAD_ARGUMENT;
  }
  *out = nullptr;
  std::string why;
  const int vc = validate_config(*cfg, why);
  if (vc != O3S_OK) {
    g_create_error = why;
    return vc;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
    g_create_error = "no usable HIP device (this library has no CPU fallback)";
    return O3S_ERR_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    g_create_error = "hipGetDeviceProperties failed";
    return O3S_ERR_HIP;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_error = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code objects only";
    return O3S_ERR_HIP;
  }
  o3s_icp* h = new o3s_icp();
  h->cfg = *cfg;
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->stage, sizeof(HostStage), hipHostMallocDefault);
  if (e == hipSuccess) e = h->mb.alloc(64);
  if (e == hipSuccess) e = h->post.alloc();
  if (e == hipSuccess) e = h->cov_mb.alloc((size_t)(host_post::kPostVals + 2 * std::max(kCovComps + 2, kern::kLocPostVals)) * 4);  // its largest post
  if (e == hipSuccess) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) h->wall_clock_khz = (double)khz;
  }
  if (e == hipSuccess) e = hipEventCreate(&h->ev_begin);
  if (e == hipSuccess) e = hipEventCreate(&h->ev_end);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)kern::k_sel_finish, hipFuncAttributeMaxDynamicSharedMemorySize, kern::kSelCap * 4);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)kern::k_sel_ne, hipFuncAttributeMaxDynamicSharedMemorySize, kern::kSelCap * 4);
  if (e != hipSuccess) {
    g_create_error = std::string("HIP initialisation failed: ") + hipGetErrorString(e);
    o3s_icp_destroy(h);
    return O3S_ERR_HIP;
  }
  h->stream = h->own_stream;
  *out = h;
  return O3S_OK;
}

void o3s_icp_destroy(o3s_icp* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
  for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
  if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
  if (h->ev_end) (void)hipEventDestroy(h->ev_end);
  if (h->stage) (void)hipHostFree(h->stage);
  h->mb.release();
  h->post.release();
  h->cov_mb.release();
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;  // the device buffers go with their members
}

const char* o3s_last_error(const o3s_icp* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int o3s_icp_set_stream(o3s_icp* h, void* hip_stream) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  (void)hipStreamSynchronize(h->stream);
  h->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : h->own_stream;
  if (h->graph_exec) {
    (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
  }
  return O3S_OK;
}

namespace {
typedef float v4f __attribute__((ext_vector_type(4)));
// One 16-byte element per lane and no loop: 6.26 TB/s on the box for a 2 GiB copy (tools/native/copy_bench.hip), the
// figure MI355X_MICROARCH.md quotes for a float4 copy (6.29).  The grid-stride forms with 4-8 loads in flight per lane
// that this entry used in round 1 stop at 4.4-4.8 TB/s (as does hipMemcpyDtoD, 4.8): a block that walks eight strides
// apart keeps eight DRAM pages open per channel instead of one.
__global__ void __launch_bounds__(256) k_stream_copy(const v4f* __restrict__ src, v4f* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
}  // namespace

int o3s_stream_copy_gbs(int device, int64_t bytes, int32_t reps, double* gbs) {
  if (!gbs || bytes < 16 || reps < 1) return O3S_ERR_BAD_ARGUMENT;
  *gbs = 0.0;
  if (hipSetDevice(device) != hipSuccess) return O3S_ERR_HIP;
  const size_t n = (size_t)bytes / 16;
  if (n > (size_t)0x7fffffff * 256) return O3S_ERR_BAD_ARGUMENT;
  DevMem ma, mb;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = O3S_ERR_HIP;
  if (ma.reset(n * 16) == hipSuccess && mb.reset(n * 16) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
      hipEventCreate(&e1) == hipSuccess && hipMemset(ma.p, 1, n * 16) == hipSuccess && hipMemset(mb.p, 0, n * 16) == hipSuccess) {
    void *a = ma.p, *b = mb.p;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_stream_copy, dim3(grid), dim3(256), 0, nullptr, (const v4f*)a, (v4f*)b, n);  // warm-up
    (void)hipEventRecord(e0, nullptr);
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_stream_copy, dim3(grid), dim3(256), 0, nullptr, (const v4f*)a, (v4f*)b, n);
    (void)hipEventRecord(e1, nullptr);
    float ms = 0.f;
    if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.f) {
      *gbs = 2.0 * (double)(n * 16) * reps / (ms * 1e-3) / 1e9;
      rc = O3S_OK;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

int o3s_icp_shard_configure(o3s_icp* h, int32_t rank, int32_t world, int64_t n_total, o3s_allreduce_fn fn, void* user, void* xbuf_dev) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (world <= 1 && !fn) {  // back to the single-GPU chain
    h->shard.active = false;
    h->shard.capturable = false;
    if (h->graph_exec) {
      (void)hipGraphExecDestroy(h->graph_exec);
      h->graph_exec = nullptr;
    }
    h->graph_candidate_valid = false;
    return O3S_OK;
  }
  if (!fn || world < 1 || rank < 0 || rank >= world || n_total <= 0) return fail(h, O3S_ERR_BAD_ARGUMENT, "shard_configure: bad rank / world / n_total / callback");
  if (h->cfg.error_minimizer == 1)  // (it would take one more all-reduce per call, of the 42 sums)
    return fail(h, O3S_ERR_BAD_CONFIG, "PointToPlaneWithCovErrorMinimizer (error_minimizer 1) is not available in the sharded mode");
  HIP_TRY(h, hipSetDevice(h->device));
  if (xbuf_dev) {
    h->shard.xbuf = reinterpret_cast<uint8_t*>(xbuf_dev);
  } else {
    HIP_TRY(h, h->shard.own.ensure((size_t)kXchgBytes));
    h->shard.xbuf = h->shard.own.as<uint8_t>();
  }
  HIP_TRY(h, hipMemsetAsync(h->shard.xbuf, 0, (size_t)kXchgBytes, h->stream));
  h->shard.rank = rank;
  h->shard.world = world;
  h->shard.n_total = n_total;
  h->shard.fn = fn;
  h->shard.user = user;
  h->shard.active = true;
  h->shard.capturable = false;
  if (h->graph_exec) {  // a graph captured for another exchange must not be replayed
    (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
  }
  h->graph_candidate_valid = false;
  return O3S_OK;
}

int o3s_icp_shard_set_capturable(o3s_icp* h, int yes) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (!h->shard.active) return fail(h, O3S_ERR_BAD_ARGUMENT, "shard_set_capturable: configure the sharded mode first");
  h->shard.capturable = yes != 0;
  return O3S_OK;
}

int64_t o3s_icp_shard_exchange_bytes(void) { return (int64_t)kXchgBytes; }
int64_t o3s_icp_shard_bytes_per_iteration(int32_t world, int64_t n_total) {
  if (world < 1 || n_total < 1) return 0;
  const int64_t per_rank = (n_total + world - 1) / world;
  return shard_bytes_per_iteration(world, std::min(kMaxPartialBlocks, nblocks(per_rank, kern::kBlock * kern::kNePPT)));
}

int o3s_icp_init_reference(o3s_icp* h, const float* xyzw, const float* normals, int64_t M) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (M <= 0) {
    h->ref_ready = false;
    return fail(h, O3S_ERR_EMPTY_REFERENCE, "reference cloud is empty");
  }
  if (!xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "xyzw is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, h->d_ref_in.ensure((size_t)M * 16));
  HIP_TRY(h, hipMemcpyAsync(h->d_ref_in.p, xyzw, (size_t)M * 16, hipMemcpyHostToDevice, h->stream));
  if (normals) {
    HIP_TRY(h, h->d_refn_in.ensure((size_t)M * 12));
    HIP_TRY(h, hipMemcpyAsync(h->d_refn_in.p, normals, (size_t)M * 12, hipMemcpyHostToDevice, h->stream));
  }
  return init_reference_impl(h, h->d_ref_in.as<float4>(), normals ? h->d_refn_in.as<float>() : nullptr, M);
}

int o3s_matcher_init(o3s_icp* h, const float* xyzw, const float* normals, int64_t M) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (M <= 0) {
    h->ref_ready = false;
    return fail(h, O3S_ERR_EMPTY_REFERENCE, "reference cloud is empty");
  }
  if (!xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "xyzw is NULL");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, h->d_ref_in.ensure((size_t)M * 16));
  HIP_TRY(h, hipMemcpyAsync(h->d_ref_in.p, xyzw, (size_t)M * 16, hipMemcpyHostToDevice, h->stream));
  if (normals) {
    HIP_TRY(h, h->d_refn_in.ensure((size_t)M * 12));
    HIP_TRY(h, hipMemcpyAsync(h->d_refn_in.p, normals, (size_t)M * 12, hipMemcpyHostToDevice, h->stream));
  }
  return init_reference_impl(h, h->d_ref_in.as<float4>(), normals ? h->d_refn_in.as<float>() : nullptr, M, /*wait_end=*/true, /*center=*/false);
}

int o3s_icp_init_reference_dev(o3s_icp* h, const void* d_xyzw, const void* d_normals, int64_t M) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (M > 0 && !d_xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "d_xyzw is NULL");
  return init_reference_impl(h, reinterpret_cast<const float4*>(d_xyzw), reinterpret_cast<const float*>(d_normals), M);
}

int o3s_icp_init_reference_dev_async(o3s_icp* h, const void* d_xyzw, const void* d_normals, int64_t M) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (M > 0 && !d_xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "d_xyzw is NULL");
  return init_reference_impl(h, reinterpret_cast<const float4*>(d_xyzw), reinterpret_cast<const float*>(d_normals), M, /*wait_end=*/false);
}

// Internal to the library (the resident submap's o3s_submap_set_reference; declared in csrc/cloud_ops.hip, not part of the C ABI):
// the reference's size is a word on the device — the patch has just been compacted there — and comes back with the statistics'
// post instead of a hand-over of its own.  max_M sizes the first launches; *M_out receives the count (0: O3S_ERR_EMPTY_REFERENCE).
int o3s_icp_init_reference_dev_counted_async(o3s_icp* h, const void* d_xyzw, const void* d_normals, const uint32_t* d_count, int64_t max_M,
                                             int64_t* M_out) {
  if (!h || !d_count) return O3S_ERR_BAD_ARGUMENT;
  if (max_M > 0 && !d_xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "d_xyzw is NULL");
  return init_reference_impl(h, reinterpret_cast<const float4*>(d_xyzw), reinterpret_cast<const float*>(d_normals), max_M, /*wait_end=*/false,
                             /*center=*/true, d_count, M_out);
}

int o3s_icp_synchronize(o3s_icp* h) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return O3S_OK;
}

int o3s_icp_wait_event(o3s_icp* h, void* hip_event) {
  if (!h || !hip_event) return O3S_ERR_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamWaitEvent(h->stream, reinterpret_cast<hipEvent_t>(hip_event), 0));
  return O3S_OK;
}

int o3s_icp_set_reading(o3s_icp* h, const float* xyzw, const float* normals, int64_t N) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  return upload_reading(h, xyzw, normals, N);
}

int o3s_icp_set_reading_dev(o3s_icp* h, const void* d_xyzw, const void* d_normals, int64_t N) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  h->reading_ready = false;
  h->elements_valid = h->pose_valid = false;
  if (N <= 0) {
    h->N = 0;
    return fail(h, O3S_ERR_EMPTY_READING, "the reading point cloud is empty");
  }
  if (N > (int64_t)(1 << 30)) return fail(h, O3S_ERR_BAD_ARGUMENT, "reading larger than 2^30 points");
  if (!d_xyzw) return fail(h, O3S_ERR_BAD_ARGUMENT, "d_xyzw is NULL");
  h->ext_xyzw = d_xyzw;
  h->ext_n = d_normals;
  h->N = (int)N;
  h->read_has_normals = d_normals != nullptr;
  h->reading_ready = true;
  h->reading_presorted = false;
  return O3S_OK;
}

int o3s_icp_reading_is_spatially_sorted(o3s_icp* h, int sorted) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  if (!h->reading_ready) return fail(h, O3S_ERR_EMPTY_READING, "reading_is_spatially_sorted: set a reading first");
  h->reading_presorted = sorted != 0;
  return O3S_OK;
}

int o3s_icp_compute_resident(o3s_icp* h, const float T_init[16], float T_out[16], o3s_icp_stats* stats) {
  if (!h || !T_init || !T_out) return O3S_ERR_BAD_ARGUMENT;
  return compute_impl(h, T_init, T_out, stats);
}

int o3s_icp_compute_resident_launch(o3s_icp* h, const float T_init[16]) {
  if (!h || !T_init) return O3S_ERR_BAD_ARGUMENT;
  return compute_launch(h, T_init);
}

int o3s_icp_compute_resident_finish(o3s_icp* h, float T_out[16], o3s_icp_stats* stats) {
  if (!h || !T_out) return O3S_ERR_BAD_ARGUMENT;
  return compute_finish(h, T_out, stats);
}

int o3s_icp_compute(o3s_icp* h, const float* xyzw, const float* normals, int64_t N, const float T_init[16], float T_out[16],
                    o3s_icp_stats* stats) {
  if (!h || !T_init || !T_out) return O3S_ERR_BAD_ARGUMENT;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "compute before a successful init_reference");
  const int rc = upload_reading(h, xyzw, normals, N);
  if (rc != O3S_OK) return rc;
  return compute_impl(h, T_init, T_out, stats);
}

int o3s_icp_compute_batch(o3s_icp* const* handles, int32_t n, const float* T_inits, float* T_outs, o3s_icp_stats* stats, int32_t* statuses) {
  if (!handles || n < 0 || !T_inits || !T_outs || !statuses) return O3S_ERR_BAD_ARGUMENT;
  for (int32_t k = 0; k < n; ++k)  // a handle holds ONE call in flight (its Call, the pinned stage): the same handle twice is a caller error
    for (int32_t j = 0; j < k; ++j)
      if (handles[k] && handles[k] == handles[j]) return O3S_ERR_BAD_ARGUMENT;
  for (int32_t k = 0; k < n; ++k) {  // issue every chain first (one stream per handle: the chains overlap on the GPU) ...
    o3s_icp* h = handles[k];
    if (h) h->many_in_flight = n > 1;
    statuses[k] = h ? compute_launch(h, T_inits + 16 * (size_t)k) : (int32_t)O3S_ERR_BAD_ARGUMENT;
    if (h) h->many_in_flight = false;
  }
  for (int32_t k = 0; k < n; ++k) {  // ... then collect
    if (statuses[k] != O3S_OK) {
      if (stats) std::memset(&stats[k], 0, sizeof(o3s_icp_stats));
      continue;
    }
    statuses[k] = compute_finish(handles[k], T_outs + 16 * (size_t)k, stats ? &stats[k] : nullptr);
  }
  return O3S_OK;
}

int o3s_icp_get_trace(const o3s_icp* h, float* T_iters, float* limits, int64_t* kept, int32_t cap) {
  if (!h) return 0;
  const int n = std::min((int)cap, h->last_iters);
  if (n <= 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (T_iters && hipMemcpy(T_iters, h->d_trace_T.p, (size_t)n * 16 * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (limits && hipMemcpy(limits, h->d_trace_limit.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (kept && hipMemcpy(kept, h->d_trace_kept.p, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

#ifdef O3S_TEST_HOOKS
// hooks build only (not declared in include/): how many leading bits of each iteration's trim limit k_classify resolved in the
// last call — 32 (the limit itself, from the previous limit's prefix), 21 (one digit left), 11 (level 1 only), 0 (no speculation).
// The trace word holds the depth in its low byte and, above it, the path that found the level-1 bin.
static int hook_sel_trace(const o3s_icp* h, int32_t* out, int32_t cap, int shift) {
  if (!h || !out || h->shard.active) return 0;
  const int n = std::min({(int)cap, h->last_iters, kSpecTrace});
  if (n <= 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  if (hipMemcpy(out, h->d_hist.as<uint32_t>() + kHistWords + kSpecWords, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (int k = 0; k < n; ++k) out[k] = (out[k] >> shift) & 0xff;
  return n;
}
int o3s_icp_hook_sel_depth(const o3s_icp* h, int32_t* depth, int32_t cap) { return hook_sel_trace(h, depth, cap, 0); }
// hooks build only: which path resolved the level-1 bin in each iteration of the last call — 2: the bin counters (the replicas
// stayed unread), 1: the scan of the level-1 replicas, 0: no selection (no Trimmed filter, no match at all, no speculation area)
int o3s_icp_hook_bin_path(const o3s_icp* h, int32_t* path, int32_t cap) { return hook_sel_trace(h, path, cap, 8); }
// hooks build only: per iteration of the last call, the queries whose certificate held at the head of k_match2 (`settled`) and those
// of them whose whole wave skipped the search (`skipped`); all zeros for a chain without certificates (O3S_NO_CERT=1, mirror, sharded)
int o3s_icp_hook_settled(const o3s_icp* h, int32_t* settled, int32_t* skipped, int32_t cap) {
  if (!h || !settled || !skipped || h->shard.active) return 0;
  const int n = std::min({(int)cap, h->last_iters, kSpecTrace});
  if (n <= 0) return 0;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  std::vector<uint32_t> rep((size_t)kHistReplicas * 2 * kSpecTrace);
  if (hipMemcpy(rep.data(), h->d_hist.as<uint32_t>() + kHistWords + kSpecWords + kSpecTrace, rep.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (int k = 0; k < n; ++k) {
    settled[k] = skipped[k] = 0;
    for (int r = 0; r < kHistReplicas; ++r) {
      settled[k] += (int32_t)rep[((size_t)r * 2 + 0) * kSpecTrace + k];
      skipped[k] += (int32_t)rep[((size_t)r * 2 + 1) * kSpecTrace + k];
    }
  }
  return n;
}
// hooks build only: the matches the last call's chain ended with, in the reading's input order — reference ids (-1: none; a pair the
// normal gate rejected keeps its id) and squared distances, as find_closests reports them
int64_t o3s_icp_hook_export_matches(o3s_icp* h, int32_t* ids, float* dists2, int64_t cap) {
  if (!h || !ids || !dists2 || h->shard.active || h->prepared_N <= 0 || cap < h->prepared_N) return 0;
  const int64_t N = h->prepared_N;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (h->d_mod_a.ensure((size_t)N * 4) != hipSuccess || h->d_mod_b.ensure((size_t)N * 4) != hipSuccess) return 0;
  hipLaunchKernelGGL(kern::k_export_matches, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, (int)N, h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), h->d_ref.as<float4>(), h->d_perm.as<int32_t>(), h->d_mod_a.as<int32_t>(), h->d_mod_b.as<float>());
  if (hipMemcpyAsync(ids, h->d_mod_a.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return 0;
  if (hipMemcpyAsync(dists2, h->d_mod_b.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  return N;
}
// hooks build only: the way the solver went in the last iteration of the last minimize / compute — IcpState::solve_branch as that
// call fetched it (0 LLT: the fast path or the general path at rank 6, 1 minimum norm or rank 0, 2 fp64 fallback); -1 without a handle
int o3s_test_last_solve_branch(const o3s_icp* h) { return h ? (int)h->stage->state.solve_branch : -1; }
#endif

int64_t o3s_icp_get_reading_order(const o3s_icp* h, int32_t* order, int64_t cap) {
  if (!h || !order || cap <= 0 || h->prepared_N <= 0) return 0;
  const int64_t n = std::min<int64_t>(cap, h->prepared_N);
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  if (hipMemcpy(order, h->d_perm.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

int o3s_icp_reference_mean(const o3s_icp* h, float mean3[3]) {
  if (!h || !mean3) return O3S_ERR_BAD_ARGUMENT;
  if (!h->ref_ready) return O3S_ERR_NOT_INITIALIZED;
  for (int d = 0; d < 3; ++d) mean3[d] = h->mean[d];
  return O3S_OK;
}

int o3s_icp_host_split(const o3s_icp* h, double out4[4]) {
  if (!h || !out4) return O3S_ERR_BAD_ARGUMENT;
  out4[0] = h->host_issue_us;
  out4[1] = h->host_wait_us;
  out4[2] = (double)h->host_queries;
  out4[3] = h->stage->state.t_begin > h->stage->state.t_prep ? 1e3 * (double)(h->stage->state.t_begin - h->stage->state.t_prep) / h->wall_clock_khz : 0.0;
  return O3S_OK;
}

int o3s_icp_host_split_ex(const o3s_icp* h, double out8[8]) {
  if (!h || !out8) return O3S_ERR_BAD_ARGUMENT;
  const int rc = o3s_icp_host_split(h, out8);
  if (rc != O3S_OK) return rc;
  out8[4] = (double)h->wait_by_post;
  out8[5] = (double)h->wait_by_event;
  out8[6] = (double)h->wait_by_guard;
  out8[7] = (double)h->issue_mode;
  return O3S_OK;
}

int o3s_icp_set_profiling(o3s_icp* h, int on) {
  if (!h) return O3S_ERR_BAD_ARGUMENT;
  h->profiling = on != 0;
  return O3S_OK;
}

int o3s_icp_kernel_ms(const o3s_icp* h, float avg_ms[5], int32_t launches[5]) {
  if (!h || !avg_ms) return O3S_ERR_BAD_ARGUMENT;
  for (int k = 0; k < kNumKernels; ++k) {
    avg_ms[k] = h->kernel_launches[k] ? h->kernel_ms[k] / (float)h->kernel_launches[k] : 0.f;
    if (launches) launches[k] = h->kernel_launches[k];
  }
  return O3S_OK;
}

int o3s_icp_profile_match(o3s_icp* h, const float T_iter[16], int32_t reps, int32_t flags, float* avg_ms) {
  if (!h || !T_iter || !avg_ms || reps <= 0) return O3S_ERR_BAD_ARGUMENT;
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "profile_match before a successful init_reference");
  if (!h->reading_ready || h->N <= 0) return fail(h, O3S_ERR_EMPTY_READING, "profile_match needs a resident reading (set_reading + compute)");
  h->elements_valid = false;  // the state is replaced below
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = ensure_iteration_buffers(h, h->N);
  if (rc != O3S_OK) return rc;
  ChainParams cp = make_chain(h, h->read_has_normals);
#ifndef O3S_TEST_HOOKS
  if (flags & 0xff) return fail(h, O3S_ERR_BAD_ARGUMENT, "profile_match: the kernel switches exist in the hooks build only (make hooks)");
#endif
  IcpState st0;
  init_state(st0);
  std::memcpy(st0.T_iter, T_iter, 16 * sizeof(float));
  rc = push_state(h, st0);
  if (rc != O3S_OK) return rc;
  const ChainArgs a = chain_args(h, cp);
#ifdef O3S_TEST_HOOKS
  cp.dbg = flags & 0xff;
#endif
  // 0x100: wipe the incumbents first (with flag 8 — no outputs — every launch then runs like the first iteration of a call)
  if (flags & 0x100) HIP_TRY(h, hipMemsetAsync(h->d_mq.p, 0, (size_t)h->N * sizeof(float4), h->stream));
  auto launch = [&]() { launch_match_any(h, a, cp, false, h->stream, /*first=*/(flags & 0x100) != 0); };  // 0x100: the launch a first iteration makes (lanes per query)
  for (int k = 0; k < 3; ++k) launch();  // warm-up
  HIP_TRY(h, hipEventRecord(h->ev_begin, h->stream));
  for (int k = 0; k < reps; ++k) launch();
  HIP_TRY(h, hipEventRecord(h->ev_end, h->stream));
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev_begin, h->ev_end));
  *avg_ms = ms / (float)reps;
  HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, kHistWords * 4, h->stream));  // the launches left counts behind
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return O3S_OK;
}

// Open3D's registration result (fitness_, inlier_rmse_) over the chain's own matcher: one matcher launch on a state with done = 0
// and the evaluation pose, then k_fit + k_fit_post over the pos / d2 streams it left, and one host post.
// Exactness.  launch_match_any passes no certificate array, so the launch is the kernel without certificates: every finite query is
// searched; what it reads of earlier launches is the incumbent d_mq[i], a reference POINT, whose distance under the pose of THIS
// launch only bounds the search from above — true for any pose.  T == NULL keeps the incumbents the last launch of the compute left
// (or an evaluation since: points of the same reference all the same; a new reference retires the pose, init_reference_impl).  An
// explicit T prepares the reading anew with the reset a compute makes (incumbents wiped) and matches what iteration 0 of that
// compute matches — on the main index, where a chain's iteration 0 may search the first-iteration index: both searches are exact.
int o3s_icp_evaluate_resident(o3s_icp* h, const float T[16], float max_correspondence_distance, o3s_icp_fitness* out) {
  if (!h || !out) return O3S_ERR_BAD_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  const float r = max_correspondence_distance;
  if (!(r >= 0.f) || r > h->cfg.max_dist) return fail(h, O3S_ERR_BAD_ARGUMENT, "evaluate: max_correspondence_distance must be in [0, max_dist]");
  if (h->shard.active) return fail(h, O3S_ERR_BAD_CONFIG, "the registration fitness is not available in the sharded mode");
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "evaluate before a successful init_reference");
  if (h->call.live) return fail(h, O3S_ERR_BAD_ARGUMENT, "evaluate between compute_resident_launch and compute_resident_finish");
  // (in front of the reading's check: a new reference also retires the resident reading, and T = NULL then asks for a pose that is gone)
  if (!T && !h->pose_valid) return fail(h, O3S_ERR_NOT_INITIALIZED, "evaluate(T = NULL) needs a successful compute on this reading and reference");
  if (!h->reading_ready || h->N <= 0) return fail(h, O3S_ERR_EMPTY_READING, "evaluate needs a resident reading");
  if (h->cfg.matcher == 1 && (int64_t)h->N > h->M) return fail(h, O3S_ERR_BAD_SHAPE, "MirrorMatcher needs reading size <= reference size");
  HIP_TRY(h, hipSetDevice(h->device));
  const int N = h->N;
  int rc = ensure_iteration_buffers(h, N);
  if (rc != O3S_OK) return rc;
  HIP_TRY(h, h->d_cov.ensure(kCovBufBytes));  // the block partials share the covariance pass's area (its results are on the host)
  const ChainParams cp = make_chain(h, h->read_has_normals);
  const bool sort = h->cfg.sort_queries != 0 && h->cfg.matcher == 0 && !h->reading_presorted;
  IcpState& st0 = h->stage->eval_state;
  init_state(st0);
  const bool fresh = T != nullptr || !h->r_is_call;  // the reading is prepared here: the launch is a first-iteration one
  if (T) {  // T_refMean_readMean as start_call forms it
    float TcInv[16], T0[16];
    hidentity(TcInv);
    for (int d = 0; d < 3; ++d) HM4(TcInv, d, 3) = -h->mean[d];
    hmul4(TcInv, T, T0);
    if (!hrigid(T0)) return fail(h, O3S_ERR_NOT_RIGID, "RigidTransformation: rotation matrix is not orthogonal (evaluation pose)");
    h->r_is_call = false;
    rc = prepare_reading(h, T0, sort, /*reset_chain=*/true, false);
  } else {
    if (!h->r_is_call) rc = prepare_reading(h, h->call.T0, sort, /*reset_chain=*/true, false);
    if (rc == O3S_OK) h->r_is_call = true;
    std::memcpy(st0.T_iter, h->last_T_iter, sizeof(st0.T_iter));
  }
  if (rc != O3S_OK) return rc;
  h->elements_valid = false;  // the state and the match streams are replaced below
  HIP_TRY(h, hipMemcpyAsync(h->d_state.p, &st0, sizeof(IcpState), hipMemcpyHostToDevice, h->stream));
  const ChainArgs a = chain_args(h, cp);
  launch_match_any(h, a, cp, false, h->stream, /*first=*/fresh);
  const float r2 = r > 0.f ? r * r : h->grid.max_r2;
  const int nb = std::min(kern::kFitMaxBlocks, nblocks(N, kern::kBlock * kern::kFitPPT));
  double* part_sum = h->d_cov.as<double>();
  unsigned long long* part_cnt = reinterpret_cast<unsigned long long*>(part_sum + kern::kFitMaxBlocks);
  double* totals = part_sum + 2 * kern::kFitMaxBlocks;
  hipLaunchKernelGGL(kern::k_fit, dim3(nb), dim3(kern::kBlock), 0, h->stream, h->d_pos.as<int32_t>(), h->d_d2.as<float>(), N, r2, part_sum, part_cnt);
  const uint32_t seq = h->cov_mb.next();
  hipLaunchKernelGGL(kern::k_fit_post, dim3(1), dim3(64), 0, h->stream, part_sum, part_cnt, nb, h->d_state.as<IcpState>(), totals, h->cov_mb.dev, seq);
  HIP_TRY(h, hipGetLastError());
  double v[4];
  const int w = host_post::fetch_post(h->cov_mb, seq, h->stream, reinterpret_cast<uint32_t*>(v), 8, host_post::kPostVals, totals);
  if (w == host_post::kPollError) return fail(h, O3S_ERR_HIP, "evaluate: the kernels failed");
  unsigned long long cnt, t0, t1;
  std::memcpy(&cnt, &v[0], 8);
  std::memcpy(&t0, &v[2], 8);
  std::memcpy(&t1, &v[3], 8);
  out->n_points = N;
  out->n_correspondences = (int64_t)cnt;
  out->fitness = (double)cnt / (double)N;
  out->inlier_rmse = cnt ? std::sqrt(v[1] / (double)cnt) : 0.0;
  out->gpu_ms = t1 > t0 ? (float)((double)(t1 - t0) / h->wall_clock_khz) : 0.f;
  return O3S_OK;
}

// ---- module-level path ----------------------------------------------------------------------------------------

int o3s_icp_find_closests(o3s_icp* h, const float* query_xyzw, int64_t N, int32_t* ids, float* dists2) {
  if (!h || !ids || !dists2) return O3S_ERR_BAD_ARGUMENT;
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "find_closests before a successful init_reference");
  if (h->cfg.matcher == 1 && N > h->M) return fail(h, O3S_ERR_BAD_SHAPE, "MirrorMatcher needs reading size <= reference size");
  int rc = upload_reading(h, query_xyzw, nullptr, N);
  if (rc != O3S_OK) return rc;
  rc = ensure_iteration_buffers(h, (int)N);
  if (rc != O3S_OK) return rc;
  rc = ensure_trace(h, 1);
  if (rc != O3S_OK) return rc;
  float I[16];
  hidentity(I);
  rc = prepare_reading(h, I, h->cfg.sort_queries != 0 && h->cfg.matcher == 0, /*reset_chain=*/true, false);
  if (rc != O3S_OK) return rc;
  ChainParams cp = make_chain(h, false);
  const ChainArgs a = chain_args(h, cp);
  launch_match_any(h, a, a.cp, false, h->stream, /*first=*/true);  // no incumbents: the far search does the work
  HIP_TRY(h, h->d_mod_a.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_mod_b.ensure((size_t)N * 4));
  hipLaunchKernelGGL(kern::k_export_matches, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, (int)N, h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), h->d_ref.as<float4>(), h->d_perm.as<int32_t>(), h->d_mod_a.as<int32_t>(), h->d_mod_b.as<float>());
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(ids, h->d_mod_a.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(dists2, h->d_mod_b.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->reading_ready = false;  // the resident reading was replaced by the query
  return O3S_OK;
}

static int import_matches(o3s_icp* h, const int32_t* ids, const float* dists2, const float* weights, int64_t N) {
  HIP_TRY(h, h->d_mod_a.ensure((size_t)N * 4));
  HIP_TRY(h, h->d_mod_b.ensure((size_t)N * 4));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_a.p, ids, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_b.p, dists2, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
  if (weights) {
    HIP_TRY(h, h->d_mod_c.ensure((size_t)N * 4));
    HIP_TRY(h, hipMemcpyAsync(h->d_mod_c.p, weights, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(kern::k_import_matches, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, (int)N, h->d_mod_a.as<int32_t>(),
                     h->d_mod_b.as<float>(), weights ? h->d_mod_c.as<float>() : (const float*)nullptr, h->d_orig_to_sorted.as<int32_t>(), h->M,
                     h->d_ref.as<float4>(), h->d_pos.as<int32_t>(), h->d_d2.as<float>(), h->d_mq.as<float4>(), h->d_cert.as<float>());
  HIP_TRY(h, hipGetLastError());
  return O3S_OK;
}

int o3s_icp_outlier_weights(o3s_icp* h, const float* reading_normals, const int32_t* ids, const float* dists2, int64_t N, float* weights) {
  if (!h || !ids || !dists2 || !weights) return O3S_ERR_BAD_ARGUMENT;
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "outlier_weights before a successful init_reference");
  if (N <= 0) return fail(h, O3S_ERR_EMPTY_READING, "empty matches");
  h->elements_valid = false;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = ensure_iteration_buffers(h, (int)N);
  if (rc != O3S_OK) return rc;
  h->reading_ready = false;
  rc = import_matches(h, ids, dists2, nullptr, N);
  if (rc != O3S_OK) return rc;
  ChainParams cp = make_chain(h, reading_normals != nullptr);
  const bool any = h->cfg.trim_ratio >= 0.f || h->cfg.max_normal_angle >= 0.f || h->cfg.max_dist_outlier >= 0.f;
  IcpState st0;
  init_state(st0);
  rc = push_state(h, st0);
  if (rc != O3S_OK) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, kHistWords * 4, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->d_sel.p, 0, sizeof(SelScratch), h->stream));
  hipLaunchKernelGGL(kern::k_hist, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, h->d_d2.as<float>(), (int)N, h->d_hist.as<uint32_t>());
  {
    float* r = h->d_r.as<float>();
    const int nbc = nblocks(N, kern::kClsBlock);
    hipLaunchKernelGGL(kern::k_classify, dim3(nbc), dim3(kern::kClsBlock), 0, h->stream, r, h->d_state.as<IcpState>(), h->d_pos.as<int32_t>(),
                       h->d_d2.as<float>(), h->d_mq.as<float4>(), (const uint32_t*)nullptr, (int)N, 0, h->d_mn.as<float4>(), h->d_ref.as<float4>(),
                       h->d_refn.as<float4>(), h->d_hist.as<uint32_t>(), h->d_sel.as<SelScratch>(), h->d_cand.as<CandRec>(), h->d_cand_cnt.as<uint32_t>(),
                       h->d_hist.as<uint32_t>() + (size_t)kHistReplicas * kHistBins, h->d_cent.as<double>(), kHistReplicas, 10, 1023u, kern::kInfF, cp);
    hipLaunchKernelGGL(kern::k_sel_finish, dim3(1), dim3(kern::kFinThreads), kern::kSelCap * 4, h->stream, h->d_hist.as<uint32_t>(),
                       h->d_state.as<IcpState>(), h->d_sel.as<SelScratch>(), h->d_cand_cnt.as<uint32_t>(),
                       h->d_hist.as<uint32_t>() + (size_t)kHistReplicas * kHistBins, h->d_cent.as<double>(), nbc, 0, h->d_cand_cnt.as<uint32_t>() + nbc,
                       h->d_cand.as<CandRec>(), (const double*)nullptr, 0, (const CandRec*)nullptr, (const uint32_t*)nullptr, cp);
  }
  const float* d_rn = nullptr;
  if (reading_normals) {
    HIP_TRY(h, h->d_in_n.ensure((size_t)N * 12));
    HIP_TRY(h, hipMemcpyAsync(h->d_in_n.p, reading_normals, (size_t)N * 12, hipMemcpyHostToDevice, h->stream));
    d_rn = h->d_in_n.as<float>();
  }
  HIP_TRY(h, h->d_mod_d.ensure((size_t)N * 4));
  hipLaunchKernelGGL(kern::k_weights, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, (int)N, h->d_pos.as<int32_t>(), h->d_d2.as<float>(), d_rn,
                     h->d_refn.as<float4>(), cp, h->d_state.as<IcpState>(), any ? 1 : 0, h->d_mod_d.as<float>());
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(weights, h->d_mod_d.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
  rc = pull_state(h);
  if (rc != O3S_OK) return rc;
  if (h->stage->state.status != 0) return fail(h, h->stage->state.status, "No matches available for computing distance quantiles");
  return O3S_OK;
}

// o3s_icp_minimize, and o3s_icp_minimize_degeneracy (degeneracy_impl.h) with `set`: k_constrain in front of k_solve (with `vals`,
// o3s_icp_minimize_degen_values of degeneracy_partial_impl.h: k_constrain_values)
static int minimize_impl(o3s_icp* h, const float* reading_xyzw, const int32_t* ids, const float* dists2, const float* weights, int64_t N,
                         const kern::DegFixed* set, const double* vals /*nullable: k_constrain_values*/, float T_out[16], float A_out[36],
                         float b_out[6], float x_out[6]) {
  if (!h || !reading_xyzw || !ids || !dists2 || !weights || !T_out) return O3S_ERR_BAD_ARGUMENT;
  if (!h->ref_ready) return fail(h, O3S_ERR_NOT_INITIALIZED, "minimize before a successful init_reference");
  if (!h->ref_has_normals) return fail(h, O3S_ERR_BAD_SHAPE, "point-to-plane needs reference normals");
  int rc = upload_reading(h, reading_xyzw, nullptr, N);
  if (rc != O3S_OK) return rc;
  h->reading_ready = false;
  rc = ensure_iteration_buffers(h, (int)N);
  if (rc != O3S_OK) return rc;
  rc = ensure_trace(h, 1);
  if (rc != O3S_OK) return rc;
  float* r = h->d_r.as<float>();
  hipLaunchKernelGGL(kern::k_aos_to_soa, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, h->d_in_xyzw.as<float4>(), (int)N, r, r + (size_t)N,
                     r + 2 * (size_t)N);
  rc = import_matches(h, ids, dists2, weights, N);
  if (rc != O3S_OK) return rc;
  ChainParams cp = make_chain(h, false);
  cp.max_out_r2 = std::numeric_limits<float>::infinity();  // the caller's weights already carry every filter
  cp.has_trim = 0;
  cp.has_normal_gate = 0;
  IcpState st0;
  init_state(st0);
  rc = push_state(h, st0);
  if (rc != O3S_OK) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, kHistWords * 4, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->d_sel.p, 0, sizeof(SelScratch), h->stream));
  const ChainArgs a = chain_args(h, cp);
  IcpState* st = h->d_state.as<IcpState>();
  hipLaunchKernelGGL(kern::k_classify, dim3(a.nb_cls), dim3(kern::kClsBlock), 0, h->stream, a.rx, st, h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), h->d_mq.as<float4>(), (const uint32_t*)nullptr, a.N, kern::kModeCentroid, h->d_mn.as<float4>(),
                     h->d_ref.as<float4>(), h->d_refn.as<float4>(), h->d_hist.as<uint32_t>(), h->d_sel.as<SelScratch>(), h->d_cand.as<CandRec>(),
                     h->d_cand_cnt.as<uint32_t>(), h->d_hist.as<uint32_t>() + (size_t)kHistReplicas * kHistBins, h->d_cent.as<double>(), kHistReplicas,
                     10, 1023u, kern::kInfF, cp);
  hipLaunchKernelGGL(kern::k_sel_finish, dim3(1), dim3(kern::kFinThreads), kern::kSelCap * 4, h->stream, h->d_hist.as<uint32_t>(), st,
                     h->d_sel.as<SelScratch>(), h->d_cand_cnt.as<uint32_t>(), h->d_hist.as<uint32_t>() + (size_t)kHistReplicas * kHistBins,
                     h->d_cent.as<double>(), a.nb_cls, kern::kModeCentroid, h->d_cand_cnt.as<uint32_t>() + a.nb_cls, h->d_cand.as<CandRec>(),
                     (const double*)nullptr, 0, (const CandRec*)nullptr, (const uint32_t*)nullptr, cp);
  hipLaunchKernelGGL(kern::k_normal_eq, dim3(a.nb_part), dim3(kern::kBlock), 0, h->stream, a.rx, (const IcpState*)st, h->d_pos.as<int32_t>(),
                     h->d_d2.as<float>(), h->d_mq.as<float4>(), h->d_mn.as<float4>(), a.N, h->d_ne.as<double>(), (uint32_t*)nullptr, cp);
  if (set) launch_constrain(h, a, a.nb_part, h->stream, set, vals);
  hipLaunchKernelGGL(kern::k_solve, dim3(1), dim3(kern::kBlock), 0, h->stream, h->d_ne.as<double>(), a.nb_part, a.N, st,
                     h->d_trace_T.as<float>(), h->d_trace_limit.as<float>(), h->d_trace_kept.as<int64_t>(), h->trace_cap, 0, (HostPost*)nullptr, cp);
  HIP_TRY(h, hipGetLastError());
  rc = pull_state(h);
  if (rc != O3S_OK) return rc;
  const IcpState& s = h->stage->state;
  if (s.status != 0) return fail(h, s.status, "ErrorMinimizer: no point to minimize");
  std::memcpy(T_out, s.dT, sizeof(s.dT));
  if (A_out) std::memcpy(A_out, s.A, sizeof(s.A));
  if (b_out) std::memcpy(b_out, s.b, sizeof(s.b));
  if (x_out) std::memcpy(x_out, s.x, sizeof(s.x));
  return O3S_OK;
}

int o3s_icp_minimize(o3s_icp* h, const float* reading_xyzw, const int32_t* ids, const float* dists2, const float* weights, int64_t N,
                     float T_out[16], float A_out[36], float b_out[6], float x_out[6]) {
  return minimize_impl(h, reading_xyzw, ids, dists2, weights, N, nullptr, nullptr, T_out, A_out, b_out, x_out);
}

int o3s_icp_get_covariance(const o3s_icp* h, double cov36[36]) {
  if (!h || !cov36) return O3S_ERR_BAD_ARGUMENT;
  if (!h->cov_valid) return O3S_ERR_NOT_INITIALIZED;
  std::memcpy(cov36, h->cov, sizeof(h->cov));
  return O3S_OK;
}

int o3s_icp_covariance_gpu_us(const o3s_icp* h, double out2[2]) {
  if (!h || !out2) return O3S_ERR_BAD_ARGUMENT;
  out2[0] = out2[1] = 0.0;
  if (h->cov_t_end > h->cov_t_start) out2[0] = 1e3 * (double)(h->cov_t_end - h->cov_t_start) / h->wall_clock_khz;
  const unsigned long long chain_end = h->stage->state.t_end;
  if (h->cov_valid && h->cfg.error_minimizer == 1 && h->cov_t_end > chain_end) out2[1] = 1e3 * (double)(h->cov_t_end - chain_end) / h->wall_clock_khz;
  return O3S_OK;
}

int o3s_icp_get_last_step(const o3s_icp* h, float T_step[16]) {
  if (!h || !T_step) return O3S_ERR_BAD_ARGUMENT;
  if (!h->cov_valid) return O3S_ERR_NOT_INITIALIZED;
  std::memcpy(T_step, h->last_step, sizeof(h->last_step));
  return O3S_OK;
}

int o3s_icp_estimate_covariance(o3s_icp* h, const float* reading_c, const float* reference_c, const float* normals, int64_t K,
                                const float T_step[16], float sensor_std_dev, double cov36[36]) {
  if (!h || !reading_c || !reference_c || !normals || !T_step || !cov36) return O3S_ERR_BAD_ARGUMENT;
  if (K <= 0) return fail(h, O3S_ERR_NO_POINTS, "estimate_covariance: no pairs");
  if (K > (int64_t)(1 << 30)) return fail(h, O3S_ERR_BAD_ARGUMENT, "estimate_covariance: more than 2^30 pairs");
  if (!(sensor_std_dev >= 0.f)) return fail(h, O3S_ERR_BAD_CONFIG, "sensor_std_dev must be >= 0");
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)K * 12;
  HIP_TRY(h, h->d_mod_a.ensure(bytes));
  HIP_TRY(h, h->d_mod_b.ensure(bytes));
  HIP_TRY(h, h->d_mod_c.ensure(bytes));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (upload_reading: a copy from pageable memory into a busy stream takes the slow path)
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_a.p, reading_c, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_b.p, reference_c, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_mod_c.p, normals, bytes, hipMemcpyHostToDevice, h->stream));
  return cov_run(h, (int)K, nullptr, nullptr, nullptr, 0.f, h->d_mod_a.as<float>(), h->d_mod_b.as<float>(), h->d_mod_c.as<float>(), T_step,
                 sensor_std_dev, cov36);
}

int64_t o3s_icp_get_error_elements(o3s_icp* h, float* reading_c, float* reference_c, float* normals, int32_t* reading_idx, int64_t cap) {
  if (!h || !h->elements_valid || h->prepared_N <= 0) return 0;
  const int N = h->prepared_N;
  if (hipSetDevice(h->device) != hipSuccess) return 0;
  if (h->d_mod_d.ensure((size_t)N * 10 * 4) != hipSuccess) return 0;
  float* d_out = h->d_mod_d.as<float>();
  int32_t* d_keep = reinterpret_cast<int32_t*>(d_out + (size_t)N * 9);
  const float* r = h->d_r.as<float>();
  hipLaunchKernelGGL(kern::k_cov_elements, dim3(nblocks(N)), dim3(kern::kBlock), 0, h->stream, r, r + (size_t)N, r + 2 * (size_t)N, N,
                     h->d_mq.as<float4>(), h->d_mn.as<float4>(), h->d_pos.as<int32_t>(), h->d_d2.as<float>(), h->last_max_out_r2,
                     h->d_state.as<IcpState>(), d_out, d_keep);
  std::vector<float> out((size_t)N * 9);
  std::vector<int32_t> keep((size_t)N), perm((size_t)N);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
      hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(keep.data(), d_keep, keep.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(perm.data(), h->d_perm.p, perm.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  int64_t K = 0;
  for (int i = 0; i < N; ++i) {
    if (!keep[(size_t)i]) continue;
    if (K < cap) {
      const float* o = &out[(size_t)i * 9];
      for (int c = 0; c < 3; ++c) {
        if (reading_c) reading_c[K * 3 + c] = o[c];
        if (reference_c) reference_c[K * 3 + c] = o[3 + c];
        if (normals) normals[K * 3 + c] = o[6 + c];
      }
      if (reading_idx) reading_idx[K] = perm[(size_t)i];
    }
    ++K;
  }
  return K;
}

}  // extern "C"

#include "localizability_impl.h"
#include "degeneracy_impl.h"
#include "degeneracy_partial_impl.h"
