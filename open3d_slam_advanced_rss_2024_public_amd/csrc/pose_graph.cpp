// pose_graph.cpp — the pose-graph solver of include/pose_graph/o3s_pose_graph.h: Open3D's GlobalOptimization with
// GlobalOptimizationLevenbergMarquardt (Choi, Zhou, Koltun 2015: line-process pose graph, Levenberg-Marquardt), restated from the
// published method as written out in DESIGN.md section 9d.  Host C++ only: no device is opened.  fp64, no FMA contraction, edges
// in index order, every sum in a fixed order.
#include "../../include/pose_graph/o3s_pose_graph.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

// 4x4 matrices are column-major: M(r, c) = m[4 c + r]
struct M4 {
  double m[16];
  double& operator()(int r, int c) { return m[4 * c + r]; }
  double operator()(int r, int c) const { return m[4 * c + r]; }
};

M4 mul(const M4& A, const M4& B) {
  M4 C;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double s = A(r, 0) * B(0, c);
      s = s + A(r, 1) * B(1, c);
      s = s + A(r, 2) * B(2, c);
      s = s + A(r, 3) * B(3, c);
      C(r, c) = s;
    }
  return C;
}

// inverse of a pose [R t; 0 1]: [R^T, -R^T t]
M4 inv_pose(const M4& T) {
  M4 I;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) I(r, c) = T(c, r);
    double s = T(0, r) * T(0, 3);
    s = s + T(1, r) * T(1, 3);
    s = s + T(2, r) * T(2, 3);
    I(r, 3) = -s;
    I(3, r) = 0.0;
  }
  I(3, 3) = 1.0;
  return I;
}

// lin(M) = [(M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23]
void lin(const M4& M, double o[6]) {
  o[0] = (M(2, 1) - M(1, 2)) / 2.0;
  o[1] = (M(0, 2) - M(2, 0)) / 2.0;
  o[2] = (M(1, 0) - M(0, 1)) / 2.0;
  o[3] = M(0, 3);
  o[4] = M(1, 3);
  o[5] = M(2, 3);
}

// G_i T for the six generators (rotations about x, y, z, translations along x, y, z): rows of T recombined
M4 gen_times(int i, const M4& T) {
  M4 O;
  std::memset(O.m, 0, sizeof O.m);
  for (int c = 0; c < 4; ++c) {
    switch (i) {
      case 0:  // G(1, 2) = -1, G(2, 1) = 1
        O(1, c) = -T(2, c);
        O(2, c) = T(1, c);
        break;
      case 1:  // G(0, 2) = 1, G(2, 0) = -1
        O(0, c) = T(2, c);
        O(2, c) = -T(0, c);
        break;
      case 2:  // G(0, 1) = -1, G(1, 0) = 1
        O(0, c) = -T(1, c);
        O(1, c) = T(0, c);
        break;
      default:  // G(i - 3, 3) = 1
        O(i - 3, c) = T(3, c);
        break;
    }
  }
  return O;
}

// TransformVector6dToMatrix4d: [Rz(v2) Ry(v1) Rx(v0), (v3, v4, v5)]
M4 exp6(const double v[6]) {
  const double ca = std::cos(v[0]), sa = std::sin(v[0]), cb = std::cos(v[1]), sb = std::sin(v[1]), cg = std::cos(v[2]), sg = std::sin(v[2]);
  M4 T;
  std::memset(T.m, 0, sizeof T.m);
  T(0, 0) = cg * cb;
  T(0, 1) = cg * sb * sa - sg * ca;
  T(0, 2) = cg * sb * ca + sg * sa;
  T(1, 0) = sg * cb;
  T(1, 1) = sg * sb * sa + cg * ca;
  T(1, 2) = sg * sb * ca - cg * sa;
  T(2, 0) = -sb;
  T(2, 1) = cb * sa;
  T(2, 2) = cb * ca;
  T(0, 3) = v[3];
  T(1, 3) = v[4];
  T(2, 3) = v[5];
  T(3, 3) = 1.0;
  return T;
}

// TransformMatrix4dToVector6d
void log6(const M4& T, double v[6]) {
  const double sy = std::sqrt(T(0, 0) * T(0, 0) + T(1, 0) * T(1, 0));
  if (!(sy < 1e-6)) {
    v[0] = std::atan2(T(2, 1), T(2, 2));
    v[1] = std::atan2(-T(2, 0), sy);
    v[2] = std::atan2(T(1, 0), T(0, 0));
  } else {
    v[0] = std::atan2(-T(1, 2), T(1, 1));
    v[1] = std::atan2(-T(2, 0), sy);
    v[2] = 0.0;
  }
  v[3] = T(0, 3);
  v[4] = T(1, 3);
  v[5] = T(2, 3);
}

struct Graph {
  std::vector<M4> poses;
  std::vector<o3s_pose_graph_edge> edges;
};

inline double info_at(const o3s_pose_graph_edge& ed, int r, int c) { return ed.information[6 * c + r]; }

// e, and (optionally) Js, Jt (6 x 6 column-major) of one edge
void edge_terms(const Graph& g, const o3s_pose_graph_edge& ed, double e[6], double* Js, double* Jt) {
  M4 X;
  std::memcpy(X.m, ed.transformation, sizeof X.m);
  const M4 A = mul(inv_pose(X), inv_pose(g.poses[(size_t)ed.target]));  // X^-1 Tt^-1
  const M4& Ts = g.poses[(size_t)ed.source];
  lin(mul(A, Ts), e);
  if (!Js) return;
  for (int i = 0; i < 6; ++i) {
    double col[6];
    lin(mul(A, gen_times(i, Ts)), col);
    for (int r = 0; r < 6; ++r) {
      Js[6 * i + r] = col[r];
      Jt[6 * i + r] = -col[r];  // lin is linear: lin(A (-G_i) Ts) = -lin(A G_i Ts), exactly
    }
  }
}

// r^2 = e^T Lambda e
double edge_r2(const o3s_pose_graph_edge& ed, const double e[6]) {
  double r2 = 0.0;
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
    for (int c = 0; c < 6; ++c) s = s + info_at(ed, r, c) * e[c];
    r2 = r2 + e[r] * s;
  }
  return r2;
}

double line_process_weight(const Graph& g, const o3s_global_optimization_option& opt) {
  int n = 0;
  double sum = 0.0;
  for (const auto& ed : g.edges)
    if (ed.uncertain) {
      sum = sum + info_at(ed, 5, 5);
      ++n;
    }
  if (n == 0) return 0.0;
  return opt.preference_loop_closure * (opt.max_correspondence_distance * opt.max_correspondence_distance) * (sum / (double)n);
}

// F = sum over edges of l r^2 + w (sqrt(l) - 1)^2
double objective(const Graph& g, double w) {
  double F = 0.0;
  for (const auto& ed : g.edges) {
    double e[6];
    edge_terms(g, ed, e, nullptr, nullptr);
    const double l = ed.confidence, q = std::sqrt(l) - 1.0;
    F = F + (l * edge_r2(ed, e) + w * (q * q));
  }
  return F;
}

void update_confidence(Graph& g, double w) {
  for (auto& ed : g.edges) {
    if (!ed.uncertain) continue;
    double e[6];
    edge_terms(g, ed, e, nullptr, nullptr);
    const double t = w / (w + edge_r2(ed, e));
    ed.confidence = t * t;
  }
}

// H (N x N column-major, N = 6 n) and b
void linear_system(const Graph& g, std::vector<double>& H, std::vector<double>& b) {
  const size_t N = 6 * g.poses.size();
  H.assign(N * N, 0.0);
  b.assign(N, 0.0);
  for (const auto& ed : g.edges) {
    double e[6], J[2][36], LJ[2][36], Le[6];
    edge_terms(g, ed, e, J[0], J[1]);
    for (int k = 0; k < 2; ++k)
      for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 6; ++r) {
          double s = 0.0;
          for (int m = 0; m < 6; ++m) s = s + info_at(ed, r, m) * J[k][6 * c + m];
          LJ[k][6 * c + r] = s;
        }
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
      for (int m = 0; m < 6; ++m) s = s + info_at(ed, r, m) * e[m];
      Le[r] = s;
    }
    const size_t off[2] = {6 * (size_t)ed.source, 6 * (size_t)ed.target};
    const double l = ed.confidence;
    for (int a = 0; a < 2; ++a) {
      for (int bb = 0; bb < 2; ++bb)
        for (int c = 0; c < 6; ++c)
          for (int r = 0; r < 6; ++r) {
            double s = 0.0;
            for (int m = 0; m < 6; ++m) s = s + J[a][6 * r + m] * LJ[bb][6 * c + m];  // (Ja^T Lambda Jb)(r, c)
            H[(off[bb] + c) * N + off[a] + r] += l * s;
          }
      for (int r = 0; r < 6; ++r) {
        double s = 0.0;
        for (int m = 0; m < 6; ++m) s = s + J[a][6 * r + m] * Le[m];
        b[off[a] + r] -= l * s;
      }
    }
  }
}

// A x = rhs by LDL^T without pivoting (A = H + lambda I is symmetric positive definite for lambda > 0); false on a pivot that is
// not positive and finite
bool ldlt_solve(std::vector<double> A, size_t N, const std::vector<double>& rhs, std::vector<double>& x) {
  std::vector<double> d(N);
  for (size_t j = 0; j < N; ++j) {  // A's strict lower triangle becomes L
    double dj = A[j * N + j];
    for (size_t k = 0; k < j; ++k) dj = dj - A[k * N + j] * A[k * N + j] * d[k];
    if (!(dj > 0.0) || !std::isfinite(dj)) return false;
    d[j] = dj;
    for (size_t i = j + 1; i < N; ++i) {
      double s = A[j * N + i];
      for (size_t k = 0; k < j; ++k) s = s - A[k * N + i] * A[k * N + j] * d[k];
      A[j * N + i] = s / dj;
    }
  }
  x = rhs;
  for (size_t i = 0; i < N; ++i)
    for (size_t k = 0; k < i; ++k) x[i] = x[i] - A[k * N + i] * x[k];
  for (size_t i = 0; i < N; ++i) x[i] = x[i] / d[i];
  for (size_t i = N; i-- > 0;)
    for (size_t k = i + 1; k < N; ++k) x[i] = x[i] - A[i * N + k] * x[k];
  return true;
}

double norm(const std::vector<double>& v) {
  double s = 0.0;
  for (double a : v) s = s + a * a;
  return std::sqrt(s);
}

std::vector<double> pose_vector(const Graph& g) {
  std::vector<double> x(6 * g.poses.size());
  for (size_t i = 0; i < g.poses.size(); ++i) log6(g.poses[i], &x[6 * i]);
  return x;
}

// GlobalOptimizationLevenbergMarquardt::OptimizePoseGraph
void optimize(Graph& g, const o3s_global_optimization_criteria& cr, const o3s_global_optimization_option& opt, o3s_global_optimization_pass& st) {
  const size_t N = 6 * g.poses.size();
  const double w = line_process_weight(g, opt);
  std::memset(&st, 0, sizeof st);
  st.n_edges = (int32_t)g.edges.size();
  st.line_process_weight = w;
  double F = objective(g, w);
  st.residual_before = st.residual_after = F;
  std::vector<double> H, b, delta, Hlm;
  linear_system(g, H, b);
  double hmax = H[0];
  for (size_t i = 1; i < N; ++i) hmax = std::max(hmax, H[i * N + i]);
  double lambda = 1e-5 * hmax, ni = 2.0, rho = 0.0;
  auto right_term = [&] { return *std::max_element(b.begin(), b.end()) < cr.min_right_term; };
  if (right_term()) {
    st.stop_rule = O3S_PG_STOP_RIGHT_TERM;
    return;
  }
  std::vector<double> x = pose_vector(g);
  bool stop = false;
  for (int iter = 0; !stop; ++iter) {
    ++st.iterations;
    int lm_count = 0;
    do {
      Hlm = H;
      for (size_t i = 0; i < N; ++i) Hlm[i * N + i] = Hlm[i * N + i] + lambda;
      ++st.lm_trials;
      const bool solved = ldlt_solve(Hlm, N, b, delta);
      rho = -1.0;  // a system that could not be solved is a rejected trial
      if (solved && norm(delta) < cr.min_relative_increment * (norm(x) + cr.min_relative_increment)) {
        stop = true;
        st.stop_rule = O3S_PG_STOP_INCREMENT;
      }
      if (!stop) {
        if (solved) {
          Graph gn = g;
          for (size_t i = 0; i < gn.poses.size(); ++i) gn.poses[i] = mul(exp6(&delta[6 * i]), g.poses[i]);
          const double Fn = objective(gn, w);  // at the current confidences
          double den = 0.0;
          for (size_t i = 0; i < N; ++i) den = den + delta[i] * (lambda * delta[i] + b[i]);
          rho = (F - Fn) / (den + 1e-3);
          if (rho > 0.0) {
            if (F - Fn < cr.min_relative_residual_increment * F) {
              stop = true;
              st.stop_rule = O3S_PG_STOP_RESIDUAL_INCREMENT;
              break;
            }
            const double t = 2.0 * rho - 1.0;
            lambda = lambda * std::max(cr.lower_scale_factor, std::min(1.0 - t * t * t, cr.upper_scale_factor));
            ni = 2.0;
            g.poses = gn.poses;
            ++st.accepted;
            update_confidence(g, w);
            // (the objective the next trial is compared with is the accepted step's, at the confidences it was taken with)
            F = Fn;
            st.residual_after = F;
            x = pose_vector(g);
            linear_system(g, H, b);
            if (right_term()) {
              stop = true;
              st.stop_rule = O3S_PG_STOP_RIGHT_TERM;
              break;
            }
          }
        }
        if (!(rho > 0.0)) {
          lambda = lambda * ni;
          ni = ni * 2.0;
        }
      }
      ++lm_count;
      if (!stop && lm_count >= cr.max_iteration_lm) {
        stop = true;
        st.stop_rule = O3S_PG_STOP_MAX_ITERATION_LM;
      }
    } while (!(rho > 0.0 || stop));
    if (!stop && F < cr.min_residual) {
      stop = true;
      st.stop_rule = O3S_PG_STOP_RESIDUAL;
    }
    if (!stop && iter + 1 >= cr.max_iteration) {
      stop = true;
      st.stop_rule = O3S_PG_STOP_MAX_ITERATION;
    }
  }
}

bool graph_valid(int32_t n_nodes, const double* poses, int32_t n_edges, const o3s_pose_graph_edge* edges) {
  if (n_nodes <= 0 || !poses || n_edges < 0 || (n_edges > 0 && !edges)) return false;
  for (int32_t k = 0; k < n_edges; ++k) {
    const o3s_pose_graph_edge& ed = edges[k];
    if (ed.source < 0 || ed.source >= n_nodes || ed.target < 0 || ed.target >= n_nodes) return false;
    if (!ed.uncertain && ed.confidence != 1.0) return false;
  }
  return true;
}

Graph make_graph(int32_t n_nodes, const double* poses, int32_t n_edges, const o3s_pose_graph_edge* edges) {
  Graph g;
  g.poses.resize((size_t)n_nodes);
  for (int32_t i = 0; i < n_nodes; ++i) std::memcpy(g.poses[(size_t)i].m, poses + 16 * (size_t)i, sizeof(M4));
  g.edges.assign(edges, edges + n_edges);
  return g;
}

}  // namespace

extern "C" {

void o3s_global_optimization_defaults(o3s_global_optimization_criteria* c, o3s_global_optimization_option* o) {
  if (c) {
    c->max_iteration = 100;
    c->max_iteration_lm = 20;
    c->min_relative_increment = 1e-6;
    c->min_relative_residual_increment = 1e-6;
    c->min_right_term = 1e-6;
    c->min_residual = 1e-6;
    c->upper_scale_factor = 2.0 / 3.0;
    c->lower_scale_factor = 1.0 / 3.0;
  }
  if (o) {
    o->max_correspondence_distance = 0.075;
    o->edge_prune_threshold = 0.25;
    o->preference_loop_closure = 1.0;
    o->reference_node = -1;
  }
}

int o3s_global_optimization(int32_t n_nodes, double* poses, int32_t n_edges, o3s_pose_graph_edge* edges, int32_t* n_edges_out,
                            const o3s_global_optimization_criteria* criteria, const o3s_global_optimization_option* option,
                            o3s_global_optimization_stats* stats) {
  if (!criteria || !option || !graph_valid(n_nodes, poses, n_edges, edges)) return O3S_ERR_BAD_ARGUMENT;
  o3s_global_optimization_stats st;
  std::memset(&st, 0, sizeof st);
  // a copy is optimised; the edges the line process has switched off are dropped; the rest is optimised again, from the first
  // pass's poses and confidences
  Graph g = make_graph(n_nodes, poses, n_edges, edges);
  const M4 ref_before = (option->reference_node >= 0 && option->reference_node < n_nodes) ? g.poses[(size_t)option->reference_node] : M4{};
  optimize(g, *criteria, *option, st.pass[0]);
  Graph p;
  p.poses = g.poses;
  for (const auto& ed : g.edges)
    if (!ed.uncertain || ed.confidence > option->edge_prune_threshold) p.edges.push_back(ed);
  optimize(p, *criteria, *option, st.pass[1]);
  if (option->reference_node >= 0 && option->reference_node < n_nodes) {
    const M4 comp = mul(ref_before, inv_pose(p.poses[(size_t)option->reference_node]));
    for (auto& T : p.poses) T = mul(comp, T);
  }
  for (int32_t i = 0; i < n_nodes; ++i) std::memcpy(poses + 16 * (size_t)i, p.poses[(size_t)i].m, sizeof(M4));
  for (size_t k = 0; k < p.edges.size(); ++k) edges[k] = p.edges[k];
  if (n_edges_out) *n_edges_out = (int32_t)p.edges.size();
  if (stats) *stats = st;
  return O3S_OK;
}

int o3s_pose_graph_linearize(int32_t n_nodes, const double* poses, int32_t n_edges, const o3s_pose_graph_edge* edges,
                             const o3s_global_optimization_option* option, double* e, double* Js, double* Jt, double* H, double* b,
                             double* objective_out, double* line_process_weight_out) {
  if (!option || !graph_valid(n_nodes, poses, n_edges, edges)) return O3S_ERR_BAD_ARGUMENT;
  const Graph g = make_graph(n_nodes, poses, n_edges, edges);
  for (int32_t k = 0; k < n_edges; ++k) {
    double ee[6], js[36], jt[36];
    edge_terms(g, g.edges[(size_t)k], ee, js, jt);
    if (e) std::memcpy(e + 6 * (size_t)k, ee, sizeof ee);
    if (Js) std::memcpy(Js + 36 * (size_t)k, js, sizeof js);
    if (Jt) std::memcpy(Jt + 36 * (size_t)k, jt, sizeof jt);
  }
  if (H || b) {
    std::vector<double> Hv, bv;
    linear_system(g, Hv, bv);
    if (H) std::memcpy(H, Hv.data(), Hv.size() * sizeof(double));
    if (b) std::memcpy(b, bv.data(), bv.size() * sizeof(double));
  }
  const double w = line_process_weight(g, *option);
  if (objective_out) *objective_out = objective(g, w);
  if (line_process_weight_out) *line_process_weight_out = w;
  return O3S_OK;
}

}  // extern "C"
