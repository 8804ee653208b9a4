// o3s_pose.hpp — the 4x4 pose arithmetic the header-only drivers share (o3s_mapper.hpp, o3s_odometry.hpp).
// 4x4 matrices are column-major doubles (Eigen::Matrix4d::data()).  Isometry products / inverses are restated as plain
// k = 0..3 accumulations (Eigen is not part of the tree: its evaluation order is not pinned).
#pragma once

namespace o3s {

struct Mat4 {
  double m[16];
  static Mat4 identity() {
    Mat4 r{};
    r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0;
    return r;
  }
  double& operator()(int r, int c) { return m[c * 4 + r]; }
  double operator()(int r, int c) const { return m[c * 4 + r]; }
};
inline Mat4 mul(const Mat4& A, const Mat4& B) {
  Mat4 C{};
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
// Eigen::Isometry3d::inverse(): [R^T, -R^T t]
inline Mat4 inverse_isometry(const Mat4& T) {
  Mat4 R = Mat4::identity();
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R(r, c) = T(c, r);
  for (int r = 0; r < 3; ++r) {
    double s = R(r, 0) * T(0, 3);
    s = s + R(r, 1) * T(1, 3);
    s = s + R(r, 2) * T(2, 3);
    R(r, 3) = -s;
  }
  return R;
}

}  // namespace o3s
