// m4q_lift.h - the host code that decides which arithmetic path a session may run: the lift of its inputs to the Hermitian operator
// basis and to the traceless coordinates, and the thresholds under which an input counts as real / as leaving the trace coordinate
// alone.  Host only, standard library only: m4q_capi.hip uses it, and tests/test_lift_host.py compiles it for the CPU against NumPy.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <vector>

#include "m4q_paths.h"

namespace m4q {
namespace lift {

// ---- Hermitian operator basis of the real path (same convention as csrc/m4q_mpc.h) ----------------
// slot c = a*d + b:  a == b: rho_aa;  a < b: sqrt2 Re rho_ab;  a > b: sqrt2 Im rho_ab.
// Column c of the unitary W (x = W r) has at most two entries; (W^H v)_c and (M W)_{.,c} cost O(1).
struct HermBasis {
  int d, n;
  explicit HermBasis(int d_) : d(d_), n(d_ * d_) {}
  // out = W^H v  (complex n-vector, stride 1)
  void lift_vec(const std::complex<double>* v, std::complex<double>* out) const {
    const double rs = 0.70710678118654752440;
    const std::complex<double> I(0, 1);
    for (int a = 0; a < d; ++a)
      for (int b = 0; b < d; ++b) {
        const int c = a * d + b, ct = b * d + a;
        if (a == b) out[c] = v[c];
        else if (a < b) out[c] = (v[c] + v[ct]) * rs;            // conj(1/sqrt2) (x_ab + x_ba)
        else out[c] = (v[c] - v[ct]) * (-I * rs);                // conj(+i/sqrt2) x_ab + conj(-i/sqrt2) x_ba
      }
  }
  // M (n x n, row-major, leading dimension ld) -> W^H M W, written to out (n x n, leading dimension ldo)
  void lift_mat(const std::complex<double>* M, long ld, std::complex<double>* out, long ldo) const {
    const double rs = 0.70710678118654752440;
    const std::complex<double> I(0, 1);
    std::vector<std::complex<double>> Y((size_t)n * n);
    for (int i = 0; i < n; ++i)
      for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b) {
          const int c = a * d + b, ct = b * d + a;
          const std::complex<double> m1 = M[i * ld + c], m2 = M[i * ld + ct];
          if (a == b) Y[(size_t)i * n + c] = m1;
          else if (a < b) Y[(size_t)i * n + c] = (m1 + m2) * rs;
          else Y[(size_t)i * n + c] = (m1 - m2) * (I * rs);      // W[(a,b),c] = +i/sqrt2, W[(b,a),c] = -i/sqrt2
        }
    std::vector<std::complex<double>> col(n), lifted(n);
    for (int j = 0; j < n; ++j) {
      for (int i = 0; i < n; ++i) col[i] = Y[(size_t)i * n + j];
      lift_vec(col.data(), lifted.data());
      for (int i = 0; i < n; ++i) out[i * ldo + j] = lifted[i];
    }
  }
};

// real part of a lifted array + the size of what was dropped, relative to the array's scale
struct LiftStat {
  double max_im = 0.0, max_abs = 0.0;
  void see(std::complex<double> v) {
    max_im = std::max(max_im, std::fabs(v.imag()));
    max_abs = std::max(max_abs, std::abs(v));
  }
  bool real_enough() const { return max_im <= 1e-13 * std::max(1.0, max_abs); }
};

// ---- traceless coordinates (COORDS_TRACELESS; csrc/m4q_mpc.h): the diagonal slots (a, a) of the Hermitian basis rotated by the orthogonal
// O[a][0] = 1/sqrt(d), O[a][l] = 1/sqrt(l(l+1)) (a < l), -l/sqrt(l(l+1)) (a == l), 0 (a > l); slot (0, 0) becomes the trace
// coordinate and is dropped when the model leaves it alone.  Works on the REAL arrays the Hermitian lift produced.
struct Traceless {
  int d, n;
  std::vector<double> O;                 // n x n: identity off the diagonal slots
  explicit Traceless(int d_) : d(d_), n(d_ * d_), O((size_t)d_ * d_ * d_ * d_, 0.0) {
    for (int c = 0; c < n; ++c) O[(size_t)c * n + c] = 1.0;
    for (int a = 0; a < d; ++a)
      for (int l = 0; l < d; ++l) {
        double v;
        if (l == 0) v = 1.0 / std::sqrt((double)d);
        else v = a < l ? 1.0 / std::sqrt((double)l * (l + 1)) : (a == l ? -(double)l / std::sqrt((double)l * (l + 1)) : 0.0);
        O[(size_t)(a * d + a) * n + (l * d + l)] = v;
      }
  }
  // r (n) -> O^T r: out[0] = trace coordinate, out[1..n) = traceless coordinates
  void vec(const double* r, double* out) const {
    for (int c = 0; c < n; ++c) {
      double acc = 0.0;
      for (int k = 0; k < n; ++k) acc += O[(size_t)k * n + c] * r[k];
      out[c] = acc;
    }
  }
  // M (n x n, leading dimension ld) -> O^T M O (n x n, dense, into out)
  void mat(const double* M, long ld, double* out) const {
    std::vector<double> Y((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k) {
        const double m = M[i * ld + k];
        if (m != 0.0)
          for (int c = 0; c < n; ++c) Y[(size_t)i * n + c] += m * O[(size_t)k * n + c];
      }
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += O[(size_t)i * n + r] * Y[(size_t)i * n + c];
        out[(size_t)r * n + c] = acc;
      }
  }
};

// how well the trace coordinate decouples: largest entry of row 0 / column 0 off what a decoupled block must hold
struct DecoupleStat {
  double worst = 0.0, scale = 0.0;
  void see_block(const double* M, int n, bool identity_block) {     // M = O^T block O
    for (int k = 0; k < n; ++k) {
      const double want = (k == 0 && identity_block) ? 1.0 : 0.0;
      worst = std::max(worst, std::fabs(M[k] - want));                       // row 0
      worst = std::max(worst, std::fabs(M[(size_t)k * n] - want));           // column 0
    }
    for (int e = 0; e < n * n; ++e) scale = std::max(scale, std::fabs(M[e]));
  }
  bool ok() const { return worst <= 1e-12 * std::max(1.0, scale); }
};

// An input on the real coordinate systems, on the host.  [COORDS_HERM]: the real part of its lift to the Hermitian basis, ok when
// the imaginary part dropped was negligible (LiftStat).  [COORDS_TRACELESS], when asked for and the Hermitian lift is ok: the same
// on the traceless coordinates, ok when the trace coordinate decouples (DecoupleStat); tau: the range of that coordinate (vectors).
struct Lift {
  std::vector<double> v[COORDS_TRACELESS + 1];
  bool ok[COORDS_TRACELESS + 1] = {};
  double tau[2] = {0, 0};
};

// count rows of nblk n x n complex blocks side by side (row-major: block p of a row occupies columns [p*n, (p+1)*n)).
// block0_identity: block 0 must carry the trace coordinate through unchanged (models [A | N_1 ..]); every other block must not
// touch it.
inline Lift lift_blocks(int d, const std::complex<double>* src, size_t count, int nblk, bool block0_identity, bool traceless) {
  const HermBasis hb(d);
  const int n = hb.n, ns = n - 1;
  const long ld = (long)n * nblk, lds = (long)ns * nblk;
  Lift L;
  std::vector<double>& out = L.v[COORDS_HERM];
  out.resize(count * n * ld);
  LiftStat st;
  std::vector<std::complex<double>> tmp((size_t)n * n);
  for (size_t it = 0; it < count; ++it)
    for (int p = 0; p < nblk; ++p) {
      hb.lift_mat(src + it * n * ld + (long)p * n, ld, tmp.data(), n);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          st.see(tmp[(size_t)i * n + j]);
          out[it * n * ld + i * ld + (long)p * n + j] = tmp[(size_t)i * n + j].real();
        }
    }
  L.ok[COORDS_HERM] = st.real_enough();
  if (!traceless || !L.ok[COORDS_HERM]) return L;
  const Traceless tl(d);
  std::vector<double>& tout = L.v[COORDS_TRACELESS];
  tout.resize(count * ns * lds);
  std::vector<double> rot((size_t)n * n);
  DecoupleStat dc;
  for (size_t it = 0; it < count; ++it)
    for (int p = 0; p < nblk; ++p) {
      tl.mat(out.data() + it * n * ld + (long)p * n, ld, rot.data());
      dc.see_block(rot.data(), n, block0_identity && p == 0);
      for (int i = 0; i < ns; ++i)
        for (int j = 0; j < ns; ++j) tout[it * ns * lds + i * lds + (long)p * ns + j] = rot[(size_t)(1 + i) * n + 1 + j];
    }
  L.ok[COORDS_TRACELESS] = dc.ok();
  return L;
}

// count complex n-vectors
inline Lift lift_vectors(int d, const std::complex<double>* src, size_t count, bool traceless) {
  const HermBasis hb(d);
  const int n = hb.n, ns = n - 1;
  Lift L;
  std::vector<double>& out = L.v[COORDS_HERM];
  out.resize(count * n);
  LiftStat st;
  std::vector<std::complex<double>> tmp(n);
  for (size_t it = 0; it < count; ++it) {
    hb.lift_vec(src + it * n, tmp.data());
    for (int i = 0; i < n; ++i) { st.see(tmp[i]); out[it * n + i] = tmp[i].real(); }
  }
  L.ok[COORDS_HERM] = st.real_enough();
  if (!traceless || !L.ok[COORDS_HERM]) return L;
  const Traceless tl(d);
  std::vector<double>& tout = L.v[COORDS_TRACELESS];
  tout.resize(count * ns);
  std::vector<double> rot(n);
  for (size_t it = 0; it < count; ++it) {
    tl.vec(out.data() + it * n, rot.data());
    for (int i = 0; i < ns; ++i) tout[it * ns + i] = rot[1 + i];
    L.tau[0] = it ? std::min(L.tau[0], rot[0]) : rot[0];
    L.tau[1] = it ? std::max(L.tau[1], rot[0]) : rot[0];
  }
  L.ok[COORDS_TRACELESS] = true;
  return L;
}

}  // namespace lift
}  // namespace m4q
