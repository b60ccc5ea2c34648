// m4q_robust_host.h - the host side of m4q_plant_robust_batch: the projected L-BFGS direction, the candidates of the line search and
// the decision, taken between two launches.  mpc4quantum_amd/plant_robust.py (_project, _absorb, _direction, _candidates, _pick) is
// the definition; what is here repeats it in the same order of operations: every dot product is a sequential loop over (t, k)
// row-major from 0.0, every product is rounded before it is added (floating-point contraction is off in this header).
// Plain C++17, no HIP: tests/robust_host/direction_driver.cpp compiles it for the CPU with the sanitizers on.
#pragma once
#include <cmath>
#include <cstddef>
#include <deque>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

namespace m4q {
namespace robust {

using Vec = std::vector<double>;
constexpr double CURVATURE = 1e-12;

struct Pair {
  Vec s, y;
};

inline double dot(const Vec& a, const Vec& b) {
  double acc = 0.0;
  for (size_t i = 0; i < a.size(); ++i) {
    const double prod = a[i] * b[i];
    acc = acc + prod;
  }
  return acc;
}

// min(max(w, -sat), sat) that lets a NaN through, as the device's clip does
inline double clip(double w, double sat) {
  w = w < -sat ? -sat : w;
  w = w > sat ? sat : w;
  return w;
}

// The iterate and what the direction needs of it.  U, g: [N m]; the memory holds at most mem pairs, newest last
struct State {
  int mem = 0;
  double sat = 0.0, step0 = 0.0;
  Vec U, g;
  std::deque<Pair> pairs;
  bool pending = false;       // a step was accepted: s_pend = U_new - U_old, g_old the gradient it left
  Vec s_pend, g_old;
  // step 2
  std::vector<char> active;
  Vec pg;
  double gmax = 0.0;
  // step 4
  Vec p;
};

// step 2: active, pg, gmax (a sequential maximum from 0.0 in which a NaN sticks)
inline void project(State& st) {
  const size_t nm = st.U.size();
  st.active.assign(nm, 0);
  st.pg.assign(nm, 0.0);
  st.gmax = 0.0;
  for (size_t i = 0; i < nm; ++i) {
    const bool act = (st.U[i] == st.sat && st.g[i] < 0) || (st.U[i] == -st.sat && st.g[i] > 0);
    st.active[i] = act ? 1 : 0;
    st.pg[i] = act ? 0.0 : st.g[i];
    const double a = std::fabs(st.pg[i]);
    if (a > st.gmax || a != a) st.gmax = a;
  }
}

// step 3: the pending pair joins the memory if it passes the curvature test; the oldest beyond mem leaves
inline void absorb(State& st) {
  if (!st.pending) return;
  st.pending = false;
  Pair pr;
  pr.s = st.s_pend;
  pr.y.resize(st.g.size());
  for (size_t i = 0; i < st.g.size(); ++i) pr.y[i] = st.g[i] - st.g_old[i];
  const double sy = dot(pr.s, pr.y), ss = dot(pr.s, pr.s), yy = dot(pr.y, pr.y);
  if (sy > CURVATURE * std::sqrt(ss * yy)) {
    st.pairs.push_back(std::move(pr));
    while ((int)st.pairs.size() > st.mem) st.pairs.pop_front();
  }
}

inline void steepest(State& st) {
  const double c = st.step0 / st.gmax;
  st.p.resize(st.pg.size());
  for (size_t i = 0; i < st.pg.size(); ++i) st.p[i] = -(c * st.pg[i]);
}

// step 4: the direction p; clears the memory when the quasi-Newton direction is not one of descent
inline void direction(State& st) {
  if (st.pairs.empty()) {
    steepest(st);
    return;
  }
  const size_t nm = st.pg.size(), np = st.pairs.size();
  Vec v = st.pg, rho(np), al(np);
  for (size_t q = np; q-- > 0;) {                       // newest to oldest
    const Pair& pr = st.pairs[q];
    rho[q] = 1.0 / dot(pr.s, pr.y);
    al[q] = rho[q] * dot(pr.s, v);
    for (size_t i = 0; i < nm; ++i) {
      const double prod = al[q] * pr.y[i];
      v[i] = v[i] - prod;
    }
  }
  const Pair& last = st.pairs.back();
  const double scale = dot(last.s, last.y) / dot(last.y, last.y);
  Vec r(nm);
  for (size_t i = 0; i < nm; ++i) r[i] = scale * v[i];
  for (size_t q = 0; q < np; ++q) {                     // oldest to newest
    const Pair& pr = st.pairs[q];
    const double c = al[q] - rho[q] * dot(pr.y, r);
    for (size_t i = 0; i < nm; ++i) {
      const double prod = c * pr.s[i];
      r[i] = r[i] + prod;
    }
  }
  st.p.resize(nm);
  for (size_t i = 0; i < nm; ++i) st.p[i] = st.active[i] ? 0.0 : -r[i];
  if (!(dot(st.p, st.g) < 0)) {
    st.pairs.clear();
    steepest(st);
  }
}

// step 5: candidate j = clip(U + 2^-j p) into out [N m] (2^-j p is exact)
inline void candidate(const State& st, int j, double* out) {
  const double a = std::ldexp(1.0, -j);
  for (size_t i = 0; i < st.U.size(); ++i) {
    const double step = a * st.p[i];
    out[i] = clip(st.U[i] + step, st.sat);
  }
}

// step 6: the smallest j attaining the least finite F_j, or -1
inline int pick(const double* F, int steps) {
  int best = -1;
  for (int j = 0; j < steps; ++j)
    if (F[j] - F[j] == 0.0 && (best < 0 || F[j] < F[best])) best = j;
  return best;
}

// step 7: the accepted candidate becomes the iterate; the pair it will form waits for the next gradient
inline void accept(State& st, const double* cand) {
  const size_t nm = st.U.size();
  st.s_pend.resize(nm);
  for (size_t i = 0; i < nm; ++i) st.s_pend[i] = cand[i] - st.U[i];
  st.g_old = st.g;
  st.U.assign(cand, cand + nm);
  st.pending = true;
}

}  // namespace robust
}  // namespace m4q
