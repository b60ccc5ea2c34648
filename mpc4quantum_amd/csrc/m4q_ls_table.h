// m4q_ls_table.h - the weight table of the node-per-lane line search (line_search_tl_nodes, m4q_mpc.h): the index arithmetic that does
// not depend on the pass, as a map only.  Host and device, no includes: m4q_mpc.h reads by it, m4q_kernels.hip sizes the workgroup's LDS and builds
// the table by it, and tests/test_ls_table_host.py compiles it for the CPU and replays every index of every lane.
//
// The line search weighs slot (a, b) of node t of the d x d state with the diagonal cost of Z slot q, where
// q counts [Re x_0 (T + 1 nodes) | Re x_1 | .. | Re x_{n-1} | Im x_0 | ..] and the staged weights are w = [wq (2 n) | wqf (2 n)]:
// block q / (2 n) of Z takes wq, the last block (== T) wqf.  That is two divisions by 2 n per weight and fifteen weights per node -
// of numbers that are fixed for the launch.  The table W[t][s], t = 0..T, holds per node the n values the loop uses, as it formed them:
//     s < n - d:  the s-th off-diagonal slot, c = a d + b = offdiag_c(d, s):   0.5 * (weight(q of (a, b)) + weight(q of (b, a)))
//                 (antisymmetric coordinates, a > b, live in the imaginary halves: both q are n (T + 1) further)
//     s >= n - d: diagonal slot a = s - (n - d):                              weight((a d + a)(T + 1) + t)
// A lane reads node t's row at byte t * 8 n, the slot an immediate.  At n = 9 the pitch is 72 B = 18 dwords: the sixteen lanes of a
// row (t = jj + 16 trip) fall on banks 18 jj mod 64 and the next - sixteen different pairs - and the four rows of the wavefront read
// the same addresses (a broadcast).
// The table takes what the workgroup's budget leaves (capacity()); a horizon with more nodes than that runs without it (tabled()).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M4Q_LS_HD __host__ __device__
#else
#define M4Q_LS_HD
#endif

namespace m4q {
namespace ls_table {

constexpr int LDS_BUDGET = 20480;          // bytes of a workgroup that leave eight of them on a CU

// ---- the staged weights
// index into w = [wq | wqf] of the weight of Z slot q
M4Q_LS_HD constexpr int weight_index(int nx, int T, int q) {
  return (q / (2 * nx) == T ? 2 * nx : 0) + (q - (q / (2 * nx)) * (2 * nx));
}

// ---- the table
M4Q_LS_HD constexpr int offdiag_c(int d, int i) { return i + 1 + i / d; }                 // c = a d + b of the i-th off-diagonal slot
M4Q_LS_HD constexpr int offdiag_slot(int d, int c) { return c - 1 - c / (d + 1); }        // ... and back (c not a multiple of d + 1)
M4Q_LS_HD constexpr int diag_slot(int nx, int d, int a) { return nx - d + a; }
M4Q_LS_HD constexpr int pitch_bytes(int nx) { return 8 * nx; }
M4Q_LS_HD constexpr int index(int nx, int t, int s) { return t * nx + s; }                // in doubles
M4Q_LS_HD constexpr int bytes(int nx, int nodes) { return nodes * pitch_bytes(nx); }
// nodes that fit behind `used` bytes of the workgroup
M4Q_LS_HD constexpr int capacity(int nx, int used) { return used < LDS_BUDGET ? (LDS_BUDGET - used) / pitch_bytes(nx) : 0; }
M4Q_LS_HD constexpr bool tabled(int T, int nodes) { return T + 1 <= nodes; }
// the node a lane reads in the trip that starts at t0 = jj + 16 trip: its own, a lane past the end the last one
M4Q_LS_HD constexpr int read_node(int T, int t) { return t <= T ? t : T; }

// the two Z slots of off-diagonal coordinate c at node t, and the one of diagonal slot a
M4Q_LS_HD constexpr int q_offdiag(int nx, int d, int T, int t, int c) {
  return c * (T + 1) + t + (c / d > c - (c / d) * d ? nx * (T + 1) : 0);
}
M4Q_LS_HD constexpr int q_offdiag_mirror(int nx, int d, int T, int t, int c) {
  return ((c - (c / d) * d) * d + c / d) * (T + 1) + t + (c / d > c - (c / d) * d ? nx * (T + 1) : 0);
}
M4Q_LS_HD constexpr int q_diag(int d, int T, int t, int a) { return (a * d + a) * (T + 1) + t; }

// entry (t, s) from the staged weights w = [wq | wqf]
template <class W>
M4Q_LS_HD inline double entry(const W* w, int nx, int d, int T, int t, int s) {
  if (s < nx - d) {
    const int c = offdiag_c(d, s);
    return 0.5 * (w[weight_index(nx, T, q_offdiag(nx, d, T, t, c))] + w[weight_index(nx, T, q_offdiag_mirror(nx, d, T, t, c))]);
  }
  return w[weight_index(nx, T, q_diag(d, T, t, s - (nx - d)))];
}

}  // namespace ls_table
}  // namespace m4q
