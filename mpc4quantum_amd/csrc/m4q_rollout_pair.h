// m4q_rollout_pair.h - the pair form of the clipped forward rollout (rollout_forward_pair, m4q_mpc.h): the map only - which half
// of a 16-lane row owns a horizon index, which indices a lane loads in trip p, where and whether it stores.
// Host and device, no includes: the kernel addresses by it and tests/test_rollout_pair_host.py compiles it for the CPU and replays
// every load and store of both halves.
//
// A row rolls a state of 8 coordinates: lane = 8 half + j2.  Trip p takes the two indices 2 p (lower half) and 2 p + 1 (upper
// half).  Half t % 2 holds everything of index t that depends on the guess alone - u_g(t), the node x_g(t), ubar_t, the affine
// gain entries k_t - and therefore row j2 of A_t, of B_t and Delta_t[j2]; x_{t+1} is produced there.  x_t itself lives in the OTHER
// half, 1 - t % 2, and so does row j2 of the gain K_t, which multiplies it.  x_0 starts in the upper half.
// An odd T leaves the upper half's last index, T, clamped in its loads and off in its stores.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M4Q_RPAIR_HD __host__ __device__
#else
#define M4Q_RPAIR_HD
#endif

namespace m4q {
namespace rollout_pair {

constexpr int HALF = 8;                                                             // lanes per half = state coordinates

M4Q_RPAIR_HD constexpr int half_of_lane(int jj) { return jj >> 3; }
M4Q_RPAIR_HD constexpr int coord_of_lane(int jj) { return jj & 7; }
M4Q_RPAIR_HD constexpr int owner_half(int t) { return t & 1; }                      // guess operands of t, and x_{t+1}
M4Q_RPAIR_HD constexpr int state_half(int t) { return 1 - (t & 1); }                // x_t and the gain row K_t[j2]
M4Q_RPAIR_HD constexpr int first_source_lane(int t) { return HALF * state_half(t); }   // the DPP sums of index t read lanes from here

M4Q_RPAIR_HD constexpr int full_pairs(int T) { return T >> 1; }                      // trips that roll two indices
M4Q_RPAIR_HD constexpr bool odd_tail(int T) { return (T & 1) != 0; }                 // ... and one more for index T - 1 alone
M4Q_RPAIR_HD constexpr int trips(int T) { return (T + 1) >> 1; }

M4Q_RPAIR_HD constexpr int own_index(int p, int half) { return 2 * p + half; }      // the index a half rolls in trip p (may be T: off)
M4Q_RPAIR_HD constexpr int clamped(int T, int t) { return t < T - 1 ? t : T - 1; }
// what a lane loads for trip p: u_g, the node, ubar and k of its own index; the gain row of the index whose state it holds
M4Q_RPAIR_HD constexpr int load_index(int T, int p, int half) { return clamped(T, own_index(p, half)); }
M4Q_RPAIR_HD constexpr int gain_index(int T, int p, int half) { return clamped(T, 2 * p + 1 - half); }

// stores of index t (x_{t+1} and u_t), shift = the solution goes into the next step's guess one node down
M4Q_RPAIR_HD constexpr bool index_live(int T, int t) { return t < T; }
M4Q_RPAIR_HD constexpr int node_slot(int t, bool shift) { return shift ? t : t + 1; }
M4Q_RPAIR_HD constexpr bool ctrl_stored(int t, bool shift) { return !shift || t >= 1; }      // (a shifting row's u_0 has no slot)
M4Q_RPAIR_HD constexpr int ctrl_slot(int t, bool shift) { return shift ? t - 1 : t; }
// a shifting row repeats its last column: x_T also at node T, u_{T-1} also at slot T - 1, by the half that owns index T - 1
M4Q_RPAIR_HD constexpr bool repeats(int T, int t, bool shift) { return shift && t == T - 1; }
M4Q_RPAIR_HD constexpr int repeat_node_slot(int T) { return T; }
M4Q_RPAIR_HD constexpr int repeat_ctrl_slot(int T) { return T - 1; }
// x_0 itself is node 0 of a row that does not shift
M4Q_RPAIR_HD constexpr bool stores_x0(int half, bool shift) { return !shift && half == 0; }

}  // namespace rollout_pair
}  // namespace m4q
