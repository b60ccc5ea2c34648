// m4q_tile_opnd.h - the LDS image through which the clipped tile sweep (m4q_tile3.h) spreads the operands of a block of four horizon
// indices to the lanes that use them: the map only - tile pitch, tile order, the per-lane byte addresses and the immediate offsets.
// Host and device, no includes: m4q_tile3.h reads and writes by it, m4q_kernels.hip sizes the workgroup's LDS by it, and
// tests/test_tile_operands_host.py compiles it for the CPU and replays every read of every lane.
//
// A tile is the 64 doubles of one wavefront register, LANE-LINEAR: lane = 16 r + 4 mb + q (m4q_tile.h) stores its double at byte
// 8 lane of the tile - one ds_write_b64 of the whole register.  Column q of the block's tiles holds time tb - q.  Tiles lie PITCH
// bytes apart, in the order
//     group K (K < NT):   BT[0][K] .. BT[NU - 1][K] | CT[K] | zero          NU + 2 tiles
//     then                UG[0] .. UG[NU - 1]                                 the controls of time tb - q, as tiles
// Reads, one ds_read_b64 each, the horizon index j (time tb - j) an immediate:
//   * W[K] = [B | c | 0] of index j: lane (r, mb, q) takes element (r, mb, j) of tile min(q, NU + 1) of group K - column q of W is
//     column j of the q-th tile;
//   * b[s][K], c[K], u_g[p] of index j, replicated over q: element (r, mb, j) of the tile, the same address in the four q (an LDS
//     broadcast).
// PITCH = 520 bytes = 130 dwords = 2 mod 64: a 64-bit read is served in two halves of 32 lanes, a lane takes banks (a / 4) mod 64
// and the next; in a half the W read touches banks 2 q + 8 mb + 32 (r & 1) + 2 j (+ 1): 32 lanes, 64 different banks.  At a
// pitch of 512 the four q of a quad would meet on one bank pair.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M4Q_OPND_HD __host__ __device__
#else
#define M4Q_OPND_HD
#endif

namespace m4q {
namespace tile_opnd {

constexpr int PITCH = 520;                                                          // bytes from tile to tile

M4Q_OPND_HD constexpr int group_tiles(int nu) { return nu + 2; }
M4Q_OPND_HD constexpr int tile_b(int nu, int s, int K) { return K * group_tiles(nu) + s; }          // BT[s][K]
M4Q_OPND_HD constexpr int tile_c(int nu, int K) { return K * group_tiles(nu) + nu; }                 // CT[K]
M4Q_OPND_HD constexpr int tile_zero(int nu, int K) { return K * group_tiles(nu) + nu + 1; }
M4Q_OPND_HD constexpr int tile_u(int nu, int nt, int p) { return nt * group_tiles(nu) + p; }         // UG[p]
M4Q_OPND_HD constexpr int tiles(int nu, int nt) { return nt * group_tiles(nu) + nu; }
M4Q_OPND_HD constexpr int bytes(int nu, int nt) { return tiles(nu, nt) * PITCH; }

// per-lane byte addresses from the start of the image (set up once per sweep) ...
M4Q_OPND_HD constexpr int write_addr(int lane) { return 8 * lane; }
M4Q_OPND_HD constexpr int w_addr(int nu, int lane) { return ((lane & 3) < nu + 1 ? (lane & 3) : nu + 1) * PITCH + 8 * (lane & ~3); }
M4Q_OPND_HD constexpr int bcast_addr(int lane) { return 8 * (lane & ~3); }
// ... and the immediate offsets added to them
M4Q_OPND_HD constexpr int write_imm(int tile) { return tile * PITCH; }
M4Q_OPND_HD constexpr int w_imm(int nu, int K, int j) { return tile_b(nu, 0, K) * PITCH + 8 * j; }
M4Q_OPND_HD constexpr int bcast_imm(int tile, int j) { return tile * PITCH + 8 * j; }

}  // namespace tile_opnd
}  // namespace m4q
