// m4q_paths.h - the arithmetic paths of the closed loop and the coordinate systems their inputs are held in.  No include of its
// own: shared by the kernel argument blocks (m4q_args.h) and the host-only lift code (m4q_lift.h).
#pragma once

namespace m4q {

// Arithmetic paths of the closed loop (m4q_session_path returns these values; session.path_detail() indexes by them)
enum Path : int {
  PATH_COMPLEX = 0,     // complex recursion on vec(rho): any model
  PATH_REAL = 1,        // real recursion in the Hermitian operator basis (n coordinates)
  PATH_TRACELESS = 2,   // real recursion on the n - 1 traceless coordinates
  PATH_TILE = 3,        // PATH_TRACELESS with the backward sweep (clipped) / the pinned sweep (exact) on matrix-core tiles
  PATH_SG = 4,          // PATH_TRACELESS, clipped solve, on shared generators instead of per-member models
};
// Coordinate systems the recursion's inputs are held in
enum Coords : int { COORDS_COMPLEX = 0, COORDS_HERM = 1, COORDS_TRACELESS = 2 };

}  // namespace m4q
