// m4q_kernels.hip - kernels for ONE problem shape, selected at compile time:
//     hipcc --offload-arch=gfx950 -DM4Q_NX=9 -DM4Q_NU=2 -DM4Q_ORDER=1 -c m4q_kernels.hip
// One wavefront per workgroup; each of its four DPP rows runs one MPC instance (m4q_device.h).
// The persistent kernel strides over instance quads, so a fixed pool of per-row workspace stays
// cache resident whatever the ensemble size.
#define M4Q_KERNEL_TU 1
#include "m4q_args.h"
#include "m4q_mpc.h"
#include "m4q_feedback.h"
#include "m4q_fit.h"
#include "m4q_fit_qr.h"
#include "m4q_online.h"
#include "m4q_grad.h"
#include "m4q_plant_param.h"
#include "m4q_plant_lin.h"
#include "m4q_plant_qp.h"
#include "m4q_noise.h"
#include "m4q_observe.h"
#include "m4q_tile3.h"

#ifndef M4Q_NX
#error "compile with -DM4Q_NX -DM4Q_NU -DM4Q_ORDER"
#endif
// Two objects per shape (build.py): the core object (libm4q_hip.so) holds every kernel except the closed-loop kernels with the
// GENERATOR plant (x+ = expm(dt (L0 + sum u_k L_k)) x on n x n operators: QExperiment with collapse operators, LExperiment - outside
// SURVEY section 8, and the largest objects of the library: up to 1 KB of scratch per lane); those are compiled with
// -DM4Q_VARIANT_GEN into libm4q_hip_gen.so, which m4q_capi.hip loads on the first session that asks for that plant.
#if defined(M4Q_PLANT_ONLY) || defined(M4Q_VARIANT_GEN)
#define M4Q_NO_AUX 1
#endif

#define M4Q_CAT_(a, b, c, d) a##b##_##c##_##d
#define M4Q_CAT(a, b, c, d) M4Q_CAT_(a, b, c, d)

namespace m4q {
// every shape lives in its own namespace: the shapes are linked into one library
namespace M4Q_CAT(shape_, M4Q_NX, M4Q_NU, M4Q_ORDER) {

constexpr int NX = M4Q_NX;
constexpr int NU = M4Q_NU;
constexpr int ORDER = M4Q_ORDER;
// n = d*d for vectorised density matrices.  A model space that is not a square (n = 8: two reduced qubit states,
// experiment.py:238-306) has no device plant and no Hermitian-basis path: only the complex QP machinery is built.
constexpr int DD = (NX == 4) ? 2 : (NX == 9) ? 3 : (NX == 16) ? 4 : 1;
constexpr bool SQUARE = DD * DD == NX;
// n = d^4: a process vector vec_r(U (x) U^*) of a d x d unitary (gate synthesis, QSynthesis).  The process plant is built on the
// complex path alone: V (x) V^* acting on M does not keep M Hermitian as a d^2 x d^2 matrix, so no Hermitian-basis path applies.
constexpr int DQ = fourth_root(NX);
constexpr bool QUARTIC = DQ > 0;
constexpr int NP = PowTab<NU, ORDER>::NP;
constexpr int PITCH = ModelPitch<NX>::value;
constexpr int MODEL_ELEMS = (1 + NP) * NX * PITCH;        // per instance, elements (of S) in LDS
// the traceless path (m4q_mpc.h) runs the recursion on NX - 1 coordinates; everything it stages is no larger than the above
constexpr int SCRATCH_ELEMS = (SQUARE ? DD * DD : 0) + 2 * NX;   // plant / basis-change scratch per instance (complex)
constexpr int ROWS = 4;                                    // instances per wavefront
// (what the timing-only ablations of round 5 bound: profiles/r05_ab_experiments.txt)
// the backward sweep on matrix-core tiles (m4q_tile3.h) is built where it is the faster form: d = 2, 3 (3 and 8 traceless coordinates)
// with an order-1 library.  At d = 4 (15 coordinates = 4 x 4 tiles) it does not fit the register file (543 spilled VGPRs, 505 against
// 71 ms on config 4) and full DPP rows leave nothing to gain; the host asks m4q_shape_*()->has_tile.
constexpr bool HAS_TILE = SQUARE && ORDER == 1 && NX - 1 <= 8;
// the shared-generator form of the clipped traceless kernel (FusedProv<..., SG>, m4q_mpc.h: one set of N_k = dt L_k per workgroup, per
// member only A_i = I + s_i0 dt L_0 and its scales) is built where the per-member models are what keeps the kernel at one wavefront
// per SIMD: d = 4 (28.8 KB of models per workgroup against 12.6).  Sessions whose models came from m4q_session_build_models with
// shared generators run it (PATH_SG); the host asks m4q_shape_*()->has_sg.
constexpr bool HAS_SG = SQUARE && ORDER == 1 && NX == 16;

// register budget: waves per SIMD the kernels are compiled for (512 / budget VGPRs per lane).  d = 2 was compiled for four until the
// end of round 3: at 128 registers every d = 2 closed-loop kernel spilled (59-372 VGPRs), and its launches are chains of
// dependent passes that a third and fourth wavefront do not shorten: config 2 5.3 -> 4.2 ms at two (131,072 members: 23.6 -> 19.5 ms).
// The same on the complex and the real path, and in the exact mode.
constexpr int WAVES = NX <= 9 ? 2 : 1;
#define M4Q_OCC __attribute__((amdgpu_waves_per_eu(WAVES, 8)))

extern __shared__ __align__(16) unsigned char m4q_lds_raw[];

// copy one instance's model (DMDc.A layout, n x n(1+P) row-major) into its LDS block [1+P][n][PITCH]
template <int N, class S>
__device__ __forceinline__ void stage_model(S* dst, const M4Q_GLOBAL S* src, int jj) {
  constexpr int W = N * (1 + NP);
  // (not unrolled: unrolling this loop costs registers and time, profiles/r02_ab_experiments.txt)
#pragma unroll 1
  for (int e = jj; e < N * W; e += 16) {
    const int i = e / W;
    const int pk = e - i * W;
    const int p = pk / N;
    const int k = pk - p * N;
    dst[ModelPitch<N>::at(p, i, k)] = gld(src, e);
  }
}

// geometry of one lane inside its quad
struct LaneGeo {
  int g, jj, j;
  bool lane_ok;
  __device__ __forceinline__ LaneGeo() {
    const int lane = threadIdx.x;
    g = lane >> 4;
    jj = lane & 15;
    j = jj < NX ? jj : NX - 1;
    lane_ok = jj < NX;
  }
};

// The auxiliary kernels stride over quads of members, one member per DPP row: row g of quad `quad` works on member b.  A row past
// the end of the ensemble repeats the last member (as row gl of the quad, for lane offsets from the quad's first member q0) so that
// every lane stays active for the broadcasts, and stores nothing (!valid).
__device__ __forceinline__ int quads_of(int B) { return (B + ROWS - 1) / ROWS; }
struct QuadRow {
  long q0;
  bool valid;
  unsigned gl;
  long b;
  __device__ __forceinline__ QuadRow(int quad, int g, int B)
      : q0((long)quad * ROWS), valid(q0 + g < B), gl(valid ? g : (unsigned)(B - 1 - q0)), b(q0 + gl) {}
};

// xn = one held-control step of the device plant PLANT (m4q_mpc.h) from x over dt; scratch: the row's SCRATCH_ELEMS of LDS (the
// generator needs none).  A macro, not a function: one more inlined call around the plant functions changes the code of every
// kernel that steps a plant at the shapes with two or three controls (other address arithmetic, two more SGPRs in one of them),
// and so does a temporary for the result in mpc_kernel.
#define M4Q_PLANT_STEP(PLANT, xn, x, u, op0, ops, dt, scratch, j, jj)                                                   \
  do {                                                                                                                  \
    if constexpr ((PLANT) == PLANT_HAMILTONIAN) xn = plant_hamiltonian<NX, NU, DD>(x, u, op0, ops, dt, scratch, j, jj); \
    else if constexpr ((PLANT) == PLANT_PROCESS) xn = plant_process<NX, NU, DQ>(x, u, op0, ops, dt, scratch, j, jj);    \
    else xn = plant_generator<NX, NU>(x, u, op0, ops, dt, j);                                                           \
  } while (0)

// Re(d^H W d) of a row: Wr is this lane's row of W (N complex), d this lane's entry, read from the others by DPP broadcast
template <int N>
__device__ __forceinline__ double quad_figure(cplx d, const M4Q_GLOBAL cplx* Wr) {
  cplx y = czero();
  static_for<0, N>([&](auto k) { cmac(y, gld(Wr, decltype(k)::value), bcast<decltype(k)::value>(d)); });
  return rowsum<N>(dot_re(d, y));
}

// ---------------------------------------------------------------------------------------------
// The fused closed loop (replaces mpc.py:161-292).
//
// Work items: an instance's run is cut at MPC step 2.  Steps 0-1 iterate the SQP to convergence (14..100
// solves, data dependent); steps >= 2 are one solve each (mpc.py:208-212).  The queue hands out all the
// "head" items (steps [step_begin, 2)) first, then the uniform "tail" items (steps [2, step_end)), so the
// long, uneven pieces are packed first and the launch drains on short uniform ones.  A tail item may be
// drawn by another workgroup - possibly on another XCD - than the one that ran its head: the head
// publishes the instance state with an agent-scope release and a flag, the tail polls the flag (without
// blocking its wavefront) and acquires.
//
// Scheduling: the wavefront is a four-slot machine.  Every DPP row pulls its OWN next instance from a
// device-wide atomic queue and carries its own (instance, MPC step, SQP iteration); one pass of the main
// loop performs one QP solve for each row at whatever point of its run that row has reached.  SQP
// iteration counts at steps 0-1 range from 14 to 100 (config 3): with rows in lockstep a quad runs at
// the pace of its slowest member and a static split leaves the slowest wave 1.6x the mean.
//
// S = cplx: any model.  S = double: Hermiticity-preserving models in the Hermitian operator basis
// (a quarter of the FMAs, half the LDS and workspace traffic); the host decides (m4q_capi.hip).
// ---------------------------------------------------------------------------------------------
constexpr int COST_ELEMS = 2 * NX * NX + NU * NU;         // Q, Qf, R staged in LDS once per workgroup
constexpr int WLS_DOUBLES = 4 * NX + 2 * NU;               // diagonal line-search weights, staged after them
constexpr int STASH_INTS = 12;                             // per-row words of RowStash
// The complex path parks x_meas in the plant / basis-change scratch (idle during a solve: 108 complex slots at d = 3, 64 needed)
// instead of a block of its own: with one the kernel needed 21,480 B of LDS, a seventh of a CU's 160 KB was 1,000 B too small for an
// eighth workgroup, and the launch ran on 1,792 wavefronts instead of 2,048 (round 3's +3.5 % on that path until this was seen in
// SQ_WAVE_CYCLES / GRBM_GUI_ACTIVE: 54 against 63).
template <class S, bool SG = false> constexpr bool stash_x_in_scratch() { return (SG || sizeof(S) == sizeof(cplx)) && ROWS * SCRATCH_ELEMS >= 64; }
template <class S, bool SG = false> constexpr int stash_bytes() {
  return 8 /* watchdog deadline */ + ROWS * STASH_INTS * 4 + (stash_x_in_scratch<S, SG>() ? 0 : 64 * 16) /* x_meas, one S per lane */;
}

// sizes of the staged model and costs for a recursion on N coordinates
template <int N> constexpr int model_elems() { return (1 + NP) * N * ModelPitch<N>::value; }
template <int N> constexpr int cost_elems() { return 2 * N * N + NU * NU; }

// Transposed copies of Q and Qf behind the costs (CostRef<S, TR>, m4q_mpc.h): the exact mode on a recursion whose rows are 64 bytes
// long (n = 8 doubles), where the row reads of (Q e)_j conflict
template <class S, int N, bool EXACT> constexpr bool cost_transposed() { return EXACT && sizeof(S) == sizeof(double) && N == 8; }
// the exact mode's pinned sweep runs on matrix-core tiles where the clipped mode's backward sweep does (traceless real path of a
// shape with HAS_TILE): config 3 exact 208 -> 190 ms (profiles/r04_ab_experiments.txt)
template <class S, bool TL, bool EXACT> constexpr bool exact_tile() { return EXACT && TL && HAS_TILE && sizeof(S) == sizeof(double); }
// SG: ROWS blocks A_i and ONE set of NP blocks N_k instead of ROWS x (1 + NP) blocks
template <int N, bool SG> constexpr int model_lds_elems() {
  return SG ? (ROWS + NP) * N * ModelPitch<N>::value : ROWS * model_elems<N>();
}
// everything but the line search's weight table, which lies behind it
template <class S, bool TL = false, bool TILE = false, bool EXACT = false, bool SG = false>
constexpr size_t mpc_lds_fixed_bytes() {
  constexpr int N = TL ? NX - 1 : NX;
  return sizeof(S) * (size_t)(model_lds_elems<N, SG>() + cost_elems<N>() + (cost_transposed<S, N, EXACT>() ? 2 * N * N : 0)) +
         sizeof(cplx) * (size_t)(ROWS * SCRATCH_ELEMS) + sizeof(double) * (size_t)WLS_DOUBLES + (size_t)stash_bytes<S, SG>() +
         (TILE ? (size_t)(TILE_LDS_BYTES + tile_opnd::bytes(NU, (N + 3) / 4)) : 0) + (exact_tile<S, TL, EXACT>() ? (size_t)(TILE_LDS_BYTES + TILE_PIN_LDS_BYTES) : 0);
}
// Which kernels read the node weights of the line search (line_search_tl_nodes, m4q_mpc.h: n - 1 even) from a table (m4q_ls_table.h)
// that every workgroup builds at kernel entry: the clipped tile kernels, in what their eighth of a CU's LDS leaves - 47 nodes at
// (9, 2, 1), horizons up to 46; a longer one runs without it.  Config 3 -0.9 % (profiles/r11_ab_experiments.txt).  The DPP and the exact
// kernels keep the divisions (the exact ones carry 150-250 spilled registers and have not measured faster with such cuts: see
// shift_in_update() below).
template <bool TL, bool TILE, bool EXACT>
constexpr bool ls_weights_tabled() {
  return TL && TILE && !EXACT && (NX - 1) % 2 == 0;
}
template <class S, bool TL = false, bool TILE = false, bool EXACT = false, bool SG = false>
constexpr int ls_table_nodes() {
  return ls_weights_tabled<TL, TILE, EXACT>() ? ls_table::capacity(NX, (int)mpc_lds_fixed_bytes<S, TL, TILE, EXACT, SG>()) : 0;
}
template <class S, bool TL = false, bool TILE = false, bool EXACT = false, bool SG = false>
constexpr size_t mpc_lds_layout_bytes() {
  return mpc_lds_fixed_bytes<S, TL, TILE, EXACT, SG>() + (size_t)ls_table::bytes(NX, ls_table_nodes<S, TL, TILE, EXACT, SG>());
}

__device__ __forceinline__ int row_bcast_int(int v) { return __shfl(v, 0, 16); }
// the same wave-uniform number, opaque to the compiler: what is derived from it is computed (and dies) where it is used
__device__ __forceinline__ int fresh(int v) { asm volatile("" : "+s"(v)); return v; }

// Kernel arguments are read out of the kernarg segment WHERE THEY ARE USED.  Taken as a by-value parameter the 46 fields of
// MpcArgs are loaded at kernel entry, stay live for the whole persistent loop and - the kernel has 106 scalar registers -
// end up in VGPR lanes (v_writelane / v_readlane: 161 "spilled SGPRs" in the round-2 build of the headline kernel, 445
// v_readlane per pass of the main loop).  kargs() returns the segment pointer through an opaque asm, once per phase of the
// loop: the compiler can neither hoist the loads of one phase to the kernel entry nor keep their results alive into the next.
typedef const __attribute__((address_space(4))) MpcArgs KArgs;
__device__ __forceinline__ KArgs* kargs() {
  KArgs* p = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // explicit arguments start at offset 0
  asm volatile("" : "+s"(p));
  return p;
}

// Per-row state that only the bookkeeping phases of the loop need, parked in LDS while the two sweeps run (they take the
// whole register file; left to the compiler these values went to scratch: 178 spilled VGPRs in the round-2 headline kernel).
// Row-uniform words are written by the row's lane 0 and read back as an LDS broadcast; volatile, so that the values are
// really re-read after the sweeps instead of being carried in registers across them.
#define M4Q_LDS __attribute__((address_space(3)))
template <class S>
struct RowStash {
  volatile M4Q_LDS int* w;          // [ROWS][STASH_INTS]
  volatile M4Q_LDS double* xm;      // [64][2]
  __device__ __forceinline__ void put_int(int g, int jj, int slot, int v) const { if (jj == 0) w[g * STASH_INTS + slot] = v; }
  __device__ __forceinline__ int get_int(int g, int slot) const { return w[g * STASH_INTS + slot]; }
  __device__ __forceinline__ void put_x(double v) const { xm[2 * threadIdx.x] = v; }
  __device__ __forceinline__ void put_x(cplx v) const { xm[2 * threadIdx.x] = v.re; xm[2 * threadIdx.x + 1] = v.im; }
  __device__ __forceinline__ void get_x(double& v) const { v = xm[2 * threadIdx.x]; }
  __device__ __forceinline__ void get_x(cplx& v) const { v.re = xm[2 * threadIdx.x]; v.im = xm[2 * threadIdx.x + 1]; }
};

// the exact mode's pinned sweep on tiles: what a row hands to the tile layout (member = (lane >> 2) & 3 there, lane >> 4 in rows)
template <int NS>
struct ExactTile {
  static constexpr bool enabled = true;
  const double* lds_models;
  volatile M4Q_LDS double* tgb; volatile M4Q_LDS int* tiw; volatile M4Q_LDS double* tpin;
  GView Xg, Ug, gains;
  const double* Q; const double* Qf; const double* R;
  unsigned sX, sU, sG;
  int g, jj;
  __device__ __forceinline__ void sweep(int T, const Window& win, const PinCtx<NU>& pin, bool going) const {
    if (jj == 0) {
      tiw[g * TILE_IO_WORDS + 0] = going ? 1 : 0;
      tiw[g * TILE_IO_WORDS + 1] = (int)win.xbm.off;
      tiw[g * TILE_IO_WORDS + 2] = (int)win.ubm.off;
      tiw[g * TILE_IO_WORDS + 3] = (int)pin.stat.off;
#pragma unroll
      for (int k = 0; k < NU; ++k) { tpin[g * TILE_PIN_DOUBLES + k] = pin.lo0[k]; tpin[g * TILE_PIN_DOUBLES + 3 + k] = pin.hi0[k]; }
    }
    wave_sync();
    TileBackwardB<NS, NU, ORDER, true> ts;
    const int mb = ts.L.mb;
    const int dm = mb - g;
    ts.mdl = lds_models + mb * model_elems<NS>();
    ts.T = T;
    ts.Xg = Xg; ts.Xg.off = Xg.off + (unsigned)(dm * (int)(sX * sizeof(double)));
    ts.Ug = Ug; ts.Ug.off = Ug.off + (unsigned)(dm * (int)(sU * sizeof(double)));
    ts.gains = gains; ts.gains.off = gains.off + (unsigned)(dm * (int)(sG * sizeof(double)));
    ts.xbm = win.xbm; ts.xbm.off = (unsigned)tiw[mb * TILE_IO_WORDS + 1];
    ts.ubm = win.ubm; ts.ubm.off = (unsigned)tiw[mb * TILE_IO_WORDS + 2];
    ts.stat = pin.stat; ts.stat.off = (unsigned)tiw[mb * TILE_IO_WORDS + 3];
    ts.sat = pin.box.sat;
    ts.Q = Q; ts.Qf = Qf; ts.R = R;
    ts.gb = tgb + mb * TILE_GB_DOUBLES;
    const bool run_t = tiw[mb * TILE_IO_WORDS + 0] != 0;
    ts.backward(run_t);
    wave_sync();
  }
};

// TL: the state lives in the NX - 1 traceless coordinates (S = double only; m4q_mpc.h).  NS = dimension of the recursion;
// the I/O side (xs, the SQP-guess checkpoint, the plant) stays NX complex numbers per node.
// TILE: the two sweeps of the clipped solve run on fp64 matrix-core tiles (m4q_tile.h) instead of DPP rows.
// smallest recursion dimension that gets the constant-target instantiation of the sweeps (round 2: 15 - at d = 3 the second
// instantiation cost more in register allocation than it saved; with round 3's lower pressure it pays: config 3 41.3 -> 40.3 ms,
// config 5's share 138.1 -> 134.7; d = 2 indifferent)
constexpr int TC_MIN_N = 8;
// EXACT: further cuts of an instance's run after step 2 (strictly increasing, > 2; see the kernel)
// (round 3, when every cut cost two passes of 41 basis changes: one cut at 5.  Round 4, with the guess handed over as it is:
//  {4, 7, 12} - config 3 185-187 ms either way, config 4 1,747 -> 1,657, config 5's share 4,315 -> 4,155; {5, 10}: 1,704 at
//  config 4; a cut at every step 3..9: 189 ms at config 3; profiles/r04_ab_experiments.txt)
constexpr int XCUTS[] = {4, 7, 12};
constexpr int NXC = (int)(sizeof(XCUTS) / sizeof(int));
// the shared-generator and the tile kernels are compiled for two wavefronts per SIMD at every shape
constexpr int WAVES_SG = 2;
constexpr int WAVES_TILE = 2;
// Issue priority by phase of the main loop (PrioMap, m4q_device.h), per instantiation and shape.  The two wavefronts of a SIMD run this
// kernel unsynchronised; at equal priority the older one wins every issue conflict for the whole launch, whatever the two are doing:
// a younger wavefront's rollout - a dependent chain of 4-cycle FMAs - then waits behind the older one's back-to-back 16-cycle MFMAs.
// With the sweep at 0 and every later phase of the pass at 1 the short instruction goes first and the sweep, which has independent
// MFMAs to spare, takes the remaining slots; no wavefront waits for another and no arithmetic changes.  Config 3 (the clipped tile
// kernel at n = 8): -1.2 to -1.3 % in each of three alternations against a 0.05 % spread of the parent's runs; the short phases at 2 above
// the rollout: the same; the sweep at 1 above everything else: +1.0 % (profiles/r07_ab_experiments.txt).  Kernels, shapes and
// plants that have not been measured faster with levels keep all zeros: their code is then the same as without this table.
template <class S, int PLANT, bool EXACT, bool TL, bool TILE, bool SG>
constexpr PrioMap prio_map() {
  if (TILE && !EXACT && NX == 9 && PLANT == PLANT_HAMILTONIAN) return PrioMap{0, 1, 1, 1, 1, 1};
  return PrioMap{0, 0, 0, 0, 0, 0};
}
// Which kernels store a finished SQP step's guess one node down in the guess update itself (see `shift_now` in mpc_kernel) instead
// of shifting it in a second pass of the step-done block.  The clipped kernels: config 3 -1.9 %, config 5's share -2.0 %, configs 2
// and 4 inside their spread.  The exact kernels keep the two passes: they carry 150-250 spilled registers, the shifted stores add
// 3-9 more at n = 8, 9, and --exact-qp (config 3) did not come out faster - 185.97 / 185.48 / 184.90 ms against the parent's
// 180.44 / 185.89 / 183.18 in one alternated call, +1.2 % in the mean inside a 3 % spread (profiles/r08_ab_experiments.txt).
template <bool EXACT>
constexpr bool shift_in_update() {
  return !EXACT;
}
// Development builds (-DM4Q_DEV_PHASE_CLOCK): PhaseClock (m4q_device.h) sums the 100 MHz clock over the phases of the main loop; every
// wavefront adds its sums to queue[8..23] (u64) on exit; M4Q_PHASE_TRACE=1 makes m4q_session_qp_stats print them.
#if defined(M4Q_DEV_PHASE_CLOCK)
#define M4Q_PHASE_FLUSH() if (threadIdx.x == 0) { for (int i = 0; i < 16; ++i) __hip_atomic_fetch_add((M4Q_GLOBAL unsigned long long*)kargs()->queue + 8 + i, pc.acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
#define M4Q_PHASE_FLUSH()
#endif
#define M4Q_PHASE_DECL PhaseClock pc;
#define M4Q_PHASE_MARK(i) pc.mark(i);
#define M4Q_PHASE_MARK_CLIP(i) if constexpr (!EXACT) pc.mark(i);      // (slots 10, 11, 13: the exact solve's own in an exact kernel)
template <class S, int PLANT, bool EXACT, bool TL = false, bool TILE = false, bool SG = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SG ? WAVES_SG : TILE ? WAVES_TILE : WAVES, 8))) void mpc_kernel(MpcArgs) {
  static_assert(!TL || (sizeof(S) == sizeof(double) && SQUARE), "the traceless path is a real path of a d x d density matrix");
  static_assert(!TILE || (TL && !EXACT && ORDER == 1), "tile sweep: clipped solve on the traceless real coordinates, order-1 libraries");
  static_assert(!SG || (TL && !TILE && !EXACT && ORDER == 1), "shared generators: the clipped traceless kernel of an order-1 library");
  constexpr int NS = TL ? NX - 1 : NX;
  using Prov = FusedProv<S, NS, NU, ORDER, SG>;
  // LDS: [4 x scratch (complex)] [4 x model (S)] [Q Qf R (S)] [line-search weights] [watchdog deadline, row stash]
  cplx* scratch = reinterpret_cast<cplx*>(m4q_lds_raw);
  S* lds = reinterpret_cast<S*>(scratch + ROWS * SCRATCH_ELEMS);
  const LaneGeo L;
  const int g = L.g, jj = L.jj;
  const int j = jj < NS ? jj : NS - 1;           // this lane's state coordinate (lanes that own none shadow the last)
  const int jio = L.j;                           // ... and its slot of vec(rho) on the I/O side
  const bool lane_ok = jj < NS, lane_io = L.lane_ok;
  double tau = 0.0;                              // TL: the member's trace coordinate tr(rho)/sqrt(d) (row-uniform)
  constexpr bool QTR = cost_transposed<S, NS, EXACT>();
  // (SG: MODEL_K is one block - the member's A_i -, the NP shared blocks N_k follow the ROWS of them)
  constexpr int MODEL_K = SG ? NS * ModelPitch<NS>::value : model_elems<NS>(), COST_K = cost_elems<NS>() + (QTR ? 2 * NS * NS : 0);
  S* mdl = lds + g * MODEL_K;
  S* mdn = lds + ROWS * MODEL_K;                   // (SG only)
  scratch += g * SCRATCH_ELEMS;
  S* ldsQ = lds + model_lds_elems<NS, SG>();
  double* ldsW = reinterpret_cast<double*>(ldsQ + COST_K);
  volatile M4Q_LDS unsigned long long* wd_slot = (volatile M4Q_LDS unsigned long long*)(ldsW + WLS_DOUBLES);
  RowStash<S> stash;
  stash.w = (volatile M4Q_LDS int*)(ldsW + WLS_DOUBLES + 1);
  stash.xm = stash_x_in_scratch<S, SG>() ? (volatile M4Q_LDS double*)m4q_lds_raw : (volatile M4Q_LDS double*)(stash.w + ROWS * STASH_INTS);
  // TILE: hand-over block between the DPP-row state machine and the tile sweeps, and the G / h broadcast tiles
  volatile M4Q_LDS double* tgb = stash.xm + 64 * 2;
  volatile M4Q_LDS int* tiw = (volatile M4Q_LDS int*)(tgb + ROWS * TILE_GB_DOUBLES);
  volatile M4Q_LDS double* tpin = (volatile M4Q_LDS double*)(tiw + ROWS * TILE_IO_WORDS);      // (exact_tile kernels only)
  volatile M4Q_LDS double* timg = (volatile M4Q_LDS double*)(tiw + ROWS * TILE_IO_WORDS);      // (TILE: the sweep's operand image, m4q_tile_opnd.h)
  // the line search's weight table (m4q_ls_table.h), behind everything else
  constexpr bool LS_TABLE = ls_weights_tabled<TL, TILE, EXACT>();
  constexpr int LS_NODES = ls_table_nodes<S, TL, TILE, EXACT, SG>();
  double* ldsT = nullptr;
  if constexpr (LS_TABLE) ldsT = reinterpret_cast<double*>(m4q_lds_raw + mpc_lds_fixed_bytes<S, TL, TILE, EXACT, SG>());
  int T0, flags;
  bool ls_diag, two_phase;
  int n_pieces;                // work items per instance: head [step_begin, 2), then [2, XCUTS[0]), ... , [.., step_end)
  auto piece_cut = [](int i) __attribute__((always_inline)) {       // where piece i (>= 1) begins
    int v = 2;
#pragma unroll
    for (int k = 0; k < NXC; ++k)
      if (i == k + 2) v = XCUTS[k];
    return v;
  };
  auto piece_of = [&](int begin, int step_begin) __attribute__((always_inline)) {   // which piece begins there
    int ph = begin == step_begin ? 0 : 1;
#pragma unroll
    for (int k = 0; k < NXC; ++k)
      if (begin == XCUTS[k] && begin != step_begin) ph = k + 2;
    return ph;
  };
  {
    KArgs* a = kargs();
    T0 = a->T;
    flags = a->flags;
    const M4Q_GLOBAL S* gQ = (const M4Q_GLOBAL S*)a->Q;
    const M4Q_GLOBAL S* gQf = (const M4Q_GLOBAL S*)a->Qf;
    const M4Q_GLOBAL S* gR = (const M4Q_GLOBAL S*)a->R;
    for (int e = threadIdx.x; e < 2 * NS * NS + NU * NU; e += 64)
      ldsQ[e] = e < NS * NS ? gld(gQ, e) : (e < 2 * NS * NS ? gld(gQf, e - NS * NS) : gld(gR, e - 2 * NS * NS));
    if constexpr (QTR) {
      for (int e = threadIdx.x; e < 2 * NS * NS; e += 64) {
        const int blk = e / (NS * NS), r = (e / NS) % NS, c = e % NS;
        ldsQ[cost_elems<NS>() + e] = gld(blk ? gQf : gQ, c * NS + r);
      }
    }
    if constexpr (SG) {
      // the workgroup's copy of N_k = dt L_k (a->gens: [1 + NP][NS][NS] doubles, already scaled by dt; block 0 = dt L_0 is read
      // per member when its A_i is formed)
      for (int e = threadIdx.x; e < NP * NS * NS; e += 64) {
        const int p = e / (NS * NS), r = (e / NS) % NS, c = e % NS;
        mdn[ModelPitch<NS>::at(p, r, c)] = gld((const M4Q_GLOBAL S*)a->gens, NS * NS + e);
      }
    }
    ls_diag = a->Wls != nullptr;
    if (ls_diag) {
      for (int e = threadIdx.x; e < WLS_DOUBLES; e += 64) ldsW[e] = gld(a->Wls, e);
      if constexpr (LS_TABLE) {
        // (once per launch: the weights, the horizon and the slots are the same for every pass)
        if (ls_table::tabled(T0, LS_NODES)) {
          wave_sync();
#pragma unroll 1
          for (int e = threadIdx.x; e < (T0 + 1) * NX; e += 64) ldsT[e] = ls_table::entry(ldsW, NX, DD, T0, e / NX, e % NX);
        }
      }
    }
    // cut the run in two work items per instance when the launch covers both regimes
    two_phase = a->step_begin < 2 && a->step_end > 2;
    // EXACT: a third piece.  The hard solves of the exact mode are the first warm steps (their shifted guess is poor: 30-130
    // active-set iterations against 1-2), so a tail [2, step_end) is as uneven as a head; cut again (XCUTS) the launch drains on the
    // late steps' uniform one-sweep solves instead (round 3, config 3: no cut 255 ms, at 8 245-247, at 6 236-239, at 5 233, at 4 244).
    n_pieces = two_phase ? 2 : 1;
    if constexpr (EXACT) {
#pragma unroll
      for (int i = 0; i < NXC; ++i)
        if (two_phase && a->step_end > XCUTS[i]) ++n_pieces;
    }
    // Watchdog.  The loop below ends when the queue is empty and every row has finished, and a tail item waits for a flag another
    // workgroup sets: exits that depend on data.  A persistent kernel whose wavefronts never finish takes the GPU (and on this pool
    // the host's other GPUs) down with it, so every wavefront also leaves once the constant 100 MHz clock has advanced
    // deadline_ticks since it started; the host finds queue[1] set and fails the launch loudly (M4Q_E_TIMEOUT).  Every loop of
    // the kernel without a data-independent trip bound passes through this check: the main loop below (one pass = at most one
    // QP solve or one active-set iteration per row; the head-flag poll is a pass of it that only sleeps), nothing else - the
    // horizon loops run T trips, the plant's squaring loop at most 60, the staging loops over fixed sizes.
    if (threadIdx.x == 0) *wd_slot = __builtin_amdgcn_s_memrealtime() + a->deadline_ticks;
  }
  CostRef<S, QTR> cost;
  cost.Q = ldsQ; cost.Qf = ldsQ + NS * NS; cost.q_stride = 0; cost.R = ldsQ + 2 * NS * NS; cost.r_stride = 0;
  if constexpr (QTR) { cost.QT = ldsQ + cost_elems<NS>(); cost.QfT = cost.QT + NS * NS; }
  // workspace of this resident row: wave-uniform base per workgroup, lane part = row within the wave
  const unsigned sX = (unsigned)(T0 + 1) * NS, sU = (unsigned)T0 * NU, sG = (unsigned)T0 * (NS + 1) * NU;
  const unsigned sXc = (unsigned)(T0 + 1) * NX;            // the SQP-guess checkpoint field: complex, NX per node
  constexpr bool PIECE_RAW = sizeof(S) == sizeof(double);     // (between items of one launch: see the publish step)
  // Lanes NX..15 of a row own no column (7 of 16 at d = 3, 12 of 16 at d = 2).  Left enabled they run the sweeps on a copy of
  // column NX-1's data: harmless for the results, but the fp64 pipe spends power on them, and the clock this chip holds under an
  // fp64-dense load follows the power.  EXEC is therefore off for them during the two sweeps (every DPP source is a lane < NX;
  // results bit-identical): the complex path runs at 2.30 GHz instead of 2.04 (133.3 -> 117.6 ms, config 3), the real path at 2.29
  // instead of 2.18 (51.2 -> 50.4 ms; config 5's share 171.2 -> 166.3 ms).  profiles/r02_ab_experiments.txt, r02_clock_ramp.txt.
  constexpr bool MASK_IDLE = NS < 16 && !EXACT && !TILE;
  // (the levels change at the phase boundaries of the main loop only, outside every lane-dependent branch: s_setprio ignores EXEC)
  constexpr PrioMap PRIO = prio_map<S, PLANT, EXACT, TL, TILE, SG>();
  constexpr bool PRIO_ON = PRIO.any();
  constexpr bool SHIFT_IN_UPDATE = shift_in_update<EXACT>();
  static_assert(!EXACT || !PRIO_ON, "the exact solve's phases are those of box_qp_iterate: no levels there yet");
  GView Xg, Ug, Xo, Uo, gains, Xalt, Ualt, pin_stat;
  {
    KArgs* a = kargs();
    const long wsb = blockIdx.x;
    M4Q_GLOBAL S* wX = (M4Q_GLOBAL S*)a->ws_Xg;
    Xg = gview(wX, wsb * ROWS * sX, g * sX);
    Ug = gview(a->ws_Ug, wsb * ROWS * sU, g * sU);
    // (Xo, Uo) live in the same allocations right behind all the (Xg, Ug): same wave-uniform base, so a row can
    // direct its rollout output to either by its lane offset alone
    Xo = gview(wX, wsb * ROWS * sX, g * sX + gridDim.x * ROWS * sX);
    Uo = gview(a->ws_Ug, wsb * ROWS * sU, g * sU + gridDim.x * ROWS * sU);
    gains = gview((M4Q_GLOBAL S*)a->ws_gains, wsb * ROWS * sG, g * sG);
    // EXACT (M4Q_QP_EXACT_BOX): third trajectory pair, working set and Newton point of the projected-Newton solver,
    // again behind the others in the same allocations
    Xalt = gview(wX, wsb * ROWS * sX, g * sX + 2 * gridDim.x * ROWS * sX);
    Ualt = gview(a->ws_Ug, wsb * ROWS * sU, g * sU + 2 * gridDim.x * ROWS * sU);
    pin_stat = gview(a->ws_Ug, wsb * ROWS * sU, g * sU + 3 * gridDim.x * ROWS * sU);
  }
  const bool band = (flags & QP_DU_BAND) != 0;

  // per-row state (uniform inside a row)
  long b = 0;
  bool active = false, need_new = true, pending = false;
  int step = 0, iter = 0, code = 0, done_steps = 0;
  int row_begin = 0, row_end = 0;
  S x_cur = zero_of<S>();
  S x_meas = zero_of<S>();     // last MEASURED state (xs[k * measure_freq]); equals x_cur when measure_freq == 1
  double uprev[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) uprev[k] = 0.0;
  double gsc[SG ? NU : 1];     // SG: this row's member's scales of the control operators
#pragma unroll
  for (int k = 0; k < (SG ? NU : 1); ++k) gsc[k] = 1.0;
  BoxQpRow qp;                 // EXACT: the box-QP solve this row has in progress (spans iterations of the loop below)
  int qp_passes = 0;           // passes of this wavefront through the solver iteration (statistics)
  unsigned xt_off = 0, ut_off = 0, op0_off = 0, ops_off = 0;      // this row's member inside the per-member arrays (bytes)
  wave_sync();
  M4Q_PHASE_DECL

  while (true) {
    // The horizon and the row's workspace offsets go through an opaque asm once per pass: everything derived from them
    // (unroll-remainder predicates of the horizon loops, 64-bit element addresses) is then computed in the phase that uses it.
    // Hoisted to the kernel entry - they are invariants of this loop - those values lived through every phase and were what
    // the allocator spilled (predicate pairs into VGPR lanes, addresses into scratch).
    int T = T0;
    asm volatile("" : "+s"(T));
    asm volatile("" : "+v"(Xg.off), "+v"(Ug.off), "+v"(Xo.off), "+v"(Uo.off), "+v"(gains.off));
    if constexpr (EXACT) asm volatile("" : "+v"(Xalt.off), "+v"(Ualt.off), "+v"(pin_stat.off));
    Prov prov;
    prov.mdl = mdl; prov.Xg = Xg; prov.Ug = Ug; prov.j = j;
    if constexpr (SG) prov.mdn = mdn;        // (prov.sc: set after the draw below - a row may take a new member in this very pass)

    if (__builtin_amdgcn_s_memrealtime() > *wd_slot) {
      if (threadIdx.x == 0) __hip_atomic_store(kargs()->queue + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    M4Q_PHASE_MARK(3)
    // ---- rows without work draw the next item; tail items wait (without blocking) for their head ----
    if (__any(need_new || pending)) {
      KArgs* a = kargs();
      const int B = a->B, n_items = n_pieces * B;
      const int step_begin = a->step_begin, step_end = a->step_end, mf = a->measure_freq;
      const long sXs = (long)(a->n_steps + 1) * NX, sUs = (long)a->n_steps * NU;
      int nb = 0;
      if (need_new && jj == 0) nb = __hip_atomic_fetch_add(a->queue, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      nb = row_bcast_int(nb);
      if (need_new) {
        need_new = false;
        if (nb < n_items) {
          const int ph = nb / B;                               // 0 head, then the later pieces in order
          b = nb - ph * B;
          row_begin = ph == 0 ? step_begin : piece_cut(ph);
          row_end = ph == n_pieces - 1 ? step_end : piece_cut(ph + 1);
          pending = true;
        }
      }
      // a tail item starts once the head of its instance has been published
      // (head_done[b] counts the pieces of the instance that have been published)
      int ready = 1;
      const bool later = two_phase && row_begin != step_begin;
      if (pending && later && jj == 0)
        ready = __hip_atomic_load(a->head_done + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= piece_of(row_begin, step_begin) ? 1 : 0;
      ready = row_bcast_int(ready);
      const bool fresh = pending && ready != 0;
      if (__any(fresh && later)) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (fresh) { pending = false; active = true; }
      wave_sync();
      if (fresh) {
        if constexpr (SG) {
          // A_i = I + s_i0 (dt L_0) from the shared generator; the member's other scales ride on the controls (FusedProv<..., SG>)
          const M4Q_GLOBAL double* sc = a->scales + b * (1 + NU);
          const double s0 = gld(sc, 0);
#pragma unroll
          for (int k = 0; k < NU; ++k) gsc[k] = gld(sc, 1 + k);

#pragma unroll 1
          for (int e = jj; e < NS * NS; e += 16) {
            const int r = e / NS, c = e - r * NS;
            mdl[ModelPitch<NS>::at(0, r, c)] = fma(s0, gld((const M4Q_GLOBAL S*)a->gens, e), r == c ? 1.0 : 0.0);
          }
        } else {
          stage_model<NS>(mdl, (const M4Q_GLOBAL S*)a->models + b * a->model_stride, jj);
        }
        xt_off = (unsigned)(b * a->xt_stride) * (unsigned)sizeof(S);
        ut_off = (unsigned)(b * a->ut_stride) * (unsigned)sizeof(double);
        op0_off = (unsigned)(b * a->plant.op0_stride) * (unsigned)sizeof(cplx);
        ops_off = (unsigned)(b * a->plant.ops_stride) * (unsigned)sizeof(cplx);
        step = row_begin;
        iter = 0;
        code = 0;
        done_steps = 0;
        if (row_begin <= 1) {                                    // u_prev of steps 0 and 1: U_ref[:, 0] (mpc.py:185)
          GView u0 = gview(a->u_targ, 0, 0);
          u0.off = ut_off;
#pragma unroll
          for (int k = 0; k < NU; ++k) uprev[k] = u0.ld<double>(k);
        }
      }
      if (__any(fresh && row_begin == 0)) {
        if (fresh && row_begin == 0) {
          // X_guess = tile(x0), U_guess = 0 (mpc.py:141-142); xs[0] = x0 (:160)
          const S x0 = gld((const M4Q_GLOBAL S*)a->x0s, b * NS + j);
          x_cur = x0;
          x_meas = x0;
          if (lane_ok) {
#pragma unroll 8
            for (int t = 0; t <= T; ++t) Xg.st<S>(t * NS + j, x0);
          }
          if (lane_io) gst(a->xs, b * sXs + jio, gld(a->x0c, b * NX + jio));
          for (int e = jj; e < T * NU; e += 16) Ug.st<double>(e, 0.0);
        }
        if constexpr (TL) {
          // the member's trace coordinate, from the complex x0 (every lane of the row ends up with it)
          double t0 = 0.0;
          const cplx xc = (fresh && row_begin == 0) ? gld(a->x0c, b * NX + jio) : czero();
          (void)Basis<S, TL>::template to_state<NX, DD>(xc, scratch, j, jj, t0);
          if (fresh && row_begin == 0) tau = t0;
        }
      }
      if (__any(fresh && row_begin != 0)) {
        // resume: the SQP guess, state and exit code of an earlier item or launch (fields X_GUESS/U_GUESS/XS/US/CODES).
        // From an earlier LAUNCH (or the host) the stored guess is complex in the original basis; the basis change needs every lane
        // (LDS exchange).  From an earlier item of THIS launch (real paths) it is the working guess itself, as the item left it in
        // the same field (PIECE_RAW: see the publish step) - a flat copy, no basis change and no rounding.
        const bool rs = fresh && row_begin != 0;
        const bool rs_raw = PIECE_RAW && rs && later;
        double tdum = 0.0, tnew = 0.0;
        if (__any(rs && !rs_raw)) {
          for (int t0 = 0; t0 <= T; t0 += 8) {
            cplx v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (rs && !rs_raw) ? gld(a->Xg, b * sXc + (t0 + q <= T ? t0 + q : T) * NX + jio) : czero();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              if (t0 + q <= T) {
                const S r = Basis<S, TL>::template to_state<NX, DD>(v[q], scratch, j, jj, tdum);
                if (rs && !rs_raw && lane_ok) Xg.st<S>((t0 + q) * NS + j, r);
              }
            }
          }
        }
        if constexpr (PIECE_RAW) {
          if (rs_raw) {
            const M4Q_GLOBAL double* raw = (const M4Q_GLOBAL double*)(a->Xg + b * sXc);
            const int count = (T + 1) * NS;
            if constexpr (NS % 2 == 0) {
              constexpr int U = 6;
              for (int e0 = 2 * jj; e0 < count; e0 += 32 * U) {
                d2_t v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const M4Q_GLOBAL d2_t*>(raw + (e0 + 32 * u < count ? e0 + 32 * u : count - 2));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                  if (e0 + 32 * u < count) {
                    const double r[2] = {v[u].x, v[u].y};
                    stn<2>(Xg, e0 + 32 * u, r);
                  }
                }
              }
            } else {
              constexpr int U = 12;
              for (int e0 = jj; e0 < count; e0 += 16 * U) {
                double v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = gld(raw, e0 + 16 * u < count ? e0 + 16 * u : count - 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < U; ++u)
                  if (e0 + 16 * u < count) Xg.st<double>(e0 + 16 * u, v[u]);
              }
            }
          }
        }
        const cplx xc = rs ? gld(a->xs, b * sXs + (long)row_begin * NX + jio) : czero();
        const S r = Basis<S, TL>::template to_state<NX, DD>(xc, scratch, j, jj, tdum);
        const cplx xm = rs ? gld(a->xs, b * sXs + (long)(row_begin / mf) * mf * NX + jio) : czero();
        const S rm = Basis<S, TL>::template to_state<NX, DD>(xm, scratch, j, jj, tnew);
        if (rs) {
          x_cur = r;
          x_meas = rm;
          tau = tnew;
          for (int e = jj; e < T * NU; e += 16) Ug.st<double>(e, gld(a->Ug, b * sU + e));
          code = gld(a->codes, b);
          done_steps = gld(a->steps_done, b);
#pragma unroll
          for (int k = 0; k < NU; ++k) uprev[k] = row_begin > 1 ? gld(a->us, b * sUs + (long)(row_begin - 1) * NU + k) : uprev[k];
          if (code != 0) step = row_end;          // finished earlier (exit code set by the host or the device)
        }
      }
      wave_sync();
    }
    M4Q_PHASE_MARK(0)
    if (!__any(active || pending)) {
      M4Q_PHASE_FLUSH()
      if (EXACT && threadIdx.x == 0)
        __hip_atomic_fetch_add((M4Q_GLOBAL unsigned long long*)kargs()->queue + 7, (unsigned long long)qp_passes, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    if (!__any(active)) {
      __builtin_amdgcn_s_sleep(8);                 // only tail items whose head is still running: poll again
      continue;
    }
    issue_prio<PRIO_ON && PRIO.sweep != 0, PRIO.sweep>();
    const bool running = active && step < row_end;
    if constexpr (SG) {
#pragma unroll
      for (int k = 0; k < NU; ++k) prov.sc[k] = gsc[k];
    }

    // ---- one QP solve per row ----
    // park what the sweeps do not need (the compiler would keep it in scratch across them)
    stash.put_int(g, jj, 0, (int)(b & 0xffffffff));
    stash.put_int(g, jj, 1, (int)(b >> 32));
    stash.put_int(g, jj, 2, code);
    stash.put_int(g, jj, 3, done_steps);
    stash.put_int(g, jj, 4, row_begin);
    stash.put_int(g, jj, 5, (active ? 1 : 0) | (need_new ? 2 : 0) | (pending ? 4 : 0));
    stash.put_int(g, jj, 6, (int)op0_off);
    stash.put_int(g, jj, 7, (int)ops_off);
    stash.put_x(x_meas);
    double uapp[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) uapp[k] = 0.0;
    double chk = 0.0;
    bool solved = running;       // the rows whose QP is solved in this pass and that go on to the line search / update / plant below.
                                 // Clipped mode: every running row, each pass.  EXACT: a row's solve spans several passes (one
                                 // active-set iteration per pass), so that no row waits for the slowest solve of its wavefront.
    bool capped = false;         // EXACT: the solve stopped at its iteration cap (not converged): exit code 2
    bool use_ls;
    Window win;
    {
      KArgs* a = kargs();
      // target window: X_ref = X_targ[:, :T+1] for steps 0 and 1, then X_targ[:, step-1:...] (mpc.py:145,276)
      const int w = step <= 1 ? 0 : step - 1;
      win.xbm = gview((const M4Q_GLOBAL S*)a->x_targ, 0, 0);
      win.xbm.off = xt_off + (unsigned)w * NS * (unsigned)sizeof(S);
      win.ubm = gview(a->u_targ, 0, 0);
      win.ubm.off = ut_off + (unsigned)w * NU * (unsigned)sizeof(double);
      const double sat = a->sat, du = a->du;
      double lo0[NU], hi0[NU];
#pragma unroll
      for (int k = 0; k < NU; ++k) {
        // u_prev = us[step-1] if step > 1 else U_ref[:, 0] (mpc.py:185): `uprev` holds whichever applies (set when the row took its
        // item and when a step ends) - read from the target array here it was a dependent global load in every pass of steps 0 and 1
        const double up = uprev[k];
        lo0[k] = band ? up - du : -sat;
        hi0[k] = band ? up + du : sat;
      }
      use_ls = !(a->warm_start && step > 1);        // mpc.py:208-213
      const bool st = running && lane_ok;
      if constexpr (TILE) {
        // ---- hand the row's solve to the tile layout: member = (lane >> 2) & 3 there, lane >> 4 here ----
        if (jj == 0) {
          tiw[g * TILE_IO_WORDS + 0] = running ? 1 : 0;
          tiw[g * TILE_IO_WORDS + 1] = (int)win.xbm.off;
          tiw[g * TILE_IO_WORDS + 2] = (int)win.ubm.off;
        }
        wave_sync();
        {
          TileBackwardB<NS, NU, ORDER> ts;
          const int mb = ts.L.mb;
          const int dm = mb - g;                                 // this lane's member there minus its member here
          ts.mdl = reinterpret_cast<const double*>(lds) + mb * MODEL_K;
          ts.T = T;
          ts.Xg = Xg; ts.Xg.off = Xg.off + (unsigned)(dm * (int)(sX * sizeof(double)));
          ts.Ug = Ug; ts.Ug.off = Ug.off + (unsigned)(dm * (int)(sU * sizeof(double)));
          ts.gains = gains; ts.gains.off = gains.off + (unsigned)(dm * (int)(sG * sizeof(double)));
          const int tfl = tiw[mb * TILE_IO_WORDS + 0];
          ts.xbm = win.xbm; ts.xbm.off = (unsigned)tiw[mb * TILE_IO_WORDS + 1];
          ts.ubm = win.ubm; ts.ubm.off = (unsigned)tiw[mb * TILE_IO_WORDS + 2];
          ts.Q = reinterpret_cast<const double*>(cost.Q); ts.Qf = reinterpret_cast<const double*>(cost.Qf);
          ts.R = reinterpret_cast<const double*>(cost.R);
          ts.gb = tgb + mb * TILE_GB_DOUBLES;
          M4Q_PHASE_MARK(3)
          ts.backward((tfl & 1) != 0, timg);
          wave_sync();
          M4Q_PHASE_MARK(1)
        }
        wave_sync();
        issue_prio<PRIO_ON && PRIO.rollout != PRIO.sweep, PRIO.rollout>();
        // the rollout on DPP rows (on tiles it was built twice: round 3's per-index form took 2.3 times as long, round 4's time-batched
        // form - tools/tile_rollout_r04.h - the same SIMD time at d = 3 and 14 % more of the launch at d = 2)
        // (idle lanes sit it out as in the DPP kernels: MASK_IDLE itself is off for TILE because the tile sweep needs all 64 lanes)
        constexpr bool MASK_FWD = NS < 16;
        // (n = 8: two indices per trip on the two halves of the row, all 16 lanes in - rollout_forward_pair, m4q_mpc.h)
        if constexpr (rollout_pair_form<S, NS, NU, false, true, Prov>())
          chk = rollout_forward_pair<NS, NU>(prov, T, x_cur, win, flags, gains, sat, lo0, hi0, Xo, Uo, jj, running, uapp, !use_ls, Xg, Ug);
        else if (!MASK_FWD || lane_ok)         // (the tile path runs with a constant target only)
          chk = rollout_forward<S, NS, NU, false, true>(prov, T, x_cur, win, cost, flags, gains, sat, lo0, hi0, Xo, Uo, j, st, uapp, !use_ls, &Xg, &Ug);
        if constexpr (MASK_FWD) {
          chk = bcast<0>(chk);
#pragma unroll
          for (int k = 0; k < NU; ++k) uapp[k] = bcast<0>(uapp[k]);
        }
      } else if constexpr (!EXACT) {
        // (xbar_t the same for every t: the sweep needs no row form of A_t - wave-uniform choice between two instantiations.
        //  Round 2: n = 16 only - config 4 85.5 -> 84.2 ms, while at n = 9 the kernel with both instantiations was SLOWER, 50.65 -> 51.7 ms,
        //  although it executes 27 vector instructions fewer per horizon index (profiles/r02_ab_experiments.txt).  Round 3, with the
        //  kernel off the register ceiling: n >= 8 - TC_MIN_N above.)
        constexpr bool HAS_TC = NS >= TC_MIN_N && sizeof(S) == sizeof(double);
        bool tc = false;
        if constexpr (HAS_TC) tc = (flags & QP_TARG_CONST) != 0;
        if constexpr (HAS_TC) {
          if (tc && (!MASK_IDLE || lane_ok))
            riccati_backward<S, NS, NU, Prov, false, true>(prov, T, win, cost, flags, gains, j, st);
        }
        M4Q_PHASE_MARK(3)
        if (!tc && (!MASK_IDLE || lane_ok)) riccati_backward<S, NS, NU>(prov, T, win, cost, flags, gains, j, st);
        wave_sync();
        issue_prio<PRIO_ON && PRIO.rollout != PRIO.sweep, PRIO.rollout>();
        M4Q_PHASE_MARK(1)
        if constexpr (HAS_TC && rollout_pair_form<S, NS, NU, false, true, Prov>()) {
          if (tc)           // (the pair form takes all 16 lanes of the row)
            chk = rollout_forward_pair<NS, NU>(prov, T, x_cur, win, flags, gains, sat, lo0, hi0, Xo, Uo, jj, running, uapp, !use_ls, Xg, Ug);
        } else if constexpr (HAS_TC) {
          if (tc && (!MASK_IDLE || lane_ok))
            chk = rollout_forward<S, NS, NU, false, true>(prov, T, x_cur, win, cost, flags, gains, sat, lo0, hi0, Xo, Uo, j, st, uapp,
                                                          !use_ls, &Xg, &Ug);
        }
        if (!tc && (!MASK_IDLE || lane_ok))
          chk = rollout_forward<S, NS, NU, false>(prov, T, x_cur, win, cost, flags, gains, sat, lo0, hi0, Xo, Uo, j, st, uapp,
                                                  !use_ls, &Xg, &Ug);
        if constexpr (MASK_IDLE) {
          // the row's scalars back into the lanes that sat the sweep out
          chk = bcast<0>(chk);
#pragma unroll
          for (int k = 0; k < NU; ++k) uapp[k] = bcast<0>(uapp[k]);
        }
      } else {
        PinCtx<NU> pin;
        pin.stat = pin_stat;
        pin.box.sat = sat;
        pin.tconst = (flags & QP_TARG_CONST) != 0;
#pragma unroll
        for (int k = 0; k < NU; ++k) { pin.lo0[k] = lo0[k]; pin.hi0[k] = hi0[k]; }
        // rows starting a solve: the current SQP guess (the shifted previous solution on warm steps: nearly the right
        // working set), clipped into the box and rolled out through the linearised model.  The linearisation point
        // (Xg, Ug) stays untouched until the solve is over.
        const bool start = running && !qp.busy();
        double J0 = 0.0;
        M4Q_PHASE_MARK(3)
        if (__any(start)) {
          J0 = rollout_open<S, NS, NU>(prov, fresh(T), x_cur, win, cost, Ug, pin.box, lo0, hi0, Xo, Uo, j, start && lane_ok);
          wave_sync();
        }
        M4Q_PHASE_MARK(14)
        bool bad_start = false;
        if (start) {
          qp.begin(J0);
          if (!finite_d(J0)) { qp.busy() = false; bad_start = true; }
        }
        if (__any(qp.busy())) ++qp_passes;
        bool ended;
        if constexpr (exact_tile<S, TL, EXACT>()) {
          // the pinned sweep on tiles: what a row hands to the tile layout (member = (lane >> 2) & 3 there, lane >> 4 here)
          ExactTile<NS> xt;
          xt.lds_models = reinterpret_cast<const double*>(lds);
          xt.tgb = tgb; xt.tiw = tiw; xt.tpin = tpin;
          xt.Xg = Xg; xt.Ug = Ug; xt.gains = gains;
          xt.Q = reinterpret_cast<const double*>(cost.Q); xt.Qf = reinterpret_cast<const double*>(cost.Qf); xt.R = reinterpret_cast<const double*>(cost.R);
          xt.sX = sX; xt.sU = sU; xt.sG = sG;
          xt.g = g; xt.jj = jj;
          ended = box_qp_iterate<S, NS, NU>(prov, fresh(T), x_cur, win, cost, flags, gains, pin, Xo, Uo, Xalt, Ualt, qp, j, jj, lane_ok, &pc, xt);
        } else {
          ended = box_qp_iterate<S, NS, NU>(prov, fresh(T), x_cur, win, cost, flags, gains, pin, Xo, Uo, Xalt, Ualt, qp, j, jj, lane_ok, &pc);
        }
        solved = running && (ended || bad_start);
        capped = solved && !bad_start && qp.stats.end_cap > 0;
        chk = qp.Jk;
        GView Xs = Xo, Us = Uo;
        Xs.off = qp.cur_is_a() ? Xo.off : Xalt.off;
        Us.off = qp.cur_is_a() ? Uo.off : Ualt.off;
        if (solved && jj == 0) {
          M4Q_GLOBAL unsigned long long* cnt = (M4Q_GLOBAL unsigned long long*)kargs()->queue;
          __hip_atomic_fetch_add(cnt + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(cnt + 2, (unsigned long long)qp.stats.sweeps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(cnt + 3, (unsigned long long)qp.stats.ratio_steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(cnt + 4, (unsigned long long)qp.stats.end_kkt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(cnt + 5, (unsigned long long)qp.stats.end_precision, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(cnt + 6, (unsigned long long)qp.stats.end_cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (solved && !bad_start) {
#pragma unroll
          for (int k = 0; k < NU; ++k) uapp[k] = Us.ld<double>(k);
          // (the row's 16 lanes share the contiguous elements; a batch issues all its loads before the first store)
          auto copy_x = [&](const GView& dst, const GView& src, int shift) __attribute__((always_inline)) {
            constexpr int U = 12;
            const int count = (T + 1) * NS, last = T * NS;
            for (int e0 = jj; e0 < count; e0 += 16 * U) {
              S v[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int e = e0 + 16 * u < count ? e0 + 16 * u : count - 1;
                v[u] = src.ld<S>(e < last ? e + shift : e);
              }
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int u = 0; u < U; ++u)
                if (e0 + 16 * u < count) dst.st<S>(e0 + 16 * u, v[u]);
            }
          };
          auto copy_u = [&](const GView& dst, const GView& src, int shift) __attribute__((always_inline)) {
            constexpr int U = 8;
            const int count = T * NU, last = (T - 1) * NU;
            for (int e0 = jj; e0 < count; e0 += 16 * U) {
              double v[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int e = e0 + 16 * u < count ? e0 + 16 * u : count - 1;
                v[u] = src.ld<double>(e < last ? e + shift : e);
              }
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int u = 0; u < U; ++u)
                if (e0 + 16 * u < count) dst.st<double>(e0 + 16 * u, v[u]);
            }
          };
          if (use_ls) {
            if (!qp.cur_is_a()) {
              copy_x(Xo, Xs, 0);
              copy_u(Uo, Us, 0);
            }
          } else {
            // warm step (alpha = 1, mpc.py:208-212): the solution becomes the next guess, shifted (mpc.py:271-272)
            copy_x(Xg, Xs, NS);
            copy_u(Ug, Us, NU);
          }
        }
      }
    }
    wave_sync();
    issue_prio<PRIO_ON && PRIO.line_search != PRIO.rollout, PRIO.line_search>();
    M4Q_PHASE_MARK(EXACT ? 15 : 2)
#if defined(M4Q_DEV_PHASE_CLOCK)
    if (__any(running && !(kargs()->warm_start && step > 1))) pc.count(9);      // passes with a line search
#endif
    // back from the stash
    b = ((long)stash.get_int(g, 1) << 32) | (long)(unsigned)stash.get_int(g, 0);
    code = stash.get_int(g, 2);
    done_steps = stash.get_int(g, 3);
    row_begin = stash.get_int(g, 4);
    {
      const int fl = stash.get_int(g, 5);
      active = (fl & 1) != 0; need_new = (fl & 2) != 0; pending = (fl & 4) != 0;
    }
    op0_off = (unsigned)stash.get_int(g, 6);
    ops_off = (unsigned)stash.get_int(g, 7);
    stash.get_x(x_meas);
    // exit code 3: non-finite objective (mpc.py:200-203).  exit code 2 (EXACT only): the solver gave up - the analogue of
    // the solver warning mpc.py:183-197 turns into code 2; either way the member's run ends here (mpc.py:196,203,231).
    const bool fail = !finite_d(chk) || capped;
    if (solved) ++iter;
    double alpha = 1.0;
    bool fin = true;
    if (__any(solved && use_ls)) {
      KArgs* a = kargs();
      ZView<NS, NU> z;
      z.T = T; z.Xg = Xg; z.Xo = Xo; z.Xt = win.xbm; z.Ug = Ug; z.Uo = Uo; z.Ut = win.ubm;
      double al = 1.0, stepn = 0.0;
      if constexpr (TL) {
        // (the host selects TL only with diagonal costs)
        if constexpr (NS % 2 == 0 && LS_TABLE) {
          // (wave-uniform: the horizon is the launch's)
          if (ls_table::tabled(T, LS_NODES)) line_search_tl_nodes<NX, NU, DD, TILE, true>(z, ldsW, ldsW + 2 * NX, ldsW + 4 * NX, jj, al, stepn, ldsT);
          else line_search_tl_nodes<NX, NU, DD, TILE>(z, ldsW, ldsW + 2 * NX, ldsW + 4 * NX, jj, al, stepn);
        } else if constexpr (NS % 2 == 0) line_search_tl_nodes<NX, NU, DD, TILE>(z, ldsW, ldsW + 2 * NX, ldsW + 4 * NX, jj, al, stepn);
        else line_search_tl<NX, NU, DD>(z, ldsW, ldsW + 2 * NX, ldsW + 4 * NX, jj, al, stepn);
      } else if (ls_diag) {
        line_search_diag<S, NX, NU, DD>(z, ldsW, ldsW + 2 * NX, ldsW + 4 * NX, jj, al, stepn);
      } else {
        if constexpr (sizeof(S) == sizeof(cplx)) line_search<NX, NU>(z, a->Cq, a->Cqf, a->Cr, jj, al, stepn);
      }
      if (use_ls) { alpha = al; fin = stepn < a->ls_tol; }   // mpc.py:224
    }
    wave_sync();
    issue_prio<PRIO_ON && PRIO.update != PRIO.line_search, PRIO.update>();
    M4Q_PHASE_MARK(4)
    const bool upd = solved && !fail && use_ls;       // warm steps wrote the shifted guess in the rollout
    // a row whose SQP step ends with this update (the step-done block below tests the same): its next step starts from
    // shift_guess of the updated guess (mpc.py:71-73,271-272: drop node 0, repeat the last), which is the updated guess stored one
    // node lower - the update stores it there, and no second pass reads and writes the guess again.
    bool shift_now = false;
    if constexpr (SHIFT_IN_UPDATE) {
      KArgs* a = kargs();
      shift_now = upd && (fin || iter >= a->max_iter);
    }
    // Element e of the updated array goes to e - (node width) where e is past node 0, and the last node also to e; rows that go
    // on iterating store at e.  In place this is safe, and what it rests on is this.  Across trips of the loops below: a trip
    // stores at or below the addresses it loaded, never into what a later trip loads.  Within a trip, across lanes: the store
    // of group u to e - n hits an address that ANOTHER lane of the row loads in group u or u - 1 of the same trip (n <= the 16
    // or 32 elements a group spans).  Every load of the trip is issued before its first store (the sched_barrier; the compiler
    // may not sink a load of the same buffer below a store), vector loads return in order, and group u's store waits for
    // group u's own data - so groups <= u have been read by all lanes when it is issued.  An edit that stores before the
    // barrier, shifts by more than one group, or gives the lanes of a row different trips breaks this.
    const int xsh = shift_now ? NS : 0, ush = shift_now ? NU : 0;
    // X_guess += alpha (X_opt - X_guess) (mpc.py:228-229)
    // (these small per-element passes are latency bound: unrolled so that several loads are in flight)
    // (the row's 16 lanes share the (T + 1) NS contiguous elements, and a batch of U elements per lane issues all its loads
    //  before the first store: left to the compiler the unrolled loop waited for every pair in turn - 22,000 cycles per update)
    if constexpr (NS % 2 == 0 && sizeof(S) == sizeof(double)) {
      // (n even: rows of the workspace start on 16-byte boundaries and hold an even number of doubles - two elements per access)
      if (upd) {
        constexpr int U = 6;
        const int count = (T + 1) * NS;
        for (int e0 = 2 * jj; e0 < count; e0 += 32 * U) {
          double xg[U][2], xo[U][2];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int e = e0 + 32 * u < count ? e0 + 32 * u : count - 2;
            ldn<2>(Xg, e, xg[u]);
            ldn<2>(Xo, e, xo[u]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (e0 + 32 * u < count) {
              double r[2];
#pragma unroll
              for (int h = 0; h < 2; ++h) r[h] = cadd(xg[u][h], cscale(csub(xo[u][h], xg[u][h]), alpha));
              const int e = e0 + 32 * u;               // (NS even: a pair lies within one node)
              if (e >= xsh) stn<2>(Xg, e - xsh, r);
              if (shift_now && e >= T * NS) stn<2>(Xg, e, r);
            }
          }
        }
      }
    } else if (upd) {
      constexpr int U = 12;
      const int count = (T + 1) * NS;
      for (int e0 = jj; e0 < count; e0 += 16 * U) {
        S xg[U], xo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = e0 + 16 * u < count ? e0 + 16 * u : count - 1;
          xg[u] = Xg.ld<S>(e);
          xo[u] = Xo.ld<S>(e);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (e0 + 16 * u < count) {
            const S r = cadd(xg[u], cscale(csub(xo[u], xg[u]), alpha));
            const int e = e0 + 16 * u;
            if (e >= xsh) Xg.st<S>(e - xsh, r);
            if (shift_now && e >= T * NS) Xg.st<S>(e, r);
          }
        }
      }
    }
    if constexpr (NU % 2 == 0) {
      if (upd) {
        constexpr int V = 4;
        const int cu = T * NU;
        for (int e0 = 2 * jj; e0 < cu; e0 += 32 * V) {
          double ug[V][2], uo[V][2];
#pragma unroll
          for (int u = 0; u < V; ++u) {
            const int e = e0 + 32 * u < cu ? e0 + 32 * u : cu - 2;
            ldn<2>(Ug, e, ug[u]);
            ldn<2>(Uo, e, uo[u]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < V; ++u) {
            if (e0 + 32 * u < cu) {
              double r[2];
#pragma unroll
              for (int h = 0; h < 2; ++h) r[h] = ug[u][h] + alpha * (uo[u][h] - ug[u][h]);
              const int e = e0 + 32 * u;
              if (e >= ush) stn<2>(Ug, e - ush, r);
              if (shift_now && e >= (T - 1) * NU) stn<2>(Ug, e, r);
            }
          }
        }
      }
    } else if (upd) {
      {
        constexpr int V = 8;
        const int cu = T * NU;
        for (int e0 = jj; e0 < cu; e0 += 16 * V) {
          double ug[V], uo[V];
#pragma unroll
          for (int u = 0; u < V; ++u) {
            const int e = e0 + 16 * u < cu ? e0 + 16 * u : cu - 1;
            ug[u] = Ug.ld<double>(e);
            uo[u] = Uo.ld<double>(e);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < V; ++u) {
            if (e0 + 16 * u < cu) {
              const double r = ug[u] + alpha * (uo[u] - ug[u]);
              const int e = e0 + 16 * u;
              if (e >= ush) Ug.st<double>(e - ush, r);
              if (shift_now && e >= (T - 1) * NU) Ug.st<double>(e, r);
            }
          }
        }
      }
    }
    wave_sync();
    issue_prio<PRIO_ON && PRIO.step_done != PRIO.update, PRIO.step_done>();

    M4Q_PHASE_MARK(8)
    // ---- rows that finished their MPC step: apply, propagate, shift (where the guess update has not) ----
    bool step_done;
    {
      KArgs* a = kargs();
      step_done = solved && (fail || fin || iter >= a->max_iter);
    }
    if (__any(step_done)) {
      KArgs* a = kargs();
      const int mf = a->measure_freq, n_steps = a->n_steps;
      const long sXs = (long)(n_steps + 1) * NX, sUs = (long)n_steps * NU;
      if (step_done && fail) code = finite_d(chk) ? 2 : 3;
      if (step_done && jj == 0) gst(a->qp_solves, b * n_steps + step, iter);
      const bool ok = step_done && !fail;
      // apply U_opt[:, 0] (mpc.py:250), propagate the plant (mpc.py:256-260)
      if (ok) {
#pragma unroll
        for (int k = 0; k < NU; ++k) uprev[k] = step >= 1 ? uapp[k] : uprev[k];     // (step 1 still takes U_ref[:, 0]: mpc.py:185)
        if (jj == 0) {
#pragma unroll
          for (int k = 0; k < NU; ++k) gst(a->us, b * sUs + (long)step * NU + k, uapp[k]);
        }
      }
      M4Q_PHASE_MARK_CLIP(10)
      if constexpr (PLANT != PLANT_NONE) {
        // (step+1) % measure_freq == 0: propagate the plant from the last measured state over the last measure_freq
        // intervals (mpc.py:252-260); the held controls are stacked newest first against an increasing time grid
        // (:257), i.e. replayed in reversed order.  Otherwise the model closes the loop (mpc.py:261-267).
        const bool measure = (step + 1) % mf == 0;
        cplx xn = czero();
        if (__any(ok && measure)) {
          GView op0 = gview(a->plant.op0, 0, 0), ops = gview(a->plant.ops, 0, 0);
          op0.off = op0_off;
          ops.off = ops_off;
          const double dt = a->dt;
          cplx xc = Basis<S, TL>::template to_complex<NX, DD>(x_meas, tau, scratch, j, jj);
          wave_sync();
          for (int i = 0; i < mf; ++i) {
            double ui[NU];
#pragma unroll
            for (int k = 0; k < NU; ++k)
              ui[k] = (i == 0 || !(ok && measure)) ? uapp[k] : gld(a->us, b * sUs + (long)(step - i) * NU + k);
            M4Q_PLANT_STEP(PLANT, xc, xc, ui, op0, ops, dt, scratch, jio, jj);
          }
          xn = xc;
          // measurement noise (m4q_session_set_noise; m4q_noise.h): added to the measured state in complex original-basis form, so
          // that it is stored, converted and carried like the plant's own result and the exit condition below reads it back.  Lanes
          // that shadow column NX - 1 draw that column's noise (jio) and store nothing.  Mode 0: one scalar branch.
          const int nmode = a->noise_mode;
          if (nmode != 0) {
            const bool add = ok && measure;
            const double sg = add ? gld(a->noise_sigma, b * a->noise_sigma_stride) : 0.0;
            const cplx e = noise_sample(nmode, a->noise_seed, a->noise_member_base + (unsigned long long)b, (unsigned)(step + 1), jio,
                                        SQUARE ? DD : 0, sg);
            if (add) xn = cadd(xn, e);
          }
        }
        double tnew = 0.0;
        S rn = Basis<S, TL>::template to_state<NX, DD>(xn, scratch, j, jj, tnew);
        if (mf > 1 && __any(ok && !measure)) {
          typename Prov::Lin lin;
#pragma unroll
          for (int k = 0; k < NU; ++k) lin.u[k] = SG ? uapp[k] * gsc[k] : uapp[k];        // (SG: the provider works on the scaled controls)
          lin.xg = x_cur;
          S pred, Bdummy[NU], ddummy;
          prov.rows(lin, x_cur, pred, Bdummy, ddummy);                 // A x + N (polyu (x) x) = A_t(u) x  (model.py:81-93)
          const cplx pc = Basis<S, TL>::template to_complex<NX, DD>(pred, tau, scratch, j, jj);
          if (!measure) { rn = pred; xn = pc; }
        }
        if (ok) x_cur = rn;
        if (ok && measure) { x_meas = rn; if constexpr (TL) tau = tnew; }
        if (ok && lane_io) gst(a->xs, b * sXs + (long)(step + 1) * NX + jio, xn);
      }
      M4Q_PHASE_MARK_CLIP(11)
      // shift_guess (mpc.py:71-73,271-272): drop column 0, repeat the last.  SHIFT_IN_UPDATE: the guess update above stored this
      // row's guess one node down already (a warm step's rollout did); else a second pass, here
      if constexpr (!SHIFT_IN_UPDATE) {
        const bool shift_late = ok && use_ls;
        if (shift_late && lane_ok) {
          for (int t0 = 0; t0 < T; t0 += 8) {
            S buf[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) buf[q] = Xg.ld<S>((t0 + q + 1 <= T ? t0 + q + 1 : T) * NS + j);
#pragma unroll
            for (int q = 0; q < 8; ++q)
              if (t0 + q < T) Xg.st<S>((t0 + q) * NS + j, buf[q]);
          }
        }
        if (shift_late && jj < NU) {
          for (int t0 = 0; t0 + 1 < T; t0 += 8) {
            double buf[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) buf[q] = Ug.ld<double>((t0 + q + 1 < T ? t0 + q + 1 : T - 1) * NU + jj);
#pragma unroll
            for (int q = 0; q < 8; ++q)
              if (t0 + q + 1 < T) Ug.st<double>((t0 + q) * NU + jj, buf[q]);
          }
        }
      }
      if (ok) done_steps = step + 1;
      if (step_done) {
        iter = 0;
        step = fail ? row_end : step + 1;
      }
      if constexpr (PLANT != PLANT_NONE) {
        // exit condition (m4q_session_set_exit), once the step is complete: q = Re((x - f)^H W (x - f)) of the state just stored
        // (NEXT: xs[step + 1] - the plant's, or the model's on a step that is not measured) or of the one the step started from
        // (PREV: xs[step], x0 at step 0), read back as stored: complex, original basis, on every path.  A row it fires for ends its
        // run with code 1 and steps_done = the step just taken, whose entries are dropped (mpc.py:289-304).  Mode 0: one scalar branch.
        const int xmode = a->exit_mode;
        if (xmode != 0) {
          const int s0 = step - 1;                                 // (ok rows: the step just completed)
          const bool prev = (xmode & EXIT_PREV) != 0;
          const cplx x = !ok ? czero() : (prev && s0 == 0) ? gld(a->x0c, b * NX + jio)
                                                           : gld(a->xs, b * sXs + (long)(prev ? s0 : s0 + 1) * NX + jio);
          const cplx d = csub(x, ok ? gld(a->exit_target, b * a->exit_tstride + jio) : czero());
          // (quad_figure<NX>, spelled out: through it two exact kernels of the (16, 3, 1) shape compile to other code)
          const M4Q_GLOBAL cplx* Wr = a->exit_W + jio * NX;       // row jio of W (shared, small) against the row's d
          cplx y = czero();
          static_for<0, NX>([&](auto k) { cmac(y, gld(Wr, decltype(k)::value), bcast<decltype(k)::value>(d)); });
          const double q = rowsum<NX>(dot_re(d, y));
          const double thr = ok ? gld(a->exit_thr, b * a->exit_thr_stride) : 0.0;
          if (ok && ((xmode & EXIT_ABOVE) ? q > thr : q < thr)) {
            code = 1;
            done_steps = s0;
            step = row_end;
          }
        }
      }
      wave_sync();
      if constexpr (PLANT == PLANT_NONE) {
        // the caller writes xs[step+1] before the next launch; inside one launch carry what is there
        const bool carry = ok && step < row_end;
        const cplx xc = carry ? gld(a->xs, b * sXs + (long)step * NX + jio) : czero();
        double tnew = 0.0;
        const S rn = Basis<S, TL>::template to_state<NX, DD>(xc, scratch, j, jj, tnew);
        if (carry) { x_cur = rn; if constexpr (TL) tau = tnew; }
      }
      M4Q_PHASE_MARK_CLIP(13)
    }

    issue_prio<PRIO_ON && PRIO.publish != PRIO.step_done, PRIO.publish>();
    M4Q_PHASE_MARK(5)
    // ---- rows that finished their item: publish the resumable state, free the slot ----
    const bool finished = active && step >= row_end;
    if (__any(finished)) {
      KArgs* a = kargs();
      // The last item of an instance publishes the guess as the host sees it: complex, original basis (eight nodes' loads in flight
      // at once; the basis change of each goes through LDS).  An earlier item's guess is only ever read by the next item of the same
      // launch: on the real paths it goes into the same field as it is (PIECE_RAW: (T + 1) NS doubles, flat) - 41 basis changes less
      // on either side of every cut, and no rounding at the cuts.
      const bool last_piece = row_end == a->step_end;
      if constexpr (TL && NS % 2 == 0) {
        // (traceless path, n_s even: one trajectory node per lane - its coordinates as 16-byte pairs, its NX slots formed and stored
        //  by that lane (tl_node_to_complex) - instead of a slot per lane with an exchange through LDS per node)
        if (finished && last_piece) {
          for (int t = jj; t <= T; t += 16) {
            double r[NS];
#pragma unroll
            for (int h = 0; h < NS / 2; ++h) {
              double p2[2];
              ldn<2>(Xg, (unsigned)(t * NS + 2 * h), p2);
              r[2 * h] = p2[0]; r[2 * h + 1] = p2[1];
            }
            cplx out[NX];
            tl_node_to_complex<NX, DD>(r, tau, out);
#pragma unroll
            for (int c = 0; c < NX; ++c) gst(a->Xg, b * sXc + t * NX + c, out[c]);
          }
        }
      } else if (__any(finished && (!PIECE_RAW || last_piece))) {
        for (int t0 = 0; t0 <= T; t0 += 8) {
          S v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = Xg.ld<S>((t0 + q <= T ? t0 + q : T) * NS + j);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            if (t0 + q <= T) {
              const cplx xc = Basis<S, TL>::template to_complex<NX, DD>(v[q], tau, scratch, j, jj);
              if (finished && (!PIECE_RAW || last_piece) && lane_io) gst(a->Xg, b * sXc + (t0 + q) * NX + jio, xc);
            }
          }
        }
      }
      if constexpr (PIECE_RAW) {
        if (finished && !last_piece) {
          M4Q_GLOBAL double* raw = (M4Q_GLOBAL double*)(a->Xg + b * sXc);
          const int count = (T + 1) * NS;
          if constexpr (NS % 2 == 0) {
            constexpr int U = 6;
            for (int e0 = 2 * jj; e0 < count; e0 += 32 * U) {
              double v[U][2];
#pragma unroll
              for (int u = 0; u < U; ++u) ldn<2>(Xg, e0 + 32 * u < count ? e0 + 32 * u : count - 2, v[u]);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int u = 0; u < U; ++u) {
                if (e0 + 32 * u < count) {
                  d2_t w; w.x = v[u][0]; w.y = v[u][1];
                  *reinterpret_cast<M4Q_GLOBAL d2_t*>(raw + e0 + 32 * u) = w;
                }
              }
            }
          } else {
            constexpr int U = 12;
            for (int e0 = jj; e0 < count; e0 += 16 * U) {
              double v[U];
#pragma unroll
              for (int u = 0; u < U; ++u) v[u] = Xg.ld<double>(e0 + 16 * u < count ? e0 + 16 * u : count - 1);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int u = 0; u < U; ++u)
                if (e0 + 16 * u < count) gst(raw, e0 + 16 * u, v[u]);
            }
          }
        }
      }
      if (finished) {
        for (int e = jj; e < T * NU; e += 16) gst(a->Ug, b * sU + e, Ug.ld<double>(e));
        if (jj == 0) {
          gst(a->codes, b, code);
          gst(a->steps_done, b, done_steps);
        }
      }
      if (two_phase && __any(finished && row_end != kargs()->step_end)) {
        // head item: make the state visible to whichever workgroup draws the tail (G16: stores drained,
        // agent-scope release, drained again, then the flag)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wave_sync();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (finished && row_end != a->step_end && jj == 0)
          __hip_atomic_store(a->head_done + b, piece_of(row_begin, a->step_begin) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (finished) {
        active = false;
        need_new = true;
      }
      wave_sync();
    }
    M4Q_PHASE_MARK(6)
    pc.count(7);
    // back to level 0 (the level a wavefront starts at) before the pass ends, so that every way round the loop arrives there at 0:
    // the watchdog exit, the draw (atomics and waits: memory latency, not issue), the final break and a wavefront that only polls
    // - a poller must not outrank the head it waits for - all run between here and the first switch of the next pass
    issue_prio<PRIO_ON, 0>();
  }
}

#ifndef M4Q_VARIANT_GEN
// ---------------------------------------------------------------------------------------------
// Open-loop rollouts (RollArgs): what a member stores of column t of its trajectory - the state, and / or the figure
// q = Re((x - f)^H W (x - f)) (quad_figure, as the exit condition of mpc_kernel).
// The modes and t are wave-uniform: branches on them keep all 64 lanes active for the broadcasts; the stores are masked.
struct RollOut {
  int N, xs_mode, q_mode;
  M4Q_GLOBAL cplx* xs; M4Q_GLOBAL double* q;
  const M4Q_GLOBAL cplx* Wr;        // row j of W
  cplx f;                           // this lane's entry of the member's f
  long b;
  int j;
  bool st, st0;                     // this lane stores its state entry / its row's figure
  __device__ __forceinline__ RollOut(const RollArgs& a, long b_, int j_, bool st_, bool st0_)
      : N(a.N), xs_mode(a.xs_mode), q_mode(a.q_mode), xs(a.xs), q(a.q), Wr(a.W + j_ * NX), f(czero()), b(b_), j(j_), st(st_), st0(st0_) {
    if (q_mode != 0) f = gld(a.target, b * a.target_stride + j);
  }
  __device__ __forceinline__ void put(int t, cplx x) const {
    const bool last = t == N;
    if (xs_mode == 2) {
      if (st) gst(xs, (b * (N + 1) + t) * NX + j, x);
    } else if (xs_mode == 1 && last) {
      if (st) gst(xs, b * NX + j, x);
    }
    if (q_mode == 2 || (q_mode == 1 && last)) {
      const double qv = quad_figure<NX>(csub(x, f), Wr);
      if (st0) gst(q, q_mode == 2 ? b * (N + 1) + t : b, qv);
    }
  }
};
// the controls of one step as the member sees them: u_scale[b][k] u[t][k], formed here in fp64
struct RollCtl {
  const M4Q_GLOBAL double* u;      // the member's (or the shared) sequence [N][NU]
  double sc[NU], un[NU];
  int N;
  __device__ __forceinline__ RollCtl(const RollArgs& a, long b) : u(a.u + b * a.u_stride), N(a.N) {
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      sc[k] = a.u_scale ? gld(a.u_scale, b * NU + k) : 1.0;
      un[k] = gld(u, k);
    }
  }
  // the controls of step t (fetched one step ago); issues the loads of step t + 1, which the arithmetic of step t then covers
  __device__ __forceinline__ void take(int t, double (&ut)[NU]) {
    const int tn = t + 1 < N ? t + 1 : t;
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      ut[k] = sc[k] * un[k];
      un[k] = gld(u, (long)tn * NU + k);
    }
  }
};

// Feedback runs (FeedbackArgs; m4q_feedback.h): what a member leaves besides its trajectory - the commanded controls of every
// step, and at its end the count of active bounds and the status (3: a state or a control was not finite).  A lane watches its own
// entry of the state; the controls are the same in every lane of the row.
struct FeedbackOut {
  M4Q_GLOBAL double* us; M4Q_GLOBAL int* clipped; M4Q_GLOBAL int* status;
  long b;
  int N;
  bool st0;
  bool bad;
  __device__ __forceinline__ FeedbackOut(const FeedbackArgs& a, long b_, bool st0_)
      : us(a.us), clipped(a.clipped), status(a.status), b(b_), N(a.roll.N), st0(st0_), bad(false) {}
  __device__ __forceinline__ void state(cplx x) { bad = bad || !finite_d(x.re) || !finite_d(x.im); }
  __device__ __forceinline__ void controls(int t, const double (&u)[NU]) const {
    if (us != nullptr && st0) {
#pragma unroll
      for (int k = 0; k < NU; ++k) gst(us, (b * N + t) * NU + k, u[k]);
    }
  }
  __device__ __forceinline__ void finish(const FeedbackRow<NX, NU>& law) const {
    const bool lost = rowsum<NX>(bad ? 1.0 : 0.0) != 0.0 || law.bad;
    if (st0) {
      gst(status, b, lost ? 3 : 0);
      if (clipped != nullptr) gst(clipped, b, law.clipped);
    }
  }
};
// ... and the measurement noise of column t + 1, added to the state the step left (m4q_noise.h; as mpc_kernel's step-done phase:
// out of line, behind one scalar branch on the mode; lanes that shadow column NX - 1 draw that column's noise)
struct FeedbackNoise {
  int mode;
  unsigned long long seed, member;
  double sg;
  __device__ __forceinline__ FeedbackNoise(const FeedbackArgs& a, long b)
      : mode(a.noise_mode), seed(a.seed), member(a.member_base + (unsigned long long)b), sg(0.0) {
    if (mode != 0) sg = gld(a.sigma, b * a.sigma_stride);
  }
  __device__ __forceinline__ cplx add(int t, cplx x, int j) const {
    if (mode != 0) x = cadd(x, noise_sample(mode, seed, member, (unsigned)(t + 1), j, SQUARE ? DD : 0, sg));
    return x;
  }
};

// Rollout gradients (GradArgs; m4q_grad.h): the controls of step t as the member saw them in the forward pass - the same product
template <class A>
__device__ __forceinline__ void grad_controls(const RollCtl& ctl, int t, A& v) {
#pragma unroll
  for (int k = 0; k < NU; ++k) v[k] = ctl.sc[k] * gld(ctl.u, (long)t * NU + k);
}
// ... what the backward pass leaves of step t: ge[t][k] = Re(lam_{t+1}^H dx_{t+1}/dv_k), parked in the member's grad [N][m]
__device__ __forceinline__ void grad_park(const GradArgs& ga, long b, int t, const double (&ge)[NU], bool st0) {
  if (st0) {
#pragma unroll
    for (int k = 0; k < NU; ++k) gst(ga.grad, (b * ga.roll.N + t) * NU + k, ge[k]);
  }
}
// ... and the pass over them with t ascending that ends a member: grad[t][k] = u_scale[k] ge[t][k], grad_scale[k] = sum_t u[t][k] ge[t][k]
__device__ __forceinline__ void grad_finish(const GradArgs& ga, const RollCtl& ctl, long b, bool st0) {
  wave_sync();
  double gs[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) gs[k] = 0.0;
  for (int t = 0; t < ga.roll.N; ++t) {
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const long idx = (b * ga.roll.N + t) * NU + k;
      const double gek = gld(ga.grad, idx);
      double prod = gld(ctl.u, (long)t * NU + k) * gek;      // rounded before the add, as grad.py adds it (the empty asm keeps
      asm volatile("" : "+v"(prod));                         // the compiler from contracting the two into an FMA)
      gs[k] = gs[k] + prod;
      if (st0) gst(ga.grad, idx, ctl.sc[k] * gek);
    }
  }
  if (st0 && ga.grad_scale) {
#pragma unroll
    for (int k = 0; k < NU; ++k) gst(ga.grad_scale, b * NU + k, gs[k]);
  }
}

// One pass of the ordered ensemble reduction of the gradients (shape-independent)
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradReduceArgs a) { grad_reduce(a); }
#endif  // M4Q_VARIANT_GEN

#ifndef M4Q_NO_AUX          // (a plant-only shape - m4q_shapes.inc - builds plant_kernel alone; the generator-plant object none of these)
// ---------------------------------------------------------------------------------------------
// WrapModel.get_model_along_traj for B trajectories (linearize.py:61-70)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) M4Q_OCC void linearize_kernel(LinArgs a) {
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* mdl = lds + g * MODEL_ELEMS;
  const int nquads = quads_of(a.B);
  const unsigned sX = (unsigned)a.T * NX, sU = (unsigned)a.T * NU;
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    wave_sync();
    stage_model<NX>(mdl, a.models + r.b * a.model_stride, jj);
    wave_sync();
    FusedProv<cplx, NX, NU, ORDER> prov;
    prov.mdl = mdl;
    prov.Xg = gview(a.X, r.q0 * sX, r.gl * sX);
    prov.Ug = gview(a.U, r.q0 * sU, r.gl * sU);
    prov.j = j;
    const GView Ao = gview(a.A_ls, r.q0 * sX * NX, r.gl * sX * NX);
    const GView Bo = gview(a.B_ls, r.q0 * sX * NU, r.gl * sX * NU);
    const GView Do = gview(a.D_ls, r.q0 * sX, r.gl * sX);
    for (int t = 0; t < a.T; ++t) {
      const auto lin = prov.fetch(t);
      cplx Ac[NX];
      prov.col(lin, Ac);
      cplx av, Brow[NU], dlt;
      prov.rows(lin, czero(), av, Brow, dlt);
      if (r.valid && L.lane_ok) {
#pragma unroll
        for (int i = 0; i < NX; ++i) Ao.st<cplx>((t * NX + i) * NX + j, Ac[i]);
#pragma unroll
        for (int k = 0; k < NU; ++k) Bo.st<cplx>((t * NX + j) * NU + k, Brow[k]);
        Do.st<cplx>(t * NX + j, dlt);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Open-loop rollout of B models over N steps (model.py:81-93: x+ = A [x ; lift_u(u) (x) x]), one launch: the member's model (or
// the shared one) staged in LDS as above, the state in registers, each step the call mpc_kernel makes for a step that is not
// measured.  Complex path.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) M4Q_OCC void model_rollout_kernel(RollArgs a) {
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* mdl = lds + g * MODEL_ELEMS;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    wave_sync();
    stage_model<NX>(mdl, a.models + r.b * a.model_stride, jj);
    wave_sync();
    FusedProv<cplx, NX, NU, ORDER> prov;
    prov.mdl = mdl;
    prov.Xg = prov.Ug = gview(a.x0, 0, 0);         // (rows() reads neither)
    prov.j = j;
    const RollOut out(a, r.b, j, r.valid && L.lane_ok, r.valid && jj == 0);
    RollCtl ctl(a, r.b);
    cplx x = gld(a.x0, r.b * NX + j);
    out.put(0, x);
    for (int t = 0; t < a.N; ++t) {
      FusedProv<cplx, NX, NU, ORDER>::Lin lin;
      ctl.take(t, lin.u);
      lin.xg = x;
      cplx pred, Bdummy[NU], ddummy;
      prov.rows(lin, x, pred, Bdummy, ddummy);      // A x + N (polyu (x) x) = A_t(u) x
      x = pred;
      out.put(t + 1, x);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// model_rollout_kernel with a stored law closing the loop (m4q_model_feedback_batch; feedback.py: model_feedback_reference is the
// definition): the controls of step t come from the state in registers (FeedbackRow), the step is that kernel's.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) M4Q_OCC void model_feedback_kernel(FeedbackArgs fa) {
  const RollArgs& a = fa.roll;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* mdl = lds + g * MODEL_ELEMS;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    wave_sync();
    stage_model<NX>(mdl, a.models + r.b * a.model_stride, jj);
    wave_sync();
    FusedProv<cplx, NX, NU, ORDER> prov;
    prov.mdl = mdl;
    prov.Xg = prov.Ug = gview(a.x0, 0, 0);         // (rows() reads neither)
    prov.j = j;
    const bool st0 = r.valid && jj == 0;
    const RollOut out(a, r.b, j, r.valid && L.lane_ok, st0);
    FeedbackRow<NX, NU> law(fa, r.b, j);
    FeedbackOut fo(fa, r.b, st0);
    const FeedbackNoise noise(fa, r.b);
    cplx x = gld(a.x0, r.b * NX + j);
    fo.state(x);
    out.put(0, x);
    for (int t = 0; t < a.N; ++t) {
      FusedProv<cplx, NX, NU, ORDER>::Lin lin;
      double u[NU];
      law.take(t, x, u, lin.u);
      fo.controls(t, u);
      lin.xg = x;
      cplx pred, Bdummy[NU], ddummy;
      prov.rows(lin, x, pred, Bdummy, ddummy);      // A x + N (polyu (x) x) = A_t(u) x
      x = noise.add(t, pred, j);
      fo.state(x);
      out.put(t + 1, x);
    }
    fo.finish(law);
  }
}

// ---------------------------------------------------------------------------------------------
// Control gradient of an open-loop model rollout (m4q_model_rollout_grad_batch; grad.py: model_rollout_grad_reference is the
// definition).  The forward pass is model_rollout_kernel's, statement for statement, with every state kept in the workspace
// a.xs [B][N + 1][n]; the backward pass reads x_t back and takes dx_{t+1}/dv_k from rows() (Brow) and A(v_t)^H lam from col().
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) M4Q_OCC void model_rollout_grad_kernel(GradArgs ga) {
  const RollArgs& a = ga.roll;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* mdl = lds + g * MODEL_ELEMS;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    wave_sync();
    stage_model<NX>(mdl, a.models + r.b * a.model_stride, jj);
    wave_sync();
    FusedProv<cplx, NX, NU, ORDER> prov;
    prov.mdl = mdl;
    prov.Xg = prov.Ug = gview(a.x0, 0, 0);         // (rows() and col() read neither)
    prov.j = j;
    const bool st0 = r.valid && jj == 0;
    const RollOut out(a, r.b, j, r.valid && L.lane_ok, st0);
    RollCtl ctl(a, r.b);
    cplx x = gld(a.x0, r.b * NX + j);
    out.put(0, x);
    for (int t = 0; t < a.N; ++t) {
      FusedProv<cplx, NX, NU, ORDER>::Lin lin;
      ctl.take(t, lin.u);
      lin.xg = x;
      cplx pred, Bdummy[NU], ddummy;
      prov.rows(lin, x, pred, Bdummy, ddummy);
      x = pred;
      out.put(t + 1, x);
    }
    wave_sync();                                   // the states of this member are in the workspace
    const M4Q_GLOBAL cplx* xw = a.xs + r.b * (a.N + 1) * NX;
    cplx lam = figure_grad<NX>(csub(x, out.f), a.W, j);
    for (int t = a.N - 1; t >= 0; --t) {
      FusedProv<cplx, NX, NU, ORDER>::Lin lin;
      grad_controls(ctl, t, lin.u);
      const cplx xt = gld(xw, (long)t * NX + j);
      lin.xg = xt;
      cplx av, Brow[NU], dlt, Ac[NX];
      prov.rows(lin, czero(), av, Brow, dlt);      // Brow[k] = (df/du_k)_j at (x_t, v_t)
      prov.col(lin, Ac);                           // column j of A(v_t)
      double ge[NU];
#pragma unroll
      for (int k = 0; k < NU; ++k) ge[k] = rowsum<NX>(dot_re(lam, Brow[k]));
      lam = matvec_h<NX>(Ac, lam);
      if (a.q_mode == 2) lam = cadd(lam, figure_grad<NX>(csub(xt, out.f), a.W, j));
      grad_park(ga, r.b, t, ge, st0);
    }
    grad_finish(ga, ctl, r.b, st0);
  }
}

// model_rollout_multi_kernel: S sequences shared by the ensemble through all members' models in one launch, the members' objectives
// alone (m4q_model_rollout_multi_batch; the line search of m4q_model_robust_batch)
#include "m4q_model_multi.h"

// ---------------------------------------------------------------------------------------------
// DMDc identification of B members (m4q_dmdc_fit_batch; fit.py: dmdc_fit_reference is the definition): one wavefront per member,
// grid-stride over members; the Gram data, the eigenvectors and the eigenvalues in dynamic LDS (FitLayout, m4q_fit.h).
// ---------------------------------------------------------------------------------------------
template <int NX_, int NU_, int ORDER_>
__global__ __launch_bounds__(64) void dmdc_fit_kernel(FitArgs a) {
  using L = FitLayout<NX_, NU_, ORDER_>;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const int lane = threadIdx.x;
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    wave_sync();                                   // the previous member's reads are done
    const bool finite = fit_accumulate<NX_, NU_, ORDER_>(a, b, lds, lane);
    bool converged = true;
    if (uniform(finite)) converged = fit_jacobi<L::NZ, L::PITCH>(lds + L::G, lds + L::V, lane);
    if (a.svals) fit_svals<NX_, NU_, ORDER_>(a, b, lds, lane, finite);
    fit_models<NX_, NU_, ORDER_>(a, b, lds, lane, finite);
    if (lane == 0) gst(a.status, b, !finite ? 3 : converged ? 0 : 1);
  }
}

// ---------------------------------------------------------------------------------------------
// DMDc identification of B members from a QR of their data (m4q_dmdc_fit_qr_batch; fit.py: dmdc_fit_qr_reference is the
// definition): the frame and the LDS layout of dmdc_fit_kernel, R, V and T in the places of G, V and C (m4q_fit_qr.h).
// ---------------------------------------------------------------------------------------------
template <int NX_, int NU_, int ORDER_>
__global__ __launch_bounds__(64) void dmdc_fit_qr_kernel(FitArgs a) {
  using L = FitLayout<NX_, NU_, ORDER_>;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const int lane = threadIdx.x;
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    wave_sync();                                   // the previous member's reads are done
    const bool finite = fit_qr_factor<NX_, NU_, ORDER_>(a, b, lds, lane);
    bool converged = true;
    if (uniform(finite)) converged = fit_qr_jacobi<L::NZ, L::PITCH>(lds + L::G, lds + L::V, lane);
    fit_qr_models<NX_, NU_, ORDER_>(a, b, lds, lane, finite);
    if (lane == 0) gst(a.status, b, !finite ? 3 : converged ? 0 : 1);
  }
}

// ---------------------------------------------------------------------------------------------
// The two fits against a prior model (m4q_dmdc_refit_batch, m4q_dmdc_refit_qr_batch; fit.py's last part is the definition): the
// kernels above with the REFIT parts of their device functions (m4q_fit.h, m4q_fit_qr.h), the same LDS layout.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ FitPrior fit_prior(const RefitArgs& a, long b) {
  const int steps = a.counts ? gld(a.counts, b) : a.fit.N;
  return FitPrior{a.A0 + b * a.A0_stride, __builtin_amdgcn_readfirstlane(steps), gld(a.discount, b * a.discount_stride)};
}

template <int NX_, int NU_, int ORDER_>
__global__ __launch_bounds__(64) void dmdc_refit_kernel(RefitArgs a) {
  using L = FitLayout<NX_, NU_, ORDER_>;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const int lane = threadIdx.x;
  for (long b = blockIdx.x; b < a.fit.B; b += gridDim.x) {
    wave_sync();                                   // the previous member's reads are done
    const FitPrior pr = fit_prior(a, b);
    const bool finite = fit_accumulate<NX_, NU_, ORDER_, true>(a.fit, b, lds, lane, pr);
    bool converged = true;
    if (uniform(finite)) converged = fit_jacobi<L::NZ, L::PITCH>(lds + L::G, lds + L::V, lane);
    if (a.fit.svals) fit_svals<NX_, NU_, ORDER_, true>(a.fit, b, lds, lane, finite, pr);
    fit_models<NX_, NU_, ORDER_, true>(a.fit, b, lds, lane, finite, pr);
    if (lane == 0) gst(a.fit.status, b, !finite ? 3 : converged ? 0 : 1);
  }
}

template <int NX_, int NU_, int ORDER_>
__global__ __launch_bounds__(64) void dmdc_refit_qr_kernel(RefitArgs a) {
  using L = FitLayout<NX_, NU_, ORDER_>;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const int lane = threadIdx.x;
  for (long b = blockIdx.x; b < a.fit.B; b += gridDim.x) {
    wave_sync();                                   // the previous member's reads are done
    const FitPrior pr = fit_prior(a, b);
    const bool finite = fit_qr_factor<NX_, NU_, ORDER_, true>(a.fit, b, lds, lane, pr);
    bool converged = true;
    if (uniform(finite)) converged = fit_qr_jacobi<L::NZ, L::PITCH>(lds + L::G, lds + L::V, lane);
    fit_qr_models<NX_, NU_, ORDER_, true>(a.fit, b, lds, lane, finite, pr);
    if (lane == 0) gst(a.fit.status, b, !finite ? 3 : converged ? 0 : 1);
  }
}

// ---------------------------------------------------------------------------------------------
// Recursive DMDc updates of B members (m4q_online_dmdc_batch; online.py: online_dmdc_reference is the definition): the frame of
// dmdc_fit_kernel, the model A and the inverse Gram matrix P in dynamic LDS from the first snapshot to the last (OnlineLayout,
// m4q_online.h).  HERM_: the conjugated form.
// ---------------------------------------------------------------------------------------------
template <int NX_, int NU_, int ORDER_, bool HERM_>
__global__ __launch_bounds__(64) void online_dmdc_kernel(OnlineArgs a) {
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const int lane = threadIdx.x;
  for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
    wave_sync();                                   // the previous member's reads are done
    online_load<NX_, NU_, ORDER_>(a, b, lds, lane);
    const int steps = a.counts ? gld(a.counts, b) : a.N;
    const double inv_discount = 1.0 / gld(a.discount, b * a.discount_stride);
    const bool data_ok = online_updates<NX_, NU_, ORDER_, HERM_>(a, b, steps, inv_discount, lds, lane);
    wave_sync();
    online_store<NX_, NU_, ORDER_>(a, b, steps, data_ok, lds, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// quad_program for B explicit linear time-varying problems (optimize.py:12-60 / lqr.py:14-79)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) M4Q_OCC void qp_kernel(QpArgs a) {
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  const int T = a.T;
  const int nquads = quads_of(a.B);
  CostRef<cplx> cost;
  // (stage costs of the explicit QP stay in global memory: generic pointers the compiler traces back to the kernel argument)
  cost.Q = (const cplx*)a.Q_ls; cost.Qf = (const cplx*)a.Q_ls + (long)T * NX * NX; cost.q_stride = (long)NX * NX;
  cost.R = (const cplx*)a.R_ls; cost.r_stride = (long)NU * NU;
  const unsigned sX = (unsigned)(T + 1) * NX, sU = (unsigned)T * NU, sG = (unsigned)T * (NX + 1) * NU;
  const unsigned sA = (unsigned)T * NX * NX, sB = (unsigned)T * NX * NU, sD = (unsigned)T * NX;
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    ExplicitProv<NX, NU> prov;
    prov.A_ls = gview(a.A_ls, r.q0 * sA, r.gl * sA);
    prov.B_ls = gview(a.B_ls, r.q0 * sB, r.gl * sB);
    prov.has_delta = a.D_ls != nullptr;
    prov.D_ls = gview(a.D_ls ? a.D_ls : a.A_ls, r.q0 * sD, r.gl * sD);
    prov.j = j;
    Window win;
    win.xbm = gview(a.X_bm, r.q0 * a.xbm_stride, r.gl * (unsigned)a.xbm_stride);
    win.ubm = gview(a.U_bm, r.q0 * a.ubm_stride, r.gl * (unsigned)a.ubm_stride);
    const GView gains = gview(a.gains, r.q0 * sG, r.gl * sG);
    const GView Xo = gview(a.X_opt, r.q0 * sX, r.gl * sX);
    const GView Uo = gview(a.U_opt, r.q0 * sU, r.gl * sU);
    const bool st = r.valid && L.lane_ok;
    riccati_backward<cplx, NX, NU>(prov, T, win, cost, a.flags, gains, j, st);
    wave_sync();
    double lo0[NU], hi0[NU], u_first[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const bool band = (a.flags & QP_DU_BAND) != 0 && a.u_prev != nullptr;
      const double up = band ? gld(a.u_prev, r.b * NU + k) : 0.0;
      lo0[k] = band ? up - a.du : -a.sat;
      hi0[k] = band ? up + a.du : a.sat;
    }
    const cplx x0 = gld(a.x_init, r.b * NX + j);
    const bool exact = (a.flags & QP_EXACT_BOX) != 0;
    // the exact solver ping-pongs between two trajectory pairs of ONE allocation (rows pick theirs by lane offset):
    // X_alt = [B][T+1][n] twice, U_alt likewise; the clipped rollout, its starting point, goes straight into the first
    const GView Xa = gview(exact ? a.X_alt : a.X_opt, r.q0 * sX, r.gl * sX);
    const GView Ua = gview(exact ? a.U_alt : a.U_opt, r.q0 * sU, r.gl * sU);
    const double obj = rollout_forward<cplx, NX, NU, true>(prov, T, x0, win, cost, a.flags, gains, a.sat, lo0, hi0, Xa, Ua, j, st,
                                                              u_first);
    wave_sync();
    double obj_out = obj;
    if (exact) {
      const GView Xb = gview(a.X_alt, r.q0 * sX, r.gl * sX + (unsigned)a.B * sX);
      const GView Ub = gview(a.U_alt, r.q0 * sU, r.gl * sU + (unsigned)a.B * sU);
      const GView stat = gview(a.pin_stat, r.q0 * sU, r.gl * sU);
      PinCtx<NU> pin;
      pin.stat = stat;
      pin.box.sat = a.sat;
#pragma unroll
      for (int k = 0; k < NU; ++k) { pin.lo0[k] = lo0[k]; pin.hi0[k] = hi0[k]; }
      BoxQpRow row;
      if (r.valid) row.begin(obj);
      while (__any(row.busy())) box_qp_iterate<cplx, NX, NU>(prov, T, x0, win, cost, a.flags, gains, pin, Xa, Ua, Xb, Ub, row, j, jj, L.lane_ok);
      obj_out = row.Jk;
      const QpStats& stats = row.stats;
      GView Xs = Xa, Us = Ua;
      Xs.off = row.cur_is_a() ? Xa.off : Xb.off;
      Us.off = row.cur_is_a() ? Ua.off : Ub.off;
      if (st) {
        for (int t = 0; t <= T; ++t) Xo.st<cplx>(t * NX + j, Xs.ld<cplx>(t * NX + j));
        if (j == 0)
          for (int i = 0; i < T * NU; ++i) Uo.st<double>(i, Us.ld<double>(i));
      }
      if (r.valid && jj == 0 && a.sweep_counts) gst(a.sweep_counts, r.b, stats.sweeps);
      wave_sync();
    }
    if (r.valid && jj == 0) gst(a.cost, r.b, obj_out);
  }
}

// ---------------------------------------------------------------------------------------------
// Observed plants (m4q_observe.h): the kernels live in the objects whose dim_x is the OBSERVED dimension - the qubit block in
// the dim_x = 4 objects (plant on n_p = 9), the partial traces in the dim_x = 8 object (plant on n_p = 16) - with the shape's
// controls.  Rows, quads and strides as the other auxiliary kernels; the lanes are laid out on n_p.
// ---------------------------------------------------------------------------------------------
constexpr int OBS_KIND = NX == 4 ? OBSERVE_QUBIT_BLOCK : NX == 8 ? OBSERVE_PARTIAL_TRACE : 0;

template <int OBS>
__global__ __launch_bounds__(64) void observe_kernel(ObserveArgs a) {
  constexpr int NPL = ObserveDims<OBS>::NP, NO = ObserveDims<OBS>::N;
  static_assert(NO == NX, "the observed state is the loop state of this shape");
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const PlantLaneGeo<NPL> L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* blk = lds + g * NPL;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const cplx z = gld(a.z, r.b * a.z_stride + j);
    const cplx x = observe_row<OBS>(z, blk, jj);
    if (r.valid && jj < NO) gst(a.x, r.b * a.x_stride + jj, x);
  }
}

// the plant step is plant_kernel's device function, unchanged, on the plant's own dimensions: the arithmetic of
// m4q_plant_step_batch at (n_p, m)
template <int OBS>
__global__ __launch_bounds__(64) void observed_plant_kernel(ObsPlantArgs a) {
  constexpr int NPL = ObserveDims<OBS>::NP, DP = ObserveDims<OBS>::DP, NO = ObserveDims<OBS>::N;
  static_assert(NO == NX, "the observed state is the loop state of this shape");
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const PlantLaneGeo<NPL> L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * observe_row_elems<OBS>();
  const int nquads = quads_of(a.B);
  const long sZ = (long)(a.n_steps + 1) * NPL, sX = (long)(a.n_steps + 1) * NO, sU = (long)a.n_steps * NU;
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    // the launch before this one completed step a.step for this member (mpc_kernel: codes, steps_done); a member that ended
    // earlier, or at this step, keeps what it has
    const bool live = r.valid && gld(a.codes, r.b) == 0 && gld(a.steps_done, r.b) == a.step + 1;
    const cplx z = gld(a.zs, r.b * sZ + (long)a.step * NPL + j);
    double u[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) u[k] = gld(a.us, r.b * sU + (long)a.step * NU + k);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const cplx zn = plant_hamiltonian<NPL, NU, DP>(z, u, op0, ops, a.dt, scratch, j, jj);
    const cplx x = observe_row<OBS>(zn, scratch, jj);
    if (live && jj < NPL) gst(a.zs, r.b * sZ + (long)(a.step + 1) * NPL + j, zn);
    if (live && jj < NO) gst(a.xs, r.b * sX + (long)(a.step + 1) * NO + jj, x);
  }
}

#endif  // M4Q_NO_AUX

#ifndef M4Q_VARIANT_GEN
// ---------------------------------------------------------------------------------------------
// One held-control plant step for B states (experiment.py:202-212)
// ---------------------------------------------------------------------------------------------
template <int PLANT>
__global__ __launch_bounds__(64) M4Q_OCC void plant_kernel(PlantArgs a) {
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * SCRATCH_ELEMS;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const cplx x = gld(a.x, r.b * NX + j);
    double u[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) u[k] = gld(a.u, r.b * NU + k);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    cplx xn;
    M4Q_PLANT_STEP(PLANT, xn, x, u, op0, ops, a.dt, scratch, j, jj);
    if (r.valid && jj < NX) gst(a.x_next, r.b * NX + j, xn);
  }
}

// ---------------------------------------------------------------------------------------------
// Open-loop rollout of B plants over N held-control intervals, one launch (QExperiment.simulate for an ensemble): the state stays
// in registers from x0 to the last step, each step is the device function plant_kernel calls, over dts[t].
template <int PLANT>
__global__ __launch_bounds__(64) M4Q_OCC void plant_rollout_kernel(RollArgs a) {
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * SCRATCH_ELEMS;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const RollOut out(a, r.b, j, r.valid && L.lane_ok, r.valid && jj == 0);
    RollCtl ctl(a, r.b);
    double dtn = gld(a.dts, 0);
    cplx x = gld(a.x0, r.b * NX + j);
    out.put(0, x);
    for (int t = 0; t < a.N; ++t) {
      double u[NU];
      ctl.take(t, u);
      const double dt = dtn;
      dtn = gld(a.dts, t + 1 < a.N ? t + 1 : t);
      // The generator's (1 + m) n operator entries per lane are read again at every step, as plant_kernel reads them at every
      // launch (L2 hits): hoisted out of the step loop - the offsets are made opaque here to prevent it - they spill (d = 3: 102
      // VGPRs against 49, d = 4: 68 against 6).  The d or (1 + m) d entries of the other two plants stay in registers.
      GView o0 = op0, ok = ops;
      if constexpr (PLANT == PLANT_GENERATOR) asm volatile("" : "+v"(o0.off), "+v"(ok.off));
      M4Q_PLANT_STEP(PLANT, x, x, u, o0, ok, dt, scratch, j, jj);
      out.put(t + 1, x);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// plant_rollout_kernel with a stored law closing the loop (m4q_plant_feedback_batch; feedback.py: plant_feedback_reference is the
// definition): the controls of step t come from the state in registers (FeedbackRow), the step is that kernel's, over dts[t].
template <int PLANT>
__global__ __launch_bounds__(64) M4Q_OCC void plant_feedback_kernel(FeedbackArgs fa) {
  const RollArgs& a = fa.roll;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * SCRATCH_ELEMS;
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const bool st0 = r.valid && jj == 0;
    const RollOut out(a, r.b, j, r.valid && L.lane_ok, st0);
    FeedbackRow<NX, NU> law(fa, r.b, j);
    FeedbackOut fo(fa, r.b, st0);
    const FeedbackNoise noise(fa, r.b);
    double dtn = gld(a.dts, 0);
    cplx x = gld(a.x0, r.b * NX + j);
    fo.state(x);
    out.put(0, x);
    for (int t = 0; t < a.N; ++t) {
      double u[NU], v[NU];
      law.take(t, x, u, v);
      fo.controls(t, u);
      const double dt = dtn;
      dtn = gld(a.dts, t + 1 < a.N ? t + 1 : t);
      GView o0 = op0, ok = ops;                      // (the generator's operators are read again at every step: plant_rollout_kernel)
      if constexpr (PLANT == PLANT_GENERATOR) asm volatile("" : "+v"(o0.off), "+v"(ok.off));
      M4Q_PLANT_STEP(PLANT, x, x, v, o0, ok, dt, scratch, j, jj);
      x = noise.add(t, x, j);
      fo.state(x);
      out.put(t + 1, x);
    }
    fo.finish(law);
  }
}

// ---------------------------------------------------------------------------------------------
// Control gradient of an open-loop plant rollout (m4q_plant_rollout_grad_batch; grad.py: plant_rollout_grad_reference is the
// definition), Hamiltonian and process plants.  The forward pass is plant_rollout_kernel's, statement for statement, with every
// state kept in the workspace a.xs [B][N + 1][n]; the backward pass reads x_t back and recomputes U and dU_k (m4q_grad.h).
template <int PLANT>
constexpr int grad_lds_elems() {
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int need = grad_scratch_elems<NX, NU, D>();
  return need > SCRATCH_ELEMS ? need : SCRATCH_ELEMS;          // (the forward step works in the same block)
}
// (d = 3: compiled for two waves per SIMD the 9 x 9 block matrix of expm_cols<9> spills 101 VGPRs, 392 B of scratch per lane)
template <int PLANT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NX == 9 ? 1 : WAVES, 8))) void plant_rollout_grad_kernel(GradArgs ga) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant has no gradient kernel");
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int NC = PLANT == PLANT_PROCESS ? D * D : 1;
  const RollArgs& a = ga.roll;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * grad_lds_elems<PLANT>();
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const bool st0 = r.valid && jj == 0;
    const RollOut out(a, r.b, j, r.valid && L.lane_ok, st0);
    RollCtl ctl(a, r.b);
    double dtn = gld(a.dts, 0);
    cplx x = gld(a.x0, r.b * NX + j);
    out.put(0, x);
    for (int t = 0; t < a.N; ++t) {
      double u[NU];
      ctl.take(t, u);
      const double dt = dtn;
      dtn = gld(a.dts, t + 1 < a.N ? t + 1 : t);
      M4Q_PLANT_STEP(PLANT, x, x, u, op0, ops, dt, scratch, j, jj);
      out.put(t + 1, x);
    }
    wave_sync();                                   // the states of this member are in the workspace
    const M4Q_GLOBAL cplx* xw = a.xs + r.b * (a.N + 1) * NX;
    cplx lam = figure_grad<NX>(csub(x, out.f), a.W, j);
    for (int t = a.N - 1; t >= 0; --t) {
      double v[NU], ge[NU];
      grad_controls(ctl, t, v);
      const cplx xt = gld(xw, (long)t * NX + j);
      lam = plant_grad_step<NX, NU, D, NC>(xt, lam, v, op0, ops, gld(a.dts, t), scratch, j, jj, ge);
      if (a.q_mode == 2) lam = cadd(lam, figure_grad<NX>(csub(xt, out.f), a.W, j));
      grad_park(ga, r.b, t, ge, st0);
    }
    grad_finish(ga, ctl, r.b, st0);
  }
}

// plant_rollout_multi_kernel: S sequences shared by the ensemble against all members in one launch, the members' objectives alone
// (m4q_plant_rollout_multi_batch; the line search of m4q_plant_robust_batch)
#include "m4q_rollout_multi.h"

// (the kernels below do not depend on the library order: they are built once per (dim_x, dim_u), in the order-1 object, which is the
// one m4q_plant_rollout_param_grad_batch asks)
#if !defined(M4Q_NO_AUX) && M4Q_ORDER == 1
// ---------------------------------------------------------------------------------------------
// Plant-parameter gradient of an open-loop plant rollout against a measured trajectory (m4q_plant_rollout_param_grad_batch;
// plant_param.py: plant_param_grad_reference is the definition), Hamiltonian and process plants, PT directions.  The forward pass is
// plant_rollout_kernel's step, statement for statement, with every state kept in the workspace a.xs [B][N + 1][n] and the figure of
// column t taken against column t of the member's data (quad_figure: the rollouts' own figure); the backward pass reads x_t back and
// recomputes U and the PT derivatives dU_e (m4q_plant_param.h), adding each direction's terms with t descending.
template <int PLANT, int PT>
constexpr int param_lds_elems() {
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int need = param_scratch_elems<NX, PT, D>();
  return need > SCRATCH_ELEMS ? need : SCRATCH_ELEMS;          // (the forward step works in the same block)
}
// the block matrix has (1 + PT) d columns: past 6 of them the kernel is compiled for one wave per SIMD, as the control gradient's
// 9 x 9 block is (two waves: expm_cols<8> of d = 2, PT = 3 spills 33 VGPRs, 136 B of scratch per lane; expm_cols<6> fits in 248)
template <int PLANT, int PT>
constexpr int param_waves() { return (1 + PT) * (PLANT == PLANT_PROCESS ? DQ : DD) > 6 ? 1 : WAVES; }
template <int PLANT, int PT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(param_waves<PLANT, PT>(), 8))) void plant_param_grad_kernel(ParamGradArgs pa) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant has no gradient kernel");
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int NC = PLANT == PLANT_PROCESS ? D * D : 1;
  const RollArgs& a = pa.roll;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * param_lds_elems<PLANT, PT>();
  const int nquads = quads_of(a.B);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const GView dirs = gview(pa.dirs, r.q0 * pa.dirs_stride, r.gl * (unsigned)pa.dirs_stride);
    const bool st = r.valid && L.lane_ok, st0 = r.valid && jj == 0;
    const M4Q_GLOBAL cplx* Wr = a.W + j * NX;
    const M4Q_GLOBAL cplx* yb = pa.data + r.b * pa.data_stride;
    M4Q_GLOBAL cplx* xw = a.xs + r.b * (a.N + 1) * NX;
    RollCtl ctl(a, r.b);
    double dtn = gld(a.dts, 0);
    cplx x = gld(a.x0, r.b * NX + j);
    double J = 0.0;
    for (int t = 0; t <= a.N; ++t) {
      if (st) gst(xw, (long)t * NX + j, x);
      const double cw = gld(pa.col_w, t);
      if (cw != 0.0) {                               // (wave-uniform: every lane stays in for the broadcasts)
        double prod = cw * quad_figure<NX>(csub(x, gld(yb, (long)t * NX + j)), Wr);
        asm volatile("" : "+v"(prod));               // rounded before the add, as plant_param.py adds it
        J = J + prod;
      }
      if (t == a.N) break;
      double u[NU];
      ctl.take(t, u);
      const double dt = dtn;
      dtn = gld(a.dts, t + 1 < a.N ? t + 1 : t);
      M4Q_PLANT_STEP(PLANT, x, x, u, op0, ops, dt, scratch, j, jj);
    }
    if (st0) gst(pa.J, r.b, J);
    wave_sync();                                   // the states of this member are in the workspace
    cplx lam = czero();
    {
      const double cw = gld(pa.col_w, a.N);
      if (cw != 0.0) lam = cscale(figure_grad<NX>(csub(x, gld(yb, (long)a.N * NX + j)), a.W, j), cw);
    }
    double acc[PT];
#pragma unroll
    for (int k = 0; k < PT; ++k) acc[k] = 0.0;
    for (int t = a.N - 1; t >= 0; --t) {
      double v[NU], ut[NU], ge[PT];
#pragma unroll
      for (int k = 0; k < NU; ++k) {
        ut[k] = gld(ctl.u, (long)t * NU + k);
        v[k] = ctl.sc[k] * ut[k];
      }
      const cplx xt = gld(xw, (long)t * NX + j);
      lam = param_grad_step<NX, NU, PT, D, NC>(xt, lam, v, ut, pa.p, op0, ops, dirs, gld(a.dts, t), scratch, j, jj, ge);
      const double cw = gld(pa.col_w, t);
      if (cw != 0.0) {
        const cplx gt = figure_grad<NX>(csub(xt, gld(yb, (long)t * NX + j)), a.W, j);
        lam = cadd(lam, cscale(gt, cw));
      }
#pragma unroll
      for (int k = 0; k < PT; ++k) acc[k] = acc[k] + ge[k];
    }
    if (st0) {
#pragma unroll
      for (int k = 0; k < PT; ++k) {
        if (k < pa.p) gst(pa.grad_theta, r.b * pa.p + k, acc[k]);
        else gst(pa.grad_scale, r.b * NU + (k - pa.p), acc[k]);
      }
    }
    wave_sync();                                   // the row's reads of its LDS block and of the workspace are done
  }
}
#endif  // !M4Q_NO_AUX && M4Q_ORDER == 1

// ---------------------------------------------------------------------------------------------
// The plant's own discrete-time Jacobians along trajectories (m4q_plant_linearize_batch; plant_linearize.py:
// plant_linearize_reference is the definition), Hamiltonian and process plants.  The work unit is a (member, point) pair: row g of
// quad `quad` works on unit 4 quad + g = b T + t, whatever member that falls in; a row past the last unit repeats it and stores
// nothing.  A is written 16 consecutive entries of its row-major [n][n] block at a time, one per lane.
template <int PLANT>
constexpr int plant_lin_lds_elems() {
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  return plant_lin_scratch_elems<NX, NU, D>();
}
// (d = 3: one wave per SIMD, as plant_rollout_grad_kernel - the same expm_cols<9> of the block matrix)
template <int PLANT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NX == 9 ? 1 : WAVES, 8))) void plant_linearize_kernel(PlantLinArgs a) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant has no linearisation kernel");
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int NC = PLANT == PLANT_PROCESS ? D * D : 1;
  constexpr int NN = NX * NX;
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * plant_lin_lds_elems<PLANT>();
  const int units = a.B * a.T;                       // (the host keeps B T inside an int)
  const int nquads = quads_of(units);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, units);                 // r.b: this row's unit
    const int b0 = (int)(r.q0 / a.T);                // the quad's first member (wave-uniform)
    const int b = (int)(r.b / a.T), t = (int)(r.b - (long)b * a.T);
    const unsigned bl = (unsigned)(b - b0);
    const GView op0 = gview(a.traj.plant.op0, b0 * a.traj.plant.op0_stride, bl * (unsigned)a.traj.plant.op0_stride);
    const GView ops = gview(a.traj.plant.ops, b0 * a.traj.plant.ops_stride, bl * (unsigned)a.traj.plant.ops_stride);
    double u[NU], sc[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      u[k] = gld(a.traj.U, b * a.traj.u_stride + (long)t * NU + k);
      sc[k] = a.traj.u_scale ? gld(a.traj.u_scale, (long)b * NU + k) : 1.0;
    }
    const cplx x = gld(a.traj.X, r.b * NX + j);
    cplx Bj[NU], dlt;
    plant_lin_point<NX, NU, D, NC>(x, u, sc, op0, ops, gld(a.traj.dts, t), scratch, j, jj, Bj, dlt);
    const bool st = r.valid && L.lane_ok;
    if (a.B_ls != nullptr && st) {
#pragma unroll
      for (int k = 0; k < NU; ++k) gst(a.B_ls, (r.b * NX + j) * NU + k, Bj[k]);
    }
    if (a.D_ls != nullptr && st) gst(a.D_ls, r.b * NX + j, dlt);
    if (a.A_ls != nullptr) {
#pragma unroll
      for (int e0 = 0; e0 < NN; e0 += 16) {
        const int e = e0 + jj;
        const int ec = e < NN ? e : NN - 1;
        const int i = ec / NX;
        const cplx val = plant_lin_entry<D, NC>(scratch, i, ec - i * NX);
        if (r.valid && e < NN) gst(a.A_ls, r.b * NN + e, val);
      }
    }
    wave_sync();                                   // the row's reads of its LDS block are done
  }
}

#ifndef M4Q_NO_AUX
// ---------------------------------------------------------------------------------------------
// The QP on the plant's own linearisation (m4q_plant_quad_program_batch; m4q_plant_qp.h): two launches on one stream.  They stay
// two kernels: the linearisation has B T independent units at the register budget of the block exponential (one wave per SIMD at
// n = 9), the sweep is serial per member at qp_kernel's budget - fused, the sweep would inherit the exponential's occupancy.
//
// plant_factor_kernel: plant_linearize_kernel's work layout and LDS; in place of A it leaves the propagator U_t - the first d^2
// entries of F, one per lane at consecutive addresses - beside B_t and Delta_t, all three in device workspaces.
template <int PLANT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NX == 9 ? 1 : WAVES, 8))) void plant_factor_kernel(PlantQpArgs a) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant has no linearisation kernel");
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int NC = PLANT == PLANT_PROCESS ? D * D : 1;
  static_assert(D * D <= 16, "one entry of U per lane of the row");
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * plant_lin_lds_elems<PLANT>();
  const int units = a.B * a.T;                       // (the host keeps B T inside an int)
  const int nquads = quads_of(units);
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, units);                 // r.b: this row's unit
    const int b0 = (int)(r.q0 / a.T);                // the quad's first member (wave-uniform)
    const int b = (int)(r.b / a.T), t = (int)(r.b - (long)b * a.T);
    const unsigned bl = (unsigned)(b - b0);
    const GView op0 = gview(a.traj.plant.op0, b0 * a.traj.plant.op0_stride, bl * (unsigned)a.traj.plant.op0_stride);
    const GView ops = gview(a.traj.plant.ops, b0 * a.traj.plant.ops_stride, bl * (unsigned)a.traj.plant.ops_stride);
    double u[NU], sc[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      u[k] = gld(a.traj.U, b * a.traj.u_stride + (long)t * NU + k);
      sc[k] = a.traj.u_scale ? gld(a.traj.u_scale, (long)b * NU + k) : 1.0;
    }
    const cplx x = gld(a.traj.X, r.b * NX + j);
    cplx Bj[NU], dlt;
    plant_lin_point<NX, NU, D, NC>(x, u, sc, op0, ops, gld(a.traj.dts, t), scratch, j, jj, Bj, dlt);
    if (r.valid && L.lane_ok) {
#pragma unroll
      for (int k = 0; k < NU; ++k) gst(a.B_ws, (r.b * NX + j) * NU + k, Bj[k]);
      gst(a.D_ws, r.b * NX + j, dlt);
    }
    const cplx ue = scratch[jj < D * D ? jj : D * D - 1];
    if (r.valid && jj < D * D) gst(a.U_ws, r.b * (D * D) + jj, ue);
    wave_sync();                                   // the row's reads of its LDS block are done
  }
}

// plant_qp_kernel: qp_kernel's body on PlantProv - A_t formed from U_t - with x_init defaulting to X[b][0].  Written beside
// qp_kernel, not shared with it, so that qp_kernel's code stays what it was.
template <int PLANT>
__global__ __launch_bounds__(64) M4Q_OCC void plant_qp_kernel(PlantQpArgs a) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant has no linearisation kernel");
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  constexpr int NC = PLANT == PLANT_PROCESS ? D * D : 1;
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  const int T = a.T;
  const int nquads = quads_of(a.B);
  CostRef<cplx> cost;
  cost.Q = (const cplx*)a.Q_ls; cost.Qf = (const cplx*)a.Q_ls + (long)T * NX * NX; cost.q_stride = (long)NX * NX;
  cost.R = (const cplx*)a.R_ls; cost.r_stride = (long)NU * NU;
  const unsigned sX = (unsigned)(T + 1) * NX, sU = (unsigned)T * NU, sG = (unsigned)T * (NX + 1) * NU;
  const unsigned sP = (unsigned)T * D * D, sB = (unsigned)T * NX * NU, sD = (unsigned)T * NX;
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    PlantProv<NX, NU, D, NC> prov;
    prov.U_ls = gview(a.U_ws, r.q0 * sP, r.gl * sP);
    prov.B_ls = gview(a.B_ws, r.q0 * sB, r.gl * sB);
    prov.D_ls = gview(a.D_ws, r.q0 * sD, r.gl * sD);
    prov.j = j;
    Window win;
    win.xbm = gview(a.X_bm, r.q0 * a.xbm_stride, r.gl * (unsigned)a.xbm_stride);
    win.ubm = gview(a.U_bm, r.q0 * a.ubm_stride, r.gl * (unsigned)a.ubm_stride);
    const GView gains = gview(a.gains, r.q0 * sG, r.gl * sG);
    const GView Xo = gview(a.X_opt, r.q0 * sX, r.gl * sX);
    const GView Uo = gview(a.U_opt, r.q0 * sU, r.gl * sU);
    const bool st = r.valid && L.lane_ok;
    riccati_backward<cplx, NX, NU>(prov, T, win, cost, a.flags, gains, j, st);
    wave_sync();
    double lo0[NU], hi0[NU], u_first[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const bool band = (a.flags & QP_DU_BAND) != 0 && a.u_prev != nullptr;
      const double up = band ? gld(a.u_prev, r.b * NU + k) : 0.0;
      lo0[k] = band ? up - a.du : -a.sat;
      hi0[k] = band ? up + a.du : a.sat;
    }
    const cplx x0 = a.x_init ? gld(a.x_init, r.b * NX + j) : gld(a.traj.X, r.b * ((long)T * NX) + j);
    const bool exact = (a.flags & QP_EXACT_BOX) != 0;
    // (the exact solver's ping-pong workspace, as qp_kernel)
    const GView Xa = gview(exact ? a.X_alt : a.X_opt, r.q0 * sX, r.gl * sX);
    const GView Ua = gview(exact ? a.U_alt : a.U_opt, r.q0 * sU, r.gl * sU);
    const double obj = rollout_forward<cplx, NX, NU, true>(prov, T, x0, win, cost, a.flags, gains, a.sat, lo0, hi0, Xa, Ua, j, st,
                                                              u_first);
    wave_sync();
    double obj_out = obj;
    if (exact) {
      const GView Xb = gview(a.X_alt, r.q0 * sX, r.gl * sX + (unsigned)a.B * sX);
      const GView Ub = gview(a.U_alt, r.q0 * sU, r.gl * sU + (unsigned)a.B * sU);
      const GView stat = gview(a.pin_stat, r.q0 * sU, r.gl * sU);
      PinCtx<NU> pin;
      pin.stat = stat;
      pin.box.sat = a.sat;
#pragma unroll
      for (int k = 0; k < NU; ++k) { pin.lo0[k] = lo0[k]; pin.hi0[k] = hi0[k]; }
      BoxQpRow row;
      if (r.valid) row.begin(obj);
      while (__any(row.busy())) box_qp_iterate<cplx, NX, NU>(prov, T, x0, win, cost, a.flags, gains, pin, Xa, Ua, Xb, Ub, row, j, jj, L.lane_ok);
      obj_out = row.Jk;
      const QpStats& stats = row.stats;
      GView Xs = Xa, Us = Ua;
      Xs.off = row.cur_is_a() ? Xa.off : Xb.off;
      Us.off = row.cur_is_a() ? Ua.off : Ub.off;
      if (st) {
        for (int t = 0; t <= T; ++t) Xo.st<cplx>(t * NX + j, Xs.ld<cplx>(t * NX + j));
        if (j == 0)
          for (int i = 0; i < T * NU; ++i) Uo.st<double>(i, Us.ld<double>(i));
      }
      if (r.valid && jj == 0 && a.sweep_counts) gst(a.sweep_counts, r.b, stats.sweeps);
      wave_sync();
    }
    if (r.valid && jj == 0) gst(a.cost, r.b, obj_out);
  }
}

// plant_step_kernel: the line search, the decision and the hand-over between two of these QPs, over points of the line to the QP's
// optimum (m4q_plant_sqp_batch) or in closed loop - the QP's gains run on the plant (m4q_plant_ilqr_batch)
#include "m4q_plant_step.h"
#endif  // M4Q_NO_AUX

// ---------------------------------------------------------------------------------------------
// The measurement noise of B members at one column of xs (noise.py: MeasurementNoise.sample), one component per lane, by the
// device function the closed loop calls: a run's noise realisation without the run.
__global__ __launch_bounds__(64) void noise_sample_kernel(NoiseArgs a) {
  const long total = (long)a.B * NX;
  for (long e = blockIdx.x * 64L + threadIdx.x; e < total; e += gridDim.x * 64L) {
    const long b = e / NX;
    const int comp = (int)(e - b * NX);
    const double sg = gld(a.sigma, b * a.sigma_stride);
    gst(a.out, e, noise_sample(a.mode, a.seed, a.member_base + (unsigned long long)b, a.state_index, comp, SQUARE ? DD : 0, sg));
  }
}

#endif  // M4Q_VARIANT_GEN

#if !defined(M4Q_NO_AUX) && M4Q_ORDER <= 2
// ---------------------------------------------------------------------------------------------
// discretize_homogeneous for B generator sets (vectorize.py:8-49): Taylor/Dyson expansion of
// exp(dt (G_0 + sum_k u_k G_k)) to ORDER, every word of operators multiplied out and binned by its control
// monomial.  One row per instance; generators staged in LDS, products column-owned in registers.
// (orders 3 and 4 have closed-loop kernels but no device discretisation: their models come from the host, discretize_homogeneous)
// ---------------------------------------------------------------------------------------------
constexpr int find_monomial(int c0, int c1, int c2) {
  constexpr PowTab<NU, ORDER> tab{};
  const int want[3] = {c0, c1, c2};
  for (int p = 0; p < PowTab<NU, ORDER>::COUNT; ++p) {
    bool same = true;
    for (int k = 0; k < NU; ++k) same = same && tab.e[p][k] == want[k];
    if (same) return p;
  }
  return -1;
}
constexpr int word_block(int a, int b) {      // monomial of a word of one (b < 0) or two letters; letter 0 = drift
  int c[3] = {0, 0, 0};
  if (a > 0) ++c[a - 1];
  if (b > 0) ++c[b - 1];
  return find_monomial(c[0], c[1], c[2]);
}

// N: matrix dimension (NX, or NX - 1 for the traceless blocks of the lifted generators)
template <class S, int N>
__global__ __launch_bounds__(64) void discretize_kernel(DiscArgs a) {
  static_assert(ORDER == 1 || ORDER == 2, "orders 1 and 2 are compiled");
  S* lds = reinterpret_cast<S*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj;
  const int j = jj < N ? jj : N - 1;
  constexpr int NX = N;                           // (shadows the shape's NX inside this kernel)
  constexpr int GEN_ELEMS = (1 + NU) * NX * NX;
  constexpr int W = NX * (1 + NP);
  S* G = lds + g * GEN_ELEMS;                      // [1+m][n][n] row-major, scaled
  const int nquads = quads_of(a.B);
  const M4Q_GLOBAL S* gens = (const M4Q_GLOBAL S*)a.gens;
  M4Q_GLOBAL S* models = (M4Q_GLOBAL S*)a.models;
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    // (QuadRow's member, written as one select: as q0 + gl it costs seven of these kernels one or two VGPRs)
    const long q0 = (long)quad * ROWS;
    const bool valid = q0 + g < a.B;
    const long b = valid ? q0 + g : a.B - 1;
    wave_sync();
    for (int e = jj; e < GEN_ELEMS; e += 16) {
      const double sc = a.scales ? gld(a.scales, b * (1 + NU) + e / (NX * NX)) : 1.0;
      G[e] = cscale(gld(gens, b * a.gen_stride + e), sc);
    }
    wave_sync();
    M4Q_GLOBAL S* out = models + b * (long)NX * W;
    // accumulate every block's column j in registers: blk[p][i]
    S blk[1 + NP][NX];
#pragma unroll
    for (int p = 0; p <= NP; ++p)
#pragma unroll
      for (int i = 0; i < NX; ++i) blk[p][i] = zero_of<S>();
#pragma unroll
    for (int i = 0; i < NX; ++i) blk[0][i] = from_real<S>(i == j ? 1.0 : 0.0);       // k = 0: identity
    static_for<0, 1 + NU>([&](auto aa) {
      constexpr int la = decltype(aa)::value;
      S Ga[NX];                                       // column j of G_a
#pragma unroll
      for (int i = 0; i < NX; ++i) Ga[i] = G[(la * NX + i) * NX + j];
      constexpr int p1 = word_block(la, -1);
#pragma unroll
      for (int i = 0; i < NX; ++i) cmac_r(blk[p1][i], Ga[i], a.dt);                    // k = 1: dt G_a
      if constexpr (ORDER >= 2) {
        static_for<0, 1 + NU>([&](auto bb) {
          constexpr int lb = decltype(bb)::value;
          S Gb[NX], prod[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) Gb[i] = G[(lb * NX + i) * NX + j];
          matmul_cols<NX>(prod, Ga, Gb);             // column j of G_a G_b (word "a then b": entry @ A_a @ A_b)
          constexpr int p2 = word_block(la, lb);
#pragma unroll
          for (int i = 0; i < NX; ++i) cmac_r(blk[p2][i], prod[i], 0.5 * a.dt * a.dt);
        });
      }
    });
    if (valid && jj < N) {
#pragma unroll
      for (int p = 0; p <= NP; ++p)
#pragma unroll
        for (int i = 0; i < NX; ++i) gst(out, i * W + p * NX + j, blk[p][i]);
    }
  }
}
#endif  // !M4Q_NO_AUX && M4Q_ORDER <= 2

// ---------------------------------------------------------------------------------------------
// host-side launchers for this shape
// ---------------------------------------------------------------------------------------------
template <class K>
static int prep_lds(K kern, size_t bytes) {
  if (bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return -(int)e;
  }
  return 0;
}

// what to do with the kernel instance picked by (arithmetic path, plant kind, QP mode)
struct LaunchOp {
  const MpcArgs& a;
  int grid;
  hipStream_t s;
  int unsupported() const { return -(int)hipErrorInvalidValue; }
  template <class S, int PLANT, bool EXACT, bool TL, bool TILE, bool SG = false>
  int run() const {
    const size_t lds = mpc_lds_layout_bytes<S, TL, TILE, EXACT, SG>();
    // (the tile kernels run two wavefronts per SIMD, eight workgroups per CU: an eighth of the CU's 160 KB each - with more, the launch
    //  runs on fewer wavefronts than the grid has)
    static_assert(!TILE || mpc_lds_layout_bytes<S, TL, TILE, EXACT, SG>() <= 20480, "tile kernel: eight workgroups per CU");
    int rc = prep_lds(mpc_kernel<S, PLANT, EXACT, TL, TILE, SG>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((mpc_kernel<S, PLANT, EXACT, TL, TILE, SG>), dim3(grid), dim3(64), lds, s, a);
    return -(int)hipGetLastError();
  }
};
struct OccupancyOp {
  int unsupported() const { return 0; }
  template <class S, int PLANT, bool EXACT, bool TL, bool TILE, bool SG = false>
  int run() const {
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, mpc_kernel<S, PLANT, EXACT, TL, TILE, SG>, 64,
                                                                 mpc_lds_layout_bytes<S, TL, TILE, EXACT, SG>());
    return e != hipSuccess ? -(int)e : nb;
  }
};
struct LdsOp {
  int unsupported() const { return 0; }
  template <class S, int PLANT, bool EXACT, bool TL, bool TILE, bool SG = false>
  int run() const { return (int)mpc_lds_layout_bytes<S, TL, TILE, EXACT, SG>(); }
};

template <class S, bool EXACT, bool TL, bool TILE, class Op, bool SG = false>
static int pick_plant(const Op& op, int plant_kind) {
  if constexpr (!SQUARE) {
#ifdef M4Q_VARIANT_GEN
    return op.unsupported();
#else
    return op.template run<S, PLANT_NONE, EXACT, false, false>();
#endif
  } else {
#ifdef M4Q_VARIANT_GEN
    if (plant_kind == PLANT_GENERATOR) return op.template run<S, PLANT_GENERATOR, EXACT, TL, TILE, SG>();
    return op.unsupported();
#else
    if (plant_kind == PLANT_HAMILTONIAN) return op.template run<S, PLANT_HAMILTONIAN, EXACT, TL, TILE, SG>();
    if (plant_kind == PLANT_GENERATOR) return op.unsupported();          // (libm4q_hip_gen.so: the host routes such sessions there)
    if (plant_kind == PLANT_PROCESS) {
      // the complex path alone (the host forces it for a process plant: m4q_session_create)
      if constexpr (QUARTIC && std::is_same<S, cplx>::value && !TL && !TILE && !SG) return op.template run<S, PLANT_PROCESS, EXACT, false, false>();
      else return op.unsupported();
    }
    return op.template run<S, PLANT_NONE, EXACT, TL, TILE, SG>();
#endif
  }
}

// PATH_TILE: the clipped solve has its own kernel; the exact solve runs its pinned sweep on tiles inside the one exact traceless
// kernel, chosen by QP_TARG_CONST and QP_NO_TILE in the flags
template <class Op>
static int pick_kernel(const Op& op, int plant_kind, Path path, int exact, int unsupported) {
  if constexpr (!SQUARE) {
    if (path != PATH_COMPLEX || plant_kind != PLANT_NONE) return unsupported;
  }
  if constexpr (HAS_SG) {
    // the clipped traceless kernel on shared generators (sessions built by m4q_session_build_models; the host falls back to
    // PATH_TRACELESS - per-member models - for the exact mode)
    if (path == PATH_SG && !exact) return pick_plant<double, false, true, false, Op, true>(op, plant_kind);
  }
  if (path == PATH_SG) path = PATH_TRACELESS;
  if constexpr (SQUARE) {
    if constexpr (HAS_TILE) { if (path == PATH_TILE && !exact) return pick_plant<double, false, true, true>(op, plant_kind); }
    if (coords_of(path) == COORDS_TRACELESS) return exact ? pick_plant<double, true, true, false>(op, plant_kind) : pick_plant<double, false, true, false>(op, plant_kind);
    if (path == PATH_REAL) return exact ? pick_plant<double, true, false, false>(op, plant_kind) : pick_plant<double, false, false, false>(op, plant_kind);
  }
  return exact ? pick_plant<cplx, true, false, false>(op, plant_kind) : pick_plant<cplx, false, false, false>(op, plant_kind);
}

#ifndef M4Q_PLANT_ONLY
static int launch_mpc(const MpcArgs& a, int plant_kind, Path path, int grid, hipStream_t s) {
  return pick_kernel(LaunchOp{a, grid, s}, plant_kind, path, (a.flags & QP_EXACT_BOX) != 0, -(int)hipErrorInvalidValue);
}

static int occupancy(int plant_kind, Path path, int exact) {
  return pick_kernel(OccupancyOp{}, plant_kind, path, exact, 0);
}

static int mpc_lds_bytes(int plant_kind, Path path, int exact) {
  return pick_kernel(LdsOp{}, plant_kind, path, exact, 0);
}

#else
static int launch_mpc(const MpcArgs&, int, Path, int, hipStream_t) { return -(int)hipErrorInvalidValue; }
static int occupancy(int, Path, int) { return 0; }
static int mpc_lds_bytes(int, Path, int) { return 0; }
#endif

static int grid_for(int B) {
  const int nquads = (B + ROWS - 1) / ROWS;
  return nquads < 4096 ? (nquads > 0 ? nquads : 1) : 4096;
}

// The three ways an auxiliary kernel is launched, each with `lds` bytes of dynamic LDS and workgroups of one wavefront:
// launch_rows: over quads of `count` rows of work - members, or (member, point) pairs - grid_for(count) workgroups
template <class K, class A>
static int launch_rows(K kern, const A& a, int count, size_t lds, hipStream_t s) {
  int rc = prep_lds(kern, lds);
  if (rc) return rc;
  hipLaunchKernelGGL(kern, dim3(grid_for(count)), dim3(64), lds, s, a);
  return -(int)hipGetLastError();
}
// launch_aux: ... whose rows are the a.B members of the block
template <class K, class A>
static int launch_aux(K kern, const A& a, size_t lds, hipStream_t s) { return launch_rows(kern, a, a.B, lds, s); }
// launch_members: one workgroup per member, 4096 at the most (the fits and the recursive update)
template <class K, class A>
[[maybe_unused]] static int launch_members(K kern, const A& a, int B, size_t lds, hipStream_t s) {
  int rc = prep_lds(kern, lds);
  if (rc) return rc;
  hipLaunchKernelGGL(kern, dim3(B < 4096 ? B : 4096), dim3(64), lds, s, a);
  return -(int)hipGetLastError();
}
[[maybe_unused]] constexpr int UNBUILT = -(int)hipErrorInvalidValue;      // what the launcher of a kernel this object does not hold returns

#ifndef M4Q_NO_AUX
constexpr size_t MODEL_LDS = sizeof(cplx) * (size_t)(ROWS * MODEL_ELEMS);
static int launch_linearize(const LinArgs& a, hipStream_t s) { return launch_aux(linearize_kernel, a, MODEL_LDS, s); }
static int launch_qp(const QpArgs& a, hipStream_t s) { return launch_aux(qp_kernel, a, 0, s); }
static int launch_model_rollout(const RollArgs& a, hipStream_t s) { return launch_aux(model_rollout_kernel, a, MODEL_LDS, s); }
static int launch_model_feedback(const FeedbackArgs& a, hipStream_t s) { return launch_rows(model_feedback_kernel, a, a.roll.B, MODEL_LDS, s); }
// (a partial specialisation, so that the kernel is instantiated only for the shapes whose layout fits)
template <bool FITS, int N_ = NX>
struct FitLaunch {
  static int run(const FitArgs&, hipStream_t) { return UNBUILT; }
  static int run_qr(const FitArgs&, hipStream_t) { return UNBUILT; }
  static int run_refit(const RefitArgs&, hipStream_t) { return UNBUILT; }
  static int run_refit_qr(const RefitArgs&, hipStream_t) { return UNBUILT; }
};
template <int N_>
struct FitLaunch<true, N_> {
  static constexpr size_t LDS = FitLayout<N_, NU, ORDER>::BYTES;
  static int run(const FitArgs& a, hipStream_t s) { return launch_members(dmdc_fit_kernel<N_, NU, ORDER>, a, a.B, LDS, s); }
  static int run_qr(const FitArgs& a, hipStream_t s) { return launch_members(dmdc_fit_qr_kernel<N_, NU, ORDER>, a, a.B, LDS, s); }
  static int run_refit(const RefitArgs& a, hipStream_t s) { return launch_members(dmdc_refit_kernel<N_, NU, ORDER>, a, a.fit.B, LDS, s); }
  static int run_refit_qr(const RefitArgs& a, hipStream_t s) { return launch_members(dmdc_refit_qr_kernel<N_, NU, ORDER>, a, a.fit.B, LDS, s); }
};
constexpr bool FIT_FITS = FitLayout<NX, NU, ORDER>::FITS;
constexpr int FIT_LDS = FIT_FITS ? (int)FitLayout<NX, NU, ORDER>::BYTES : 0;
static int launch_fit(const FitArgs& a, hipStream_t s) { return FitLaunch<FIT_FITS>::run(a, s); }
static int launch_fit_qr(const FitArgs& a, hipStream_t s) { return FitLaunch<FIT_FITS>::run_qr(a, s); }
static int launch_refit(const RefitArgs& a, hipStream_t s) { return FitLaunch<FIT_FITS>::run_refit(a, s); }
static int launch_refit_qr(const RefitArgs& a, hipStream_t s) { return FitLaunch<FIT_FITS>::run_refit_qr(a, s); }
template <bool FITS, int N_ = NX>
struct OnlineLaunch {
  static int run(const OnlineArgs&, int, hipStream_t) { return UNBUILT; }
};
template <int N_>
struct OnlineLaunch<true, N_> {
  template <bool HERM>
  static int go(const OnlineArgs& a, hipStream_t s) {
    return launch_members(online_dmdc_kernel<N_, NU, ORDER, HERM>, a, a.B, OnlineLayout<N_, NU, ORDER>::BYTES, s);
  }
  static int run(const OnlineArgs& a, int hermitian, hipStream_t s) { return hermitian ? go<true>(a, s) : go<false>(a, s); }
};
constexpr bool ONLINE_FITS = OnlineLayout<NX, NU, ORDER>::FITS;
constexpr int ONLINE_LDS = ONLINE_FITS ? (int)OnlineLayout<NX, NU, ORDER>::BYTES : 0;
static int launch_online(const OnlineArgs& a, int hermitian, hipStream_t s) { return OnlineLaunch<ONLINE_FITS>::run(a, hermitian, s); }
// (a partial specialisation, so that the kernels are instantiated only in the objects they belong to)
template <int OBS>
struct ObserveLaunch {
  static int lift(const ObserveArgs& a, hipStream_t s) {
    if (a.kind != OBS) return UNBUILT;
    return launch_aux(observe_kernel<OBS>, a, sizeof(cplx) * (size_t)(ROWS * ObserveDims<OBS>::NP), s);
  }
  static int step(const ObsPlantArgs& a, hipStream_t s) {
    if (a.kind != OBS) return UNBUILT;
    return launch_aux(observed_plant_kernel<OBS>, a, sizeof(cplx) * (size_t)(ROWS * observe_row_elems<OBS>()), s);
  }
};
template <>
struct ObserveLaunch<0> {
  static int lift(const ObserveArgs&, hipStream_t) { return UNBUILT; }
  static int step(const ObsPlantArgs&, hipStream_t) { return UNBUILT; }
};
static int launch_observe(const ObserveArgs& a, hipStream_t s) { return ObserveLaunch<OBS_KIND>::lift(a, s); }
static int launch_observed_plant(const ObsPlantArgs& a, hipStream_t s) { return ObserveLaunch<OBS_KIND>::step(a, s); }
#else
constexpr int OBS_KIND = 0;
static int launch_observe(const ObserveArgs&, hipStream_t) { return UNBUILT; }
static int launch_observed_plant(const ObsPlantArgs&, hipStream_t) { return UNBUILT; }
constexpr int FIT_LDS = 0;
static int launch_fit(const FitArgs&, hipStream_t) { return UNBUILT; }
static int launch_fit_qr(const FitArgs&, hipStream_t) { return UNBUILT; }
static int launch_refit(const RefitArgs&, hipStream_t) { return UNBUILT; }
static int launch_refit_qr(const RefitArgs&, hipStream_t) { return UNBUILT; }
constexpr int ONLINE_LDS = 0;
static int launch_online(const OnlineArgs&, int, hipStream_t) { return UNBUILT; }
static int launch_linearize(const LinArgs&, hipStream_t) { return UNBUILT; }
static int launch_qp(const QpArgs&, hipStream_t) { return UNBUILT; }
static int launch_model_rollout(const RollArgs&, hipStream_t) { return UNBUILT; }
static int launch_model_feedback(const FeedbackArgs&, hipStream_t) { return UNBUILT; }
#endif

#ifndef M4Q_VARIANT_GEN
// The kernel of plant `kind` among those of one family, over quads of `count` rows: kernel_of(ic<PLANT>) names the family's kernel,
// lds_elems(ic<PLANT>) the complex LDS elements it asks for per row.  GEN: the family has a kernel for the generator plant, which
// then serves every kind that is neither of the other two; without one such a kind is UNBUILT, as the process plant is where n is
// no fourth power and every plant where n is no square.  Only the kernels of the branches taken are instantiated.
template <bool GEN, class A, class F, class L>
static int launch_by_plant(const A& a, int kind, int count, hipStream_t s, F kernel_of, L lds_elems) {
  if constexpr (!SQUARE) {
    return UNBUILT;
  } else {
    const auto go = [&](auto plant) { return launch_rows(kernel_of(plant), a, count, sizeof(cplx) * (size_t)(ROWS * lds_elems(plant)), s); };
    if (kind == PLANT_HAMILTONIAN) return go(ic<PLANT_HAMILTONIAN>{});
    if (kind == PLANT_PROCESS) {
      if constexpr (QUARTIC) return go(ic<PLANT_PROCESS>{});
      else return UNBUILT;
    }
    if constexpr (GEN) return go(ic<PLANT_GENERATOR>{});
    else return UNBUILT;
  }
}
// (LDS per row: the plant step's scratch; what the block exponential of the linearisation asks for; none)
constexpr auto step_lds = [](auto) { return SCRATCH_ELEMS; };
constexpr auto lin_lds = [](auto plant) { return plant_lin_lds_elems<decltype(plant)::value>(); };
[[maybe_unused]] constexpr auto no_lds = [](auto) { return 0; };
static int launch_plant(const PlantArgs& a, hipStream_t s) {
  return launch_by_plant<true>(a, a.kind, a.B, s, [](auto plant) { return plant_kernel<decltype(plant)::value>; }, step_lds);
}
static int launch_plant_rollout(const RollArgs& a, hipStream_t s) {
  return launch_by_plant<true>(a, a.kind, a.B, s, [](auto plant) { return plant_rollout_kernel<decltype(plant)::value>; }, step_lds);
}
static int launch_plant_feedback(const FeedbackArgs& a, hipStream_t s) {
  return launch_by_plant<true>(a, a.roll.kind, a.roll.B, s, [](auto plant) { return plant_feedback_kernel<decltype(plant)::value>; }, step_lds);
}

static int launch_noise(const NoiseArgs& a, hipStream_t s) {
  const long blocks = ((long)a.B * NX + 63) / 64;
  hipLaunchKernelGGL(noise_sample_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(64), 0, s, a);
  return -(int)hipGetLastError();
}

// the two passes of the ordered reduction behind a gradient kernel, on its stream: members in chunks of GRAD_CHUNK into
// a.partial [chunks][N m + 1], then the chunk partials, as one chunk and without weights, into a.grad_mean and a.q_mean
static int launch_grad_reduce(const GradArgs& a, hipStream_t s) {
  if (!a.reduce) return 0;
  const RollArgs& r = a.roll;
  const int nm = r.N * NU;
  const int nchunks = (r.B + GRAD_CHUNK - 1) / GRAD_CHUNK;
  GradReduceArgs p{};
  p.count = r.B; p.chunk = GRAD_CHUNK; p.nm = nm; p.q_cols = r.q_mode == 2 ? r.N + 1 : 1;
  p.vals = a.grad; p.row_stride = nm; p.q = r.q; p.w = a.weights;
  p.out = a.partial; p.out_stride = nm + 1; p.out_last = a.partial + nm; p.last_stride = nm + 1;
  GradReduceArgs f{};
  f.count = nchunks; f.chunk = nchunks; f.nm = nm; f.q_cols = 0;
  f.vals = a.partial; f.row_stride = nm + 1;
  f.out = a.grad_mean; f.out_last = a.q_mean;
  const long threads = (long)nchunks * (nm + 1);
  const long blocks = (threads + 255) / 256;
  hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, p);
  if (hipError_t e = hipGetLastError()) return -(int)e;
  hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((nm + 1 + 255) / 256)), dim3(256), 0, s, f);
  return -(int)hipGetLastError();
}
// a gradient kernel over quads of members, then the reduction when the call asks for one
static int launch_plant_grad(const GradArgs& a, hipStream_t s) {
  const int rc = launch_by_plant<false>(a, a.roll.kind, a.roll.B, s, [](auto plant) { return plant_rollout_grad_kernel<decltype(plant)::value>; },
                                        [](auto plant) { return grad_lds_elems<decltype(plant)::value>(); });
  return rc ? rc : launch_grad_reduce(a, s);
}
// a linearisation kernel over quads of (member, point) pairs
static int launch_plant_linearize(const PlantLinArgs& a, hipStream_t s) {
  return launch_by_plant<false>(a, a.kind, a.B * a.T, s, [](auto plant) { return plant_linearize_kernel<decltype(plant)::value>; }, lin_lds);
}
#ifndef M4Q_NO_AUX
static int launch_model_grad(const GradArgs& a, hipStream_t s) {
  const int rc = launch_rows(model_rollout_grad_kernel, a, a.roll.B, MODEL_LDS, s);
  return rc ? rc : launch_grad_reduce(a, s);
}
#else
static int launch_model_grad(const GradArgs&, hipStream_t) { return UNBUILT; }
#endif
#if !defined(M4Q_NO_AUX) && M4Q_ORDER == 1
// the parameter-gradient kernel of plant PLANT compiled for p_tot directions, over quads of members: PT counts up from 1 to the
// last count whose block matrix fits a row, (1 + PT) d <= 16; any other p_tot is UNBUILT
template <int PLANT, int PT>
static int launch_param_pt(const ParamGradArgs& a, int p_tot, hipStream_t s) {
  constexpr int D = PLANT == PLANT_PROCESS ? DQ : DD;
  if constexpr ((1 + PT) * D > 16) {
    return UNBUILT;
  } else {
    if (p_tot == PT)
      return launch_rows(plant_param_grad_kernel<PLANT, PT>, a, a.roll.B, sizeof(cplx) * (size_t)(ROWS * param_lds_elems<PLANT, PT>()), s);
    return launch_param_pt<PLANT, PT + 1>(a, p_tot, s);
  }
}
// (a template, as launch_by_plant: only the kernels of the branches taken are instantiated)
template <class A>
static int launch_param_by_plant(const A& a, int p_tot, hipStream_t s) {
  if constexpr (!SQUARE) {
    return UNBUILT;
  } else {
    const auto go = [&](auto plant) { return launch_param_pt<decltype(plant)::value, 1>(a, p_tot, s); };
    if (a.roll.kind == PLANT_HAMILTONIAN) return go(ic<PLANT_HAMILTONIAN>{});
    if (a.roll.kind == PLANT_PROCESS) {
      if constexpr (QUARTIC) return go(ic<PLANT_PROCESS>{});
      else return UNBUILT;
    }
    return UNBUILT;
  }
}
static int launch_plant_param_grad(const ParamGradArgs& a, int p_tot, hipStream_t s) { return launch_param_by_plant(a, p_tot, s); }
#else
static int launch_plant_param_grad(const ParamGradArgs&, int, hipStream_t) { return UNBUILT; }
#endif
// the S shared sequences of MultiArgs against every member (m4q_rollout_multi.h): over quads of members with the rollouts' LDS,
// then - a.F set - the two passes of the ordered reduction over J [B][S] on the same stream.  grad_reduce's element
// nm is row i's vals[i][nm] when q_cols is 0, so nm = S - 1 over rows of S covers the S columns.
// (A: MultiArgs or ModelMultiArgs - the reduction reads what the two blocks name alike)
template <class A>
static int launch_multi_reduce(const A& a, hipStream_t s) {
  if (!a.F) return 0;
  const int nchunks = (a.B + GRAD_CHUNK - 1) / GRAD_CHUNK;
  GradReduceArgs p{};
  p.count = a.B; p.chunk = GRAD_CHUNK; p.nm = a.S - 1; p.q_cols = 0;
  p.vals = a.J; p.row_stride = a.S; p.w = a.weights;
  p.out = a.partial; p.out_stride = a.S; p.out_last = a.partial + (a.S - 1); p.last_stride = a.S;
  GradReduceArgs f{};
  f.count = nchunks; f.chunk = nchunks; f.nm = a.S - 1; f.q_cols = 0;
  f.vals = a.partial; f.row_stride = a.S;
  f.out = a.F; f.out_last = a.F + (a.S - 1);
  const long blocks = ((long)nchunks * a.S + 255) / 256;
  hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, p);
  if (hipError_t e = hipGetLastError()) return -(int)e;
  hipLaunchKernelGGL(grad_reduce_kernel, dim3(1), dim3(256), 0, s, f);
  return -(int)hipGetLastError();
}
static int launch_plant_multi(const MultiArgs& a, hipStream_t s) {
  const int rc = launch_by_plant<false>(a, a.kind, a.B, s, [](auto plant) { return plant_rollout_multi_kernel<decltype(plant)::value>; }, step_lds);
  return rc ? rc : launch_multi_reduce(a, s);
}
// ... through the members' models (m4q_model_multi.h): over quads of members with the model rollouts' LDS, then the same reduction
#ifndef M4Q_NO_AUX
static int launch_model_multi(const ModelMultiArgs& a, hipStream_t s) {
  const int rc = launch_aux(model_rollout_multi_kernel, a, MODEL_LDS, s);
  return rc ? rc : launch_multi_reduce(a, s);
}
#else
static int launch_model_multi(const ModelMultiArgs&, hipStream_t) { return UNBUILT; }
#endif
#else
static int launch_plant_multi(const MultiArgs&, hipStream_t) { return UNBUILT; }
static int launch_model_multi(const ModelMultiArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant(const PlantArgs&, hipStream_t) { return UNBUILT; }
static int launch_noise(const NoiseArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant_rollout(const RollArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant_feedback(const FeedbackArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant_grad(const GradArgs&, hipStream_t) { return UNBUILT; }
static int launch_model_grad(const GradArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant_linearize(const PlantLinArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant_param_grad(const ParamGradArgs&, int, hipStream_t) { return UNBUILT; }
#endif

#ifndef M4Q_NO_AUX
// the two kernels of the QP on the plant's own linearisation, on one stream: the factors of every (member, point) pair, then the
// sweep over quads of members
static int launch_plant_qp(const PlantQpArgs& a, hipStream_t s) {
  const int rc = launch_by_plant<false>(a, a.kind, a.B * a.T, s, [](auto plant) { return plant_factor_kernel<decltype(plant)::value>; }, lin_lds);
  return rc ? rc : launch_by_plant<false>(a, a.kind, a.B, s, [](auto plant) { return plant_qp_kernel<decltype(plant)::value>; }, no_lds);
}
// the step between two of them (m4q_plant_step.h): over quads of members, the rollouts' LDS
template <bool CLOSED>
static int launch_plant_step_of(const PlantStepArgs& a, hipStream_t s) {
  return launch_by_plant<false>(a, a.kind, a.B, s, [](auto plant) { return plant_step_kernel<decltype(plant)::value, CLOSED>; }, step_lds);
}
static int launch_plant_step(const PlantStepArgs& a, hipStream_t s) {
  return a.closed ? launch_plant_step_of<true>(a, s) : launch_plant_step_of<false>(a, s);
}
#else
static int launch_plant_qp(const PlantQpArgs&, hipStream_t) { return UNBUILT; }
static int launch_plant_step(const PlantStepArgs&, hipStream_t) { return UNBUILT; }
#endif

#if !defined(M4Q_NO_AUX) && M4Q_ORDER <= 2
// coords: complex generators; real n x n (lifted to the Hermitian basis); real (n-1) x (n-1) (their traceless blocks)
static int launch_discretize(const DiscArgs& a, Coords coords, hipStream_t s) {
  if (!SQUARE && coords != COORDS_COMPLEX) return UNBUILT;
  constexpr size_t elems = (size_t)ROWS * (1 + NU) * NX * NX;
  if constexpr (SQUARE) {
    if (coords == COORDS_TRACELESS) return launch_aux(discretize_kernel<double, NX - 1>, a, elems * sizeof(double), s);
  }
  if (coords == COORDS_HERM) return launch_aux(discretize_kernel<double, NX>, a, elems * sizeof(double), s);
  return launch_aux(discretize_kernel<cplx, NX>, a, elems * sizeof(cplx), s);
}
#else
static int launch_discretize(const DiscArgs&, Coords, hipStream_t) { return UNBUILT; }
#endif

static int power_list(int32_t* out) {
  constexpr PowTab<NU, ORDER> tab{};
  for (int p = 0; p < PowTab<NU, ORDER>::COUNT; ++p)
    for (int k = 0; k < NU; ++k) out[p * NU + k] = tab.e[p][k];
  return PowTab<NU, ORDER>::COUNT;
}

static const ShapeOps* shape_ops() {
#ifdef M4Q_PLANT_ONLY
  constexpr int plant_only = 1;
#else
  constexpr int plant_only = 0;
#endif
  static const ShapeOps ops = {NX, NU, ORDER, NP, DD, HAS_TILE ? 1 : 0, HAS_SG ? 1 : 0, plant_only, mpc_lds_bytes, launch_mpc, launch_linearize, launch_qp, launch_plant,
                               launch_discretize, power_list, occupancy, launch_noise, launch_plant_rollout, launch_model_rollout, FIT_LDS, launch_fit,
                               ONLINE_LDS, launch_online, launch_plant_grad, launch_model_grad, OBS_KIND, launch_observe, launch_observed_plant, launch_fit_qr,
                               launch_plant_feedback, launch_model_feedback, launch_refit, launch_refit_qr, launch_plant_linearize, launch_plant_qp,
                               launch_plant_step, launch_plant_multi, launch_model_multi, launch_plant_param_grad};
  return &ops;
}

}  // namespace shape_<nx>_<nu>_<order>
}  // namespace m4q

// registration symbol of this shape: m4q_shape_<nx>_<nu>_<order> (linked into libm4q_hip.so), or - the generator-plant object -
// m4q_shapeg_<nx>_<nu>_<order>, which libm4q_hip.so looks up in libm4q_hip_gen.so with dlsym
#ifdef M4Q_VARIANT_GEN
extern "C" __attribute__((visibility("default"))) const m4q::ShapeOps* M4Q_CAT(m4q_shapeg_, M4Q_NX, M4Q_NU, M4Q_ORDER)() {
  return m4q::M4Q_CAT(shape_, M4Q_NX, M4Q_NU, M4Q_ORDER)::shape_ops();
}
#else
extern "C" __attribute__((visibility("hidden"))) const m4q::ShapeOps* M4Q_CAT(m4q_shape_, M4Q_NX, M4Q_NU, M4Q_ORDER)() {
  return m4q::M4Q_CAT(shape_, M4Q_NX, M4Q_NU, M4Q_ORDER)::shape_ops();
}
#endif
