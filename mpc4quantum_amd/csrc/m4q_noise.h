// m4q_noise.h - the device form of mpc4quantum_amd/noise.py (the normative definition): measurement noise drawn by a counter-based
// generator, so that a draw depends on (seed, global member, column of xs, component) and on nothing else - not the launch, the
// resident row, the work item or the rank.
//
//   bits      Philox4x32-10 (Salmon et al., Random123); key (seed lo, seed hi), counter (member lo, member hi, state_index, component)
//   uniforms  u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53 in (0, 1],  u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53 in [0, 1): exact in fp64
//   normal    z = sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2)
//   NOISE_IID        e = sigma z                                          (the reference's set_sigma, experiment.py:212)
//   NOISE_HERMITIAN  e = sigma ((Z + Z^H) / 2 - (Re tr Z / d) I),  Z[a][b] = z of component a d + b: Hermitian, traceless
//
// The integer stage is the replica's bit for bit; log / sqrt / sincospi are the device library's, a few ulps from NumPy's.
// The includer defines m4q::cplx { double re, im; } first.
#pragma once
#include <hip/hip_runtime.h>

namespace m4q {

enum : int { NOISE_IID = 1, NOISE_HERMITIAN = 2 };     // (mirrored in include/m4q.h: M4Q_NOISE_*)

struct Philox4 { unsigned w[4]; };

__device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the unit complex normal of (member, state_index, component)
__device__ inline cplx noise_unit(unsigned long long seed, unsigned long long member, unsigned state_index, unsigned component) {
  const Philox4 p = philox4x32_10((unsigned)member, (unsigned)(member >> 32), state_index, component, (unsigned)seed,
                                  (unsigned)(seed >> 32));
  const double u1 = ((double)(p.w[0] >> 5) * 67108864.0 + (double)(p.w[1] >> 6) + 1.0) * 0x1p-53;
  const double u2 = ((double)(p.w[2] >> 5) * 67108864.0 + (double)(p.w[3] >> 6)) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  cplx z;
  z.re = r * cs; z.im = r * sn;
  return z;
}

// The noise of component `comp` (row-major in the d x d state for NOISE_HERMITIAN; d = 0: only NOISE_IID is meaningful).  No
// cross-lane exchange: a lane evaluates the draw of its transposed component as well, a diagonal lane the d diagonal draws of the
// trace term - in one loop around ONE copy of the generator, whose trip count is wave-uniform (lanes with fewer draws idle).
// Out of line on purpose: inlined into the closed loop's step-done phase, the generator's temporaries (fp64 log and sincospi) sit
// on top of every value that lives across that phase and set the kernel's register allocation - +38 VGPRs on the d = 2 kernels,
// 42 spilled VGPRs in the headline kernel (255, none).  As a call it costs that kernel nothing: 255 VGPRs, no spill, no scratch.
__device__ __attribute__((noinline)) inline cplx noise_sample(int mode, unsigned long long seed, unsigned long long member,
                                                              unsigned state_index, int comp, int d, double sigma) {
  const bool herm = mode == NOISE_HERMITIAN && d > 0;
  const int a = herm ? comp / d : 0, b2 = herm ? comp - a * d : 0;
  const bool diag = herm && a == b2;
  const int trips = herm ? (d > 2 ? d : 2) : 1;
  cplx own, tr;
  own.re = own.im = tr.re = tr.im = 0.0;
  double t = 0.0;
#pragma unroll 1
  for (int i = 0; i < trips; ++i) {
    // diagonal lane: draw i is diagonal entry i; any other lane: its own component, then the transposed one
    const int c = !herm ? comp : diag ? (i < d ? i * d + i : comp) : (i == 0 ? comp : b2 * d + a);
    const cplx z = noise_unit(seed, member, state_index, (unsigned)c);
    if (diag) {
      if (i < d) t += z.re;                    // (summed in index order, as noise.py sums it)
      if (i == a) { own = z; tr = z; }
    } else {
      if (i == 0) own = z;
      if (i == 1) tr = z;
    }
  }
  cplx e = own;
  if (herm) {
    e.re = (own.re + tr.re) * 0.5;
    e.im = (own.im - tr.im) * 0.5;
    if (diag) e.re -= t / (double)d;
  }
  e.re *= sigma; e.im *= sigma;
  return e;
}

}  // namespace m4q
