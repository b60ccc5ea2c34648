"""The host code that decides a session's arithmetic path (csrc/m4q_lift.h: HermBasis, Traceless, LiftStat, DecoupleStat, lift_blocks,
lift_vectors), compiled for the CPU and checked against NumPy for d = 2, 3, 4: the values of both lifted copies, the verdicts on inputs
whose answer NumPy alone gives, and the two thresholds (1e-13 on the imaginary part dropped, 1e-12 on the coupling of the trace
coordinate) pinned from both sides.

W and O are written here from the comments above HermBasis and Traceless, not from their code.

Value tolerance: 1e-14 max(1, max|input|).  An entry of W^H M W is a sum of at most four products with factors 1/sqrt2; the rotation
by O adds sums of at most d products per side: at most n + 4 = 20 products of O(1) factors in all, about 2e-15, a factor five left over."""
import os
import subprocess

import numpy as np
import pytest

from tests.kernel_variants import lindblad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"              # the compiler the library itself is built with

_DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include "m4q_lift.h"
// argv: in out.  in: int32 kind (0 blocks, 1 vectors), d, count, nblk, block0_identity, traceless; then the complex input.
// out: doubles ok[HERM], ok[TRACELESS], tau[0], tau[1], size of v[HERM], size of v[TRACELESS]; then the two arrays.
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[6];
  if (std::fread(h, sizeof(int32_t), 6, f) != 6) return 4;
  const int d = h[1], n = d * d;
  const size_t count = (size_t)h[2], items = h[0] == 0 ? count * n * n * h[3] : count * n;
  std::vector<std::complex<double>> src(items);
  if (std::fread(src.data(), sizeof(std::complex<double>), items, f) != items) return 5;
  std::fclose(f);
  const m4q::lift::Lift L = h[0] == 0 ? m4q::lift::lift_blocks(d, src.data(), count, h[3], h[4] != 0, h[5] != 0)
                                      : m4q::lift::lift_vectors(d, src.data(), count, h[5] != 0);
  const std::vector<double>&vh = L.v[m4q::COORDS_HERM], &vt = L.v[m4q::COORDS_TRACELESS];
  const double head[6] = {(double)L.ok[m4q::COORDS_HERM], (double)L.ok[m4q::COORDS_TRACELESS], L.tau[0], L.tau[1], (double)vh.size(),
                          (double)vt.size()};
  f = std::fopen(argv[2], "wb");
  if (!f) return 6;
  std::fwrite(head, sizeof(double), 6, f);
  std::fwrite(vh.data(), sizeof(double), vh.size(), f);
  std::fwrite(vt.data(), sizeof(double), vt.size(), f);
  return std::fclose(f) == 0 ? 0 : 7;
}
'''


class _Lifted:
    def __init__(self, out):
        self.ok_herm, self.ok_tl = bool(out[0]), bool(out[1])
        self.tau = out[2:4]
        nh, nt = int(out[4]), int(out[5])
        self.herm, self.tl = out[6:6 + nh], out[6 + nh:6 + nh + nt]
        assert out.size == 6 + nh + nt


@pytest.fixture(scope="module")
def lift(tmp_path_factory):
    """The header compiled with the plain host compiler (no HIP include path: it must not need one); returns the two entry points."""
    tmp = tmp_path_factory.mktemp("lift")
    (tmp / "driver.cpp").write_text(_DRIVER)
    exe = str(tmp / "lift_host")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "mpc4quantum_amd", "csrc"),
                    str(tmp / "driver.cpp"), "-o", exe], check=True)
    calls = [0]

    def run(kind, d, src, nblk, block0_identity, traceless):
        calls[0] += 1
        fin, fout = str(tmp / ("in%d.bin" % calls[0])), str(tmp / ("out%d.bin" % calls[0]))
        src = np.ascontiguousarray(src, dtype=np.complex128)
        n = d * d
        count = src.size // (n * n * nblk) if kind == 0 else src.size // n
        with open(fin, "wb") as f:
            np.array([kind, d, count, nblk, int(block0_identity), int(traceless)], dtype=np.int32).tofile(f)
            src.tofile(f)
        subprocess.run([exe, fin, fout], check=True)
        return _Lifted(np.fromfile(fout, dtype=np.float64))

    class Entry:
        @staticmethod
        def blocks(d, src, nblk, block0_identity, traceless=True):
            """src [count][n][nblk n]: nblk blocks side by side"""
            return run(0, d, src, nblk, block0_identity, traceless)

        @staticmethod
        def vectors(d, src, traceless=True):
            return run(1, d, src, 1, False, traceless)
    return Entry


# ---------------------------------------------------------------- NumPy definitions
def basis_W(d):
    """x = W r.  Slot c = a d + b of r:  a == b: rho_aa;  a < b: sqrt2 Re rho_ab;  a > b: sqrt2 Im rho_ab  (x = vec(rho), row-major)."""
    n = d * d
    W = np.zeros((n, n), dtype=complex)
    for a in range(d):
        for b in range(d):
            c = a * d + b
            if a == b:
                W[c, c] = 1.0
            elif a < b:                       # rho_ab = rho_ba^* = (r_c + i r_c') / sqrt2 with c' the slot (b, a): the real part
                W[a * d + b, c] = W[b * d + a, c] = 1 / np.sqrt(2)
            else:                             # slot (a, b), a > b, holds sqrt2 Im rho_ab: rho_ab gets + i, rho_ba - i
                W[a * d + b, c] = 1j / np.sqrt(2)
                W[b * d + a, c] = -1j / np.sqrt(2)
    return W


def rotation_O(d):
    """Identity off the diagonal slots (a, a); on them O[a][0] = 1/sqrt(d), O[a][l] = 1/sqrt(l(l+1)) (a < l), -l/sqrt(l(l+1)) (a == l),
    0 (a > l)."""
    n = d * d
    O = np.eye(n)
    for a in range(d):
        for l in range(d):
            if l == 0:
                v = 1 / np.sqrt(d)
            else:
                v = 1 / np.sqrt(l * (l + 1)) if a < l else (-l / np.sqrt(l * (l + 1)) if a == l else 0.0)
            O[a * d + a, l * d + l] = v
    return O


@pytest.mark.parametrize("d", [2, 3, 4])
def test_W_is_unitary_and_O_orthogonal(d):
    W, O = basis_W(d), rotation_O(d)
    n = d * d
    assert np.abs(W.conj().T @ W - np.eye(n)).max() <= 1e-15 and np.abs(O.T @ O - np.eye(n)).max() <= 1e-15
    rng = np.random.default_rng(d)
    rho = _density(d, rng)
    r = W.conj().T @ rho.reshape(-1)
    assert np.abs(r.imag).max() <= 1e-15 and abs((O.T @ r.real)[0] - 1 / np.sqrt(d)) <= 1e-15      # coordinate 0: trace / sqrt(d)


# ---------------------------------------------------------------- inputs
def _herm(d, rng):
    M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return 0.5 * (M + M.conj().T)


def _density(d, rng):
    M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    rho = M @ M.conj().T
    rho = 0.5 * (rho + rho.conj().T)                                # (exactly Hermitian)
    return rho / np.trace(rho).real


def _liouvillian(H):
    """-i [H, .] on vec(rho), row-major: vec(A rho B) = (A (x) B^T) vec(rho)"""
    eye = np.eye(H.shape[0])
    return -1j * (np.kron(H, eye) - np.kron(eye, H.T))


def _model(d, rng, m, count, dt=0.05, damping=0.0):
    """[count][n][(1 + m) n]: first-order models [I + dt L0 | dt L1 ...] of Liouvillians of random Hermitian H, with an
    amplitude-damping dissipator (the lowering operator) of rate `damping` added to L0"""
    n = d * d
    out = np.zeros((count, n, (1 + m) * n), dtype=complex)
    lower = np.diag(np.sqrt(np.arange(1.0, d)), 1)
    for it in range(count):
        for k in range(1 + m):
            L = _liouvillian(_herm(d, rng))
            if k == 0:
                L = np.eye(n) / dt + L + damping * lindblad(lower)
            out[it, :, k * n:(k + 1) * n] = dt * L
    return out


def _blocks_of(M, n):
    """[count][n][nblk n] -> [count][nblk][n][n]"""
    count, _, w = M.shape
    return M.reshape(count, n, w // n, n).transpose(0, 2, 1, 3)


def _side_by_side(blocks):
    """[count][nblk][n][n] -> [count][n][nblk n]"""
    count, nblk, n, _ = blocks.shape
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(count, n, nblk * n))


def _expect_blocks(d, M):
    """NumPy's lift of [count][n][nblk n]: the complex W^H M W per block, and O^T Re(.) O per block"""
    n = d * d
    W, O = basis_W(d), rotation_O(d)
    blocks = _blocks_of(M, n)
    herm = W.conj().T @ blocks @ W
    return herm, O.T @ herm.real @ O


def _real_enough(herm):
    return np.abs(herm.imag).max() <= 1e-13 * max(1.0, np.abs(herm).max())


def _decoupled(rot, block0_identity):
    want = np.zeros_like(rot)
    if block0_identity:
        want[:, 0, 0, 0] = 1.0
    worst = max(np.abs(rot - want)[:, :, 0, :].max(), np.abs(rot - want)[:, :, :, 0].max())
    return worst <= 1e-12 * max(1.0, np.abs(rot).max())


def _tol(src):
    return 1e-14 * max(1.0, np.abs(src).max())


def _check_block_values(d, M, got, traceless_copy):
    n = d * d
    herm, rot = _expect_blocks(d, M)
    count, nblk = herm.shape[:2]
    assert np.abs(got.herm.reshape(count, n, nblk * n) - _side_by_side(herm.real)).max() <= _tol(M)
    if traceless_copy:
        assert np.abs(got.tl.reshape(count, n - 1, nblk * (n - 1)) - _side_by_side(rot[:, :, 1:, 1:])).max() <= _tol(M)
    else:
        assert got.tl.size == 0


# ---------------------------------------------------------------- values and verdicts
@pytest.mark.parametrize("d", [2, 3, 4])
def test_liouvillian_model_qualifies_on_both_coordinate_systems(lift, d):
    M = _model(d, np.random.default_rng(10 + d), m=2, count=3)
    herm, rot = _expect_blocks(d, M)
    assert np.abs(herm.imag).max() <= 1e-15 and _real_enough(herm) and _decoupled(rot, True)       # NumPy alone says so
    got = lift.blocks(d, M, 3, True)
    assert got.ok_herm and got.ok_tl
    _check_block_values(d, M, got, True)
    # block0_identity off: block 0 carries the trace coordinate through, which a block that must not touch it may not
    assert not _decoupled(rot, False)
    got = lift.blocks(d, M, 3, False)
    assert got.ok_herm and not got.ok_tl
    # traceless copy not asked for: none made
    got = lift.blocks(d, M, 3, True, traceless=False)
    assert got.ok_herm and not got.ok_tl and got.tl.size == 0


@pytest.mark.parametrize("d", [2, 3, 4])
def test_non_unital_model_qualifies_on_the_hermitian_basis_alone(lift, d):
    M = _model(d, np.random.default_rng(20 + d), m=1, count=2, damping=0.3)
    herm, rot = _expect_blocks(d, M)
    assert _real_enough(herm)
    assert np.abs(rot[:, :, 0, 1:]).max() <= 1e-15                  # trace preserving: nothing feeds the trace coordinate
    assert np.abs(rot[:, 0, 1:, 0]).max() > 1e-3                    # not unital: the trace coordinate feeds the others (column 0)
    assert not _decoupled(rot, True)
    got = lift.blocks(d, M, 2, True)
    assert got.ok_herm and not got.ok_tl
    _check_block_values(d, M, got, True)                            # (the copy is made, and marked unusable)


@pytest.mark.parametrize("d", [2, 3, 4])
def test_random_complex_blocks_qualify_nowhere(lift, d):
    rng = np.random.default_rng(30 + d)
    n = d * d
    M = rng.standard_normal((2, n, 3 * n)) + 1j * rng.standard_normal((2, n, 3 * n))
    herm, _ = _expect_blocks(d, M)
    assert not _real_enough(herm)
    got = lift.blocks(d, M, 3, False)
    assert not got.ok_herm and not got.ok_tl
    _check_block_values(d, M, got, False)                           # the Hermitian copy is W^H M W all the same; no traceless copy


@pytest.mark.parametrize("d", [2, 3, 4])
def test_vectors(lift, d):
    rng = np.random.default_rng(40 + d)
    n = d * d
    W, O = basis_W(d), rotation_O(d)
    rhos = np.stack([_density(d, rng).reshape(-1) for _ in range(3)])
    r = rhos @ W.conj()                                             # rows (W^H v)^T
    assert np.abs(r.imag).max() <= 1e-15
    got = lift.vectors(d, rhos)
    assert got.ok_herm and got.ok_tl
    assert np.abs(got.herm.reshape(3, n) - r.real).max() <= _tol(rhos)
    rot = r.real @ O                                                # rows (O^T r)^T
    assert np.abs(got.tl.reshape(3, n - 1) - rot[:, 1:]).max() <= _tol(rhos)
    assert abs(got.tau[0] - rot[:, 0].min()) <= _tol(rhos) and abs(got.tau[1] - rot[:, 0].max()) <= _tol(rhos)
    assert abs(got.tau[0] - 1 / np.sqrt(d)) <= 1e-15 and abs(got.tau[1] - 1 / np.sqrt(d)) <= 1e-15
    # states of different trace: tau is the range of coordinate 0
    scaled = rhos * np.array([1.0, 0.5, 2.0])[:, None]
    got = lift.vectors(d, scaled)
    assert got.ok_herm and abs(got.tau[0] - 0.5 / np.sqrt(d)) <= 1e-15 and abs(got.tau[1] - 2 / np.sqrt(d)) <= 1e-15
    # a random complex vector is no Hermitian matrix
    v = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    lifted = v @ W.conj()
    assert np.abs(lifted.imag).max() > 1e-3
    got = lift.vectors(d, v)
    assert not got.ok_herm and not got.ok_tl and got.tl.size == 0
    assert np.abs(got.herm.reshape(2, n) - lifted.real).max() <= _tol(v)


@pytest.mark.parametrize("d", [2, 3, 4])
def test_cost_identity_and_block0_identity(lift, d):
    """Q = I: O^T I O = I has a one in the corner, which only a block that carries the trace coordinate through may have."""
    n = d * d
    Q = np.eye(n, dtype=complex)[None]
    _, rot = _expect_blocks(d, Q)
    assert _decoupled(rot, True) and not _decoupled(rot, False)
    assert lift.blocks(d, Q, 1, True).ok_tl and not lift.blocks(d, Q, 1, False).ok_tl
    got = lift.blocks(d, Q, 1, False)
    assert got.ok_herm and np.abs(got.tl.reshape(n - 1, n - 1) - np.eye(n - 1)).max() <= 1e-14


# ---------------------------------------------------------------- the thresholds, from both sides
@pytest.mark.parametrize("d", [2, 3, 4])
def test_thresholds_are_where_the_header_says(lift, d):
    """One lifted entry is moved and the input rebuilt from it with W and O in NumPy, so that exactly that entry differs after the
    lift.  The perturbations sit a factor of 100 on either side of 1e-13 (imaginary part dropped, LiftStat) and 1e-12 (coupling of the
    trace coordinate, DecoupleStat).  The inverse transform rounds by about 1e-15 itself: that is why the passing perturbations are
    1e-15 and 1e-14, a factor of 100 under the thresholds, and not closer - closer, the rounding would decide."""
    n = d * d
    W, O = basis_W(d), rotation_O(d)
    M = _model(d, np.random.default_rng(50 + d), m=1, count=1)
    herm, rot = _expect_blocks(d, M)
    scale = max(1.0, np.abs(herm).max())
    assert scale < 10.0                                             # (the thresholds are relative to max(1, scale))

    def back(h):                                                    # [count][nblk][n][n] lifted -> the model
        return _side_by_side(W @ h @ W.conj().T)

    for eps, ok in ((1e-11, False), (1e-15, True)):
        h = herm.copy()
        h[0, 1, 2, 1] += 1j * eps
        Mp = back(h)
        again, _ = _expect_blocks(d, Mp)
        assert abs(again[0, 1, 2, 1].imag - eps) <= 2e-15 and (np.abs(again.imag).max() > 1e-13 * scale) == (not ok)
        got = lift.blocks(d, Mp, 2, True)
        assert got.ok_herm == ok and got.ok_tl == ok, eps
    for eps, ok in ((1e-10, False), (1e-14, True)):
        r = rot.copy()
        r[0, 1, 0, n - 1] += eps                                    # row 0 of the second block: something feeds the trace coordinate
        Mp = back((O @ r @ O.T).astype(complex))
        _, again = _expect_blocks(d, Mp)
        assert abs(again[0, 1, 0, n - 1] - eps) <= 2e-15 and _decoupled(again, True) == ok
        got = lift.blocks(d, Mp, 2, True)
        assert got.ok_herm and got.ok_tl == ok, eps
