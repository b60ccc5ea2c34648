"""Batched DMDc identification: trajectories and controls of B members in, their models out, in ONE launch
(m4q_dmdc_fit_batch) - `DiscrepDMDc.from_data(X2, X1, krtimes(U1, X1), rcond=...)` for an ensemble and a whole grid of rcond.

This module is the normative definition of what the kernel computes (csrc/m4q_fit.h reproduces it, in the same order of
operations), as noise.py is for the generator.  Per member, with E experiments of N steps (xs [E, N + 1, n] complex, u [E, N, m]
real, optional u_scale [m]: the member sees u_scale[k] u[t][k], one fp64 product):

  snapshots   z = [x_t ; lift(u_t) (x) x_t] for every (e, t), e outer, t inner; lift(u) = the non-constant monomials in
              create_power_list(order, m) order (WrapModel.lift_u), the Kronecker rows as krtimes numbers them (p n + j):
              nz = n (1 + P).
  Gram data   G = sum z z^H (nz x nz; the upper triangle is accumulated, the lower is its conjugate, the diagonal real) and
              C = sum x_{t+1} z^H (n x nz).
  spectrum    G = V diag(lam) V^H by cyclic-by-rows Jacobi with complex Hermitian rotations (p < q, p outer).  A rotation is
              skipped when |g_pq|^2 <= eps^2 |g_pp g_qq|; the solver stops after a sweep that skipped every rotation, and after
              MAX_SWEEPS = 30 sweeps in any case (status 1).
  models      for each rcond: keep lam_k > rcond^2 max(lam);  A = sum over the kept k, ascending, of (W[:, k] / lam_k) V[:, k]^H
              with W = C V;  rank = the number kept.  This is Y pinv(Z, rcond): s_k = sqrt(lam_k), and numpy cuts at
              s > rcond s_max.
  svals       s_k = sqrt(sum |v_k^H z|^2) over the snapshots in their order, descending: lam_k = v_k^H G v_k taken from the data
              themselves, a sum of non-negative terms, so a singular value that vanishes comes back at ~eps s_0 and not at
              sqrt of G's rounding floor (~1e-8 s_0).  The ranks and the models are decided by lam alone.

The decomposition is done once, every rcond costs one truncated product.  rcond must lie in [RCOND_MIN, 1) = [1e-7, 1): below that
the cut-off rcond^2 sits in the Gram matrix's own rounding floor (~ nz eps relative to max(lam)) and the rank is no longer
decidable from G.  The host `DiscrepDMDc.from_data` (an SVD of Z itself) remains the path for rcond = 1e-15.

The QR route (method="qr", m4q_dmdc_fit_qr_batch; dmdc_fit_qr_reference is its definition, csrc/m4q_fit_qr.h reproduces it) takes
the same fit from the data themselves, so that its error is O(eps kappa) and not O(eps kappa^2):
  QR          R = 0 [nz, nz], T = 0 [nz, n]; every snapshot, in the same order, contributes the row (z^H | x_{t+1}^H), rotated in by
              Givens rotations j = 0 .. nz - 1: a = R[j, j], b = row[j] (skipped when b == 0), h = sqrt(|a|^2 + |b|^2), c = a / h,
              s = b / h, R[j, j:] <- conj(c) R[j, j:] + conj(s) row[j:], row[j:] <- c row[j:] - s R[j, j:] (the old R[j, j:]), the same
              on T[j] and the right-hand side.  Then Z^H = Q R, T = Q^H Y^H, and R has Z's singular values.  (Rows z^T | y^T and a
              conjugate on the final product would be the same numbers, bit for bit.)
  spectrum    one-sided (Hestenes) Jacobi on the columns of M = R, V = I accumulated, pairs cyclic by rows: a_pp = m_p^H m_p,
              a_qq = m_q^H m_q, g = m_p^H m_q (each a lane_sum over the nz axis); skipped when |g|^2 <= eps^2 a_pp a_qq, otherwise
              jacobi_hermitian's rotation on columns p, q of M and V; the same stopping rule and cap.
  models      lam_k = m_k^H m_k; per rcond keep lam_k > rcond^2 max(lam); A = sum over the kept k, ascending, of
              (W[:, k] / lam_k) V[:, k]^H with W = T^H M.  svals = sqrt(lam) descending: no second pass, this route has no floor.
rcond must lie in [RCOND_MIN_QR, 1) = [1e-12, 1): the singular values come out to a few eps s_0, so a cut-off a factor 1.2 from every
singular value is decidable down to about 1e3 eps; numpy's default 1e-15 lies inside the rounding of the data themselves and stays
a host call.  status 3: R or T has a non-finite entry.  Data that are exactly rank-deficient (fewer snapshots than nz) can reach the
cap: null columns are rotated until they underflow; the models at the cap are good.

status per member: 0 ok; 1 the Jacobi iteration hit its cap (the models are written from the last iterate); 3 non-finite data
(G or C has a non-finite entry, which any non-finite sample produces): the models are zero and the rank is 0.

Prior model (A0, discount, counts; m4q_dmdc_refit_batch / m4q_dmdc_refit_qr_batch): one DiscrepDMDc.fit_iteration (model.py),
A <- A0 + (Y - A0 Z) pinv(Z, rcond) on the discounted stacks = A0 (I - Pi_r) + Y Z_r^+: the fit where the data excited the plant,
the prior everywhere else.  With any of the three given (A0 defaults to 0, discount to 1):
  counts      member b takes t < counts[b] of every experiment, as online_dmdc_batch does; the others stream past.
  discount    snapshot s of the S taken has weight discount^(S-1-s), as a recurrence: before a snapshot is accumulated
              G <- d2 G, C <- d2 C and the sums behind svals likewise, with d2 = discount * discount formed once per member, each a
              rounded product of its own; the QR route: R <- discount R, T <- discount T before the snapshot's rotations.
  discrepancy Gram route, after G and C are accumulated: D[i][l] = C[i][l] - sum_k A0[i][k] G[k][l], k ascending, the terms
              subtracted one at a time from C[i][l] (as online.update forms r); D takes C's place.  QR route, after the Givens
              phase: T[j][i] <- T[j][i] - sum_{k >= j} R[j][k] conj(A0[i][k]), k ascending.  Spectrum, ranks, svals (those of the
              weighted stack) and truncated products as above; A0 is added once per entry at the end.
status 3 also when A0 has a non-finite entry.  counts[b] = 0: models = A0, rank 0, status 0."""
import numpy as np

from . import _lib
from .library import create_power_list, size_of_library
from .rollout import model_rollout_batch

RCOND_MIN = 1e-7
RCOND_MIN_QR = 1e-12
METHODS = ("gram", "qr")
MAX_RCONDS = 16
MAX_SWEEPS = 30
_EPS = float(np.finfo(np.float64).eps)


def lift_controls(u, order):
    """u [..., m] -> the P non-constant monomials [..., P] in create_power_list order; the powers as repeated products
    u (u (u ...)), the factors taken over the controls in their order."""
    u = np.asarray(u, dtype=np.float64)
    m = u.shape[-1]
    out = []
    for powers in create_power_list(order, m)[1:]:
        v = np.ones(u.shape[:-1])
        for k in range(m):
            w = np.ones(u.shape[:-1])
            for _ in range(int(powers[k])):
                w = u[..., k] * w
            v = v * w
        out.append(v)
    return np.stack(out, axis=-1)


def stack_snapshots(xs, u, order):
    """One member's Z [nz, E N] and Y = X2 [n, E N] in the (e, t) order of the sums; xs [E, N + 1, n], u [E, N, m] as the member
    sees them."""
    E, N1, n = xs.shape
    pu = lift_controls(u, order)                                                      # [E, N, P]
    x1 = xs[:, :-1, :]
    z = np.concatenate([x1[:, :, None, :], pu[:, :, :, None] * x1[:, :, None, :]], axis=2)     # [E, N, 1 + P, n]
    return z.reshape(E * (N1 - 1), -1).T, xs[:, 1:, :].reshape(E * (N1 - 1), n).T


def gram(Z, Y, d2=None):
    """G = sum z z^H and C = sum y z^H over the columns in their order; d2: G <- d2 G, C <- d2 C before every column."""
    nz, S = Z.shape
    G = np.zeros((nz, nz), dtype=np.complex128)
    C = np.zeros((Y.shape[0], nz), dtype=np.complex128)
    for s in range(S):
        if d2 is not None:
            G *= d2
            C *= d2
        G += np.outer(Z[:, s], Z[:, s].conj())
        C += np.outer(Y[:, s], Z[:, s].conj())
    iu = np.triu_indices(nz, 1)
    G[(iu[1], iu[0])] = G[iu].conj()
    G[np.diag_indices(nz)] = G[np.diag_indices(nz)].real
    return G, C


def jacobi_hermitian(G):
    """Cyclic-by-rows Jacobi on a Hermitian matrix.  Returns (lam [nz], V [nz, nz], sweeps, converged): G = V diag(lam) V^H;
    `sweeps` counts every sweep made, the last, all-skipped one included."""
    G = np.array(G, dtype=np.complex128)
    nz = G.shape[0]
    V = np.eye(nz, dtype=np.complex128)
    others = np.arange(nz)
    for sweep in range(1, MAX_SWEEPS + 1):
        rotated = False
        for p in range(nz - 1):
            for q in range(p + 1, nz):
                g = G[p, q]
                app, aqq = G[p, p].real, G[q, q].real
                m2 = g.real * g.real + g.imag * g.imag
                if m2 <= _EPS * _EPS * abs(app * aqq):
                    continue
                rotated = True
                absg = np.sqrt(m2)
                w = complex(g.real / absg, g.imag / absg)
                tau = (aqq - app) / (2.0 * absg)
                t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                sw = complex(t * c * w.real, t * c * w.imag)
                k = others[(others != p) & (others != q)]
                gp, gq = G[k, p].copy(), G[k, q].copy()
                G[k, p] = c * gp - sw.conjugate() * gq
                G[k, q] = sw * gp + c * gq
                G[p, k] = G[k, p].conj()
                G[q, k] = G[k, q].conj()
                G[p, p] = app - t * absg
                G[q, q] = aqq + t * absg
                G[p, q] = G[q, p] = 0.0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - sw.conjugate() * vq
                V[:, q] = sw * vp + c * vq
        if not rotated:
            return G.diagonal().real.copy(), V, sweep, True
    return G.diagonal().real.copy(), V, MAX_SWEEPS, False


def singular_values(V, Z, d2=None):
    """s_k = sqrt(sum over the snapshots, in their order, of |v_k^H z|^2), descending: the Rayleigh quotients v_k^H G v_k taken
    from the data themselves, every term non-negative (the inner products summed over the rows of V in ascending index).
    d2: the sums are scaled by it before every snapshot, as gram() scales G."""
    nz, S = Z.shape
    acc = np.zeros(nz)
    for s in range(S):
        if d2 is not None:
            acc = acc * d2
        d = np.zeros(nz, dtype=np.complex128)
        for j in range(nz):
            d += V[j, :].conj() * Z[j, s]
        acc += d.real * d.real + d.imag * d.imag
    return np.sqrt(np.sort(acc)[::-1])


def truncated_products(lam, Wl, V, rconds):
    """A [R, n, nz] and rank [R] from the spectrum and Wl = W / lam: the sums run over the kept k in ascending index."""
    lmax = lam.max()
    A = np.zeros((len(rconds),) + Wl.shape, dtype=np.complex128)
    rank = np.zeros(len(rconds), dtype=np.int32)
    for r, rc in enumerate(rconds):
        keep = lam > (rc * rc) * lmax
        rank[r] = int(keep.sum())
        for k in np.nonzero(keep)[0]:
            A[r] += np.outer(Wl[:, k], V[:, k].conj())
    return A, rank


def truncated_models(lam, V, C, rconds):
    """A [R, n, nz] and rank [R] from the spectrum: the sums run over the kept eigenpairs in ascending index."""
    W = np.zeros(C.shape, dtype=np.complex128)
    for j in range(V.shape[0]):
        W += np.outer(C[:, j], V[j, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        Wl = W * (1.0 / lam)[None, :]
    return truncated_products(lam, Wl, V, rconds)


# ---------------------------------------------------------------- the QR route (m4q_dmdc_fit_qr_batch, csrc/m4q_fit_qr.h)
def givens_qr(Z, Y, discount=None):
    """Row-wise Givens QR of the stacked data, one snapshot at a time in their order: the snapshot contributes the row
    (z^H | y^H) (the conjugated columns of Z [nz, S] and Y [n, S]), rotated into R [nz, nz] (upper triangular, real diagonal)
    and T [nz, n] by nz dependent rotations.  Afterwards Z^H = Q R and T = Q^H Y^H, and R has Z's singular values.
    discount: R <- discount R, T <- discount T before every snapshot's rotations."""
    nz, S = Z.shape
    R = np.zeros((nz, nz), dtype=np.complex128)
    T = np.zeros((nz, Y.shape[0]), dtype=np.complex128)
    for s in range(S):
        if discount is not None:
            R *= discount
            T *= discount
        row = Z[:, s].conj()
        rhs = Y[:, s].conj()
        for j in range(nz):
            b = row[j]
            if b == 0:
                continue
            a = R[j, j]
            h = np.sqrt((a.real * a.real + a.imag * a.imag) + (b.real * b.real + b.imag * b.imag))
            c = complex(a.real / h, a.imag / h)
            sn = complex(b.real / h, b.imag / h)
            cc, sc = c.conjugate(), sn.conjugate()
            rj, tj = R[j, j:].copy(), T[j].copy()
            R[j, j:] = cc * rj + sc * row[j:]
            row[j:] = c * row[j:] - sn * rj
            T[j] = cc * tj + sc * rhs
            rhs = c * rhs - sn * tj
    return R, T


def lane_sum(v):
    """The sum over the nz axis (last, at most 64 long) in the wavefront's order: lane l holds entry l; the 16 lanes of each DPP
    row are added in ascending order, then the four row sums in ascending order."""
    pad = np.zeros(v.shape[:-1] + (64,))
    pad[..., :v.shape[-1]] = v
    rows = np.cumsum(pad.reshape(v.shape[:-1] + (4, 16)), axis=-1)[..., -1]
    return ((rows[..., 0] + rows[..., 1]) + rows[..., 2]) + rows[..., 3]


def column_products(mp, mq):
    """(m_p^H m_p, m_q^H m_q, Re m_p^H m_q, Im m_p^H m_q) of two columns, each summed by lane_sum."""
    return lane_sum(np.stack([mp.real * mp.real + mp.imag * mp.imag, mq.real * mq.real + mq.imag * mq.imag,
                              mp.real * mq.real + mp.imag * mq.imag, mp.real * mq.imag - mp.imag * mq.real]))


def jacobi_one_sided(R):
    """One-sided (Hestenes) Jacobi on the columns of M = R, cyclic by rows, with jacobi_hermitian's rotation and skip rule applied
    to the implicit Gram matrix M^H M.  Returns (M [nz, nz], V [nz, nz], sweeps, converged): R V = M, the columns of M
    orthogonal; `sweeps` counts every sweep made, the last, all-skipped one included."""
    M = np.array(R, dtype=np.complex128)
    nz = M.shape[0]
    V = np.eye(nz, dtype=np.complex128)
    for sweep in range(1, MAX_SWEEPS + 1):
        rotated = False
        for p in range(nz - 1):
            for q in range(p + 1, nz):
                mp, mq = M[:, p].copy(), M[:, q].copy()
                app, aqq, gre, gim = column_products(mp, mq)
                m2 = gre * gre + gim * gim
                if m2 <= _EPS * _EPS * (app * aqq):
                    continue
                rotated = True
                absg = np.sqrt(m2)
                w = complex(gre / absg, gim / absg)
                tau = (aqq - app) / (2.0 * absg)
                t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                sw = complex(t * c * w.real, t * c * w.imag)
                M[:, p] = c * mp - sw.conjugate() * mq
                M[:, q] = sw * mp + c * mq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - sw.conjugate() * vq
                V[:, q] = sw * vp + c * vq
        if not rotated:
            return M, V, sweep, True
    return M, V, MAX_SWEEPS, False


def qr_models(M, V, T, rconds):
    """(A [R, n, nz], rank [R], lam [nz]) from the orthogonalised factor: lam_k = m_k^H m_k (lane_sum), W = T^H M summed over the
    rows in ascending index, A = sum over the kept k, ascending, of (W[:, k] / lam_k) V[:, k]^H."""
    lam = lane_sum((M.real * M.real + M.imag * M.imag).T)
    W = np.zeros((T.shape[1], M.shape[0]), dtype=np.complex128)
    for j in range(M.shape[0]):
        W += np.outer(T[j].conj(), M[j, :])
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        Wl = W * (1.0 / lam)[None, :]
    A, rank = truncated_products(lam, Wl, V, rconds)
    return A, rank, lam


# ---------------------------------------------------------------- the prior model (m4q_dmdc_refit_batch, m4q_dmdc_refit_qr_batch)
def taken_snapshots(Z, Y, E, steps):
    """The columns (e, t) with t < steps of Z [nz, E N] and Y [n, E N], in their order."""
    N = Z.shape[1] // E
    keep = (np.arange(E * N) % N) < steps
    return Z[:, keep], Y[:, keep]


def gram_discrepancy(G, C, A0):
    """D = C - A0 G, the cross-Gram matrix of the discrepancy Y - A0 Z: the terms k = 0, 1, ... subtracted one at a time from C."""
    D = C.copy()
    for k in range(G.shape[0]):
        D -= np.outer(A0[:, k], G[k, :])
    return D


def qr_discrepancy(R, T, A0):
    """T - R A0^H, the discrepancy's Q^H (Y - A0 Z)^H: T[j][i] - sum_{k >= j} R[j][k] conj(A0[i][k]), k ascending."""
    T = T.copy()
    for k in range(R.shape[0]):
        T[:k + 1] -= np.outer(R[:k + 1, k], A0[:, k].conj())
    return T


def _check_prior(B, N, n, nz, A0, discount, counts):
    """Shapes and values of the prior's arguments; None when none is given, else a dict: "A0" [B|1, n, nz] (zero by default),
    "discount" [B|1] (1 by default), "counts" [B] int32 or None, and the per-member flags."""
    if A0 is None and discount is None and counts is None:
        return None
    if A0 is None:
        A0 = np.zeros((n, nz), dtype=np.complex128)
    A0 = np.ascontiguousarray(A0, dtype=np.complex128)
    if A0.shape not in ((n, nz), (B, n, nz)):
        raise ValueError("A0 must be [n, nz] = (%d, %d) or [B, n, nz] with B = %d, got %s" % (n, nz, B, A0.shape))
    discount = np.asarray(1.0 if discount is None else discount, dtype=np.float64)
    if discount.shape not in ((), (B,)):
        raise ValueError("discount must be a scalar or [B] = (%d,), got shape %s" % (B, discount.shape))
    if not np.all((discount > 0.0) & (discount <= 1.0)):
        raise ValueError("discount must lie in (0, 1], got %s" % (discount,))
    if counts is not None:
        c = np.asarray(counts)
        if c.shape != (B,) or not np.issubdtype(c.dtype, np.integer):
            raise ValueError("counts must be [B] = (%d,) integers, got shape %s of %s" % (B, c.shape, c.dtype))
        if np.any((c < 0) | (c > N)):
            raise ValueError("counts must lie in [0, N = %d], got %s" % (N, c))
        counts = np.ascontiguousarray(c, dtype=np.int32)
    return {"A0": A0.reshape((-1, n, nz)), "A0_per": int(A0.ndim == 3 and B > 1), "discount": np.ascontiguousarray(discount.reshape(-1)),
            "discount_per": int(discount.ndim == 1 and B > 1), "counts": counts}


def _member_prior(prior, b, N):
    """(A0 [n, nz], discount, steps) of member b."""
    return (prior["A0"][b if prior["A0_per"] else 0], float(prior["discount"][b if prior["discount_per"] else 0]),
            N if prior["counts"] is None else int(prior["counts"][b]))


def _method(method):
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (METHODS, method))
    return method


def _check(xs, us, order, rcond, u_scale, method="gram"):
    """Shapes and values of a fit call; returns (xs [B, E, N + 1, n], us [B|1, E, N, m], u_per, u_scale, rconds, scalar_rcond).
    The rcond range is the method's: [RCOND_MIN, 1) for "gram", [RCOND_MIN_QR, 1) for "qr"."""
    order = int(order)
    if order < 1:
        raise ValueError("order must be at least 1, got %d" % order)
    xs = np.ascontiguousarray(xs, dtype=np.complex128)
    if xs.ndim == 3:
        xs = xs[:, None]
    if xs.ndim != 4 or min(xs.shape) < 1 or xs.shape[2] < 2:
        raise ValueError("xs must be [B, N + 1, n] or [B, E, N + 1, n] with N >= 1, got shape %s" % (xs.shape,))
    B, E, N1, n = xs.shape
    N = N1 - 1
    us = np.ascontiguousarray(us, dtype=np.float64)
    if us.ndim == 2:
        us = us[None, None]
    elif us.ndim == 3:                      # [E, N, m] shared by the ensemble, or - a single experiment - [B, N, m]
        us = us[None] if (E > 1 or us.shape[0] != B) else us[:, None]
    if us.ndim != 4 or us.shape[0] not in (1, B) or us.shape[1:3] != (E, N) or us.shape[3] < 1:
        raise ValueError("us must be [N, m], [E, N, m] (one set for the ensemble) or [B, E, N, m] with B = %d, E = %d, N = %d, "
                         "got shape %s" % (B, E, N, us.shape))
    m = us.shape[3]
    u_per = 1 if (us.shape[0] == B and B > 1) else 0
    if u_scale is not None:
        u_scale = np.ascontiguousarray(u_scale, dtype=np.float64)
        if u_scale.shape != (B, m):
            raise ValueError("u_scale must be [B, m] = (%d, %d), got %s" % (B, m, u_scale.shape))
    rc = np.asarray(rcond, dtype=np.float64)
    scalar = rc.ndim == 0
    rconds = np.ascontiguousarray(rc.reshape(-1) if rc.ndim <= 1 else rc)
    if rconds.ndim != 1 or not 1 <= rconds.shape[0] <= MAX_RCONDS:
        raise ValueError("rcond must be a scalar or a 1-D array of 1 to %d values, got shape %s" % (MAX_RCONDS, rc.shape))
    if method == "qr":
        if not np.all((rconds >= RCOND_MIN_QR) & (rconds < 1.0)):
            raise ValueError("rcond must lie in [%g, 1) with method=\"qr\": below that (numpy's default 1e-15 included) the cut-off "
                             "is inside the rounding of the data themselves (use the host DiscrepDMDc.from_data), got %s"
                             % (RCOND_MIN_QR, rconds))
    elif not np.all((rconds >= RCOND_MIN) & (rconds < 1.0)):
        raise ValueError("rcond must lie in [%g, 1): below that the cut-off is in the Gram matrix's rounding floor (use the host "
                         "DiscrepDMDc.from_data), got %s" % (RCOND_MIN, rconds))
    return xs, us, u_per, u_scale, rconds, scalar, order


def _result(models, rank, svals, status, scalar):
    return {"models": models[0] if scalar else models, "rank": rank[0] if scalar else rank, "svals": svals, "status": status}


def dmdc_fit_reference(xs, us, order, rcond, u_scale=None, A0=None, discount=None, counts=None):
    """The definition above in NumPy, member by member.  Arguments and result as dmdc_fit_batch, plus "sweeps" [B]."""
    xs, us, u_per, u_scale, rconds, scalar, order = _check(xs, us, order, rcond, u_scale)
    B, E, N1, n = xs.shape
    nz = n * size_of_library(order, us.shape[3])
    prior = _check_prior(B, N1 - 1, n, nz, A0, discount, counts)
    R = rconds.shape[0]
    models = np.zeros((R, B, n, nz), dtype=np.complex128)
    rank = np.zeros((R, B), dtype=np.int32)
    svals = np.zeros((B, nz))
    status = np.zeros(B, dtype=np.int32)
    sweeps = np.zeros(B, dtype=np.int32)
    for b in range(B):
        u = us[b if u_per else 0]
        if u_scale is not None:
            u = u_scale[b] * u
        a0, d2 = None, None
        with np.errstate(all="ignore"):
            Z, Y = stack_snapshots(xs[b], u, order)
            if prior is not None:
                a0, d, steps = _member_prior(prior, b, N1 - 1)
                d2 = d * d
                Z, Y = taken_snapshots(Z, Y, E, steps)
            G, C = gram(Z, Y, d2)
        if not (np.all(np.isfinite(G)) and np.all(np.isfinite(C)) and (a0 is None or np.all(np.isfinite(a0)))):
            status[b] = 3
            continue
        if a0 is not None:
            C = gram_discrepancy(G, C, a0)
        lam, V, sweeps[b], converged = jacobi_hermitian(G)
        status[b] = 0 if converged else 1
        models[:, b], rank[:, b] = truncated_models(lam, V, C, rconds)
        if a0 is not None:
            models[:, b] += a0
        svals[b] = singular_values(V, Z, d2)
    out = _result(models, rank, svals, status, scalar)
    out["sweeps"] = sweeps
    return out


def dmdc_fit_qr_reference(xs, us, order, rcond, u_scale=None, A0=None, discount=None, counts=None):
    """The QR route's definition in NumPy, member by member (the module docstring's QR part).  Arguments and result as
    dmdc_fit_batch(method="qr"), plus "sweeps" [B]."""
    xs, us, u_per, u_scale, rconds, scalar, order = _check(xs, us, order, rcond, u_scale, "qr")
    B, E, N1, n = xs.shape
    nz = n * size_of_library(order, us.shape[3])
    prior = _check_prior(B, N1 - 1, n, nz, A0, discount, counts)
    R = rconds.shape[0]
    models = np.zeros((R, B, n, nz), dtype=np.complex128)
    rank = np.zeros((R, B), dtype=np.int32)
    svals = np.zeros((B, nz))
    status = np.zeros(B, dtype=np.int32)
    sweeps = np.zeros(B, dtype=np.int32)
    for b in range(B):
        u = us[b if u_per else 0]
        if u_scale is not None:
            u = u_scale[b] * u
        a0, d = None, None
        with np.errstate(all="ignore"):
            Z, Y = stack_snapshots(xs[b], u, order)
            if prior is not None:
                a0, d, steps = _member_prior(prior, b, N1 - 1)
                Z, Y = taken_snapshots(Z, Y, E, steps)
            Rf, T = givens_qr(Z, Y, d)
        if not (np.all(np.isfinite(Rf)) and np.all(np.isfinite(T)) and (a0 is None or np.all(np.isfinite(a0)))):
            status[b] = 3
            continue
        if a0 is not None:
            T = qr_discrepancy(Rf, T, a0)
        M, V, sweeps[b], converged = jacobi_one_sided(Rf)
        status[b] = 0 if converged else 1
        models[:, b], rank[:, b], lam = qr_models(M, V, T, rconds)
        if a0 is not None:
            models[:, b] += a0
        svals[b] = np.sqrt(np.sort(lam)[::-1])
    out = _result(models, rank, svals, status, scalar)
    out["sweeps"] = sweeps
    return out


def dmdc_fit_batch(xs, us, order, rcond, u_scale=None, method="gram", A0=None, discount=None, counts=None):
    """Fit B DMDc models on the device in one launch.

    xs [B, N + 1, n] or [B, E, N + 1, n] complex: E experiments of N steps per member; us [N, m] / [E, N, m] (shared by the
    ensemble), [B, N, m] (E = 1) or [B, E, N, m]; u_scale [B, m]: member b saw u_scale[b] * us; rcond a scalar or up to 16 values
    in [1e-7, 1).  Returns a dict: "models" [R, B, n, n (1 + P)] ([B, n, n (1 + P)] for a scalar rcond) in the layout every other
    entry point takes, "rank" [R, B] ([B]), "svals" [B, nz] (the singular values of the stacked data, descending) and "status" [B]
    (0 ok, 1 the eigen-iteration hit its cap, 3 non-finite data: zero models, rank 0).
    method "gram" (m4q_dmdc_fit_batch): from the Gram matrix of the data, error O(eps kappa^2), rcond in [1e-7, 1);
    method "qr" (m4q_dmdc_fit_qr_batch): from a QR of the data themselves, error O(eps kappa), rcond in [1e-12, 1).
    A0 [n, nz] or [B, n, nz], discount (a scalar or [B], in (0, 1]), counts [B] integers in [0, N]: the fit against a prior model
    (the module docstring's last part; m4q_dmdc_refit_batch / m4q_dmdc_refit_qr_batch): "models" are A0 + the truncated fit of
    Y - A0 Z on the snapshots t < counts[b], weighted discount^(age); "svals" and "rank" those of the weighted stack; status 3
    also for a non-finite A0.  With all three None the call is today's."""
    xs, us, u_per, u_scale, rconds, scalar, order = _check(xs, us, order, rcond, u_scale, _method(method))
    B, E, N1, n = xs.shape
    m = us.shape[3]
    nz = n * size_of_library(order, m)
    prior = _check_prior(B, N1 - 1, n, nz, A0, discount, counts)
    R = rconds.shape[0]
    models = np.empty((R, B, n, nz), dtype=np.complex128)
    rank = np.empty((R, B), dtype=np.int32)
    svals = np.empty((B, nz), dtype=np.float64)
    status = np.empty(B, dtype=np.int32)
    dp, ip = _lib._dp, _lib._ip
    L = _lib.lib()
    args = (B, n, m, order, E, N1 - 1, xs.ctypes.data_as(dp), us.ctypes.data_as(dp), u_per,
            None if u_scale is None else u_scale.ctypes.data_as(dp), rconds.ctypes.data_as(dp), R,
            models.ctypes.data_as(dp), rank.ctypes.data_as(ip), svals.ctypes.data_as(dp), status.ctypes.data_as(ip))
    if prior is None:
        entry = L.m4q_dmdc_fit_qr_batch if method == "qr" else L.m4q_dmdc_fit_batch
    else:
        entry = L.m4q_dmdc_refit_qr_batch if method == "qr" else L.m4q_dmdc_refit_batch
        args += (prior["A0"].ctypes.data_as(dp), prior["A0_per"], prior["discount"].ctypes.data_as(dp), prior["discount_per"],
                 None if prior["counts"] is None else prior["counts"].ctypes.data_as(ip))
    _lib.check(entry(*args))
    return _result(models, rank, svals, status, scalar)


def prediction_losses(xs, models, us, order, u_scale=None):
    """The reference's training loss of every (rcond, member): the spectral norm of X2 - X2_predict, the model rolled from the
    experiment's first state along its controls, summed over the experiments.  xs [B, E, N + 1, n], models [R, B, n, nz],
    us [B|1, E, N, m] -> [R, B].  One model_rollout_batch(keep="all") per rcond and experiment; the norms on the host."""
    R, B = models.shape[:2]
    E = xs.shape[1]
    losses = np.zeros((R, B))
    for r in range(R):
        for e in range(E):
            pred = model_rollout_batch(xs[:, e, 0], us[:, e] if us.shape[0] == B and B > 1 else us[0, e], models[r], order,
                                       u_scale=u_scale, keep="all")["xs"]
            diff = xs[:, e, 1:] - pred[:, 1:]
            losses[r] += np.linalg.norm(diff, 2, axis=(1, 2))
    return losses


def train_models_batch(xs, us, order, rconds=np.logspace(-6, -1, 10), u_scale=None, method="gram", A0=None):
    """The reference's hyper-parameter search (its tests/util_training.train_model) for an ensemble: one fit call covers all
    rconds, every candidate is rolled along the training controls, and each member keeps the model that loses least (the first
    of equals, as the reference's `loss < smallest_loss`).  Returns a dict: "models" [B, n, nz], "rcond" [B], "index" [B] (into
    rconds), "losses" [R, B], "status" [B].  method: dmdc_fit_batch's.  A0 [n, nz] or [B, n, nz]: every fit of the grid is made
    against this prior model (dmdc_fit_batch's A0); the selection is the same."""
    xs4, us4, _, u_scale, rconds, _, order = _check(xs, us, order, np.atleast_1d(rconds), u_scale, _method(method))
    fit = dmdc_fit_batch(xs4, us4, order, rconds, u_scale, method, A0=A0)
    losses = prediction_losses(xs4, fit["models"], us4, order, u_scale)
    finite = np.where(np.isfinite(losses), losses, np.inf)
    index = np.argmin(finite, axis=0)
    members = np.arange(xs4.shape[0])
    return {"models": np.ascontiguousarray(fit["models"][index, members]), "rcond": rconds[index], "index": index,
            "losses": losses, "status": fit["status"]}


def refit_models_batch(run, models, order, clock, rcond, discount=1.0, method="gram", layout="auto", reference=False):
    """ONE update of every member's model from its own closed-loop run: what DiscrepDMDc.from_bootstrap(A0) holds after the run's
    snapshots and one fit_iteration, A0 + (Y - A0 Z) pinv(Z, rcond) on the discounted stacks, in one call of dmdc_fit_batch with
    counts = steps_done and A0 = models.

    run: the result dict of mpc_batch (xs [B, n, n_steps + 1], us [B, m, n_steps]) or of a session's results() (time axis second),
    read as stream_models_batch reads it; models [n, nz] or [B, n, nz]: what the loops were handed; clock: the run's StepClock;
    rcond, discount, method as dmdc_fit_batch.  reference=True evaluates the NumPy definition instead.  Returns dmdc_fit_batch's
    dict.  ValueError for clock.measure_freq > 1: the unmeasured states of such a run are the model's own predictions, not data.
    The reference's matrix_rank gate (no update while the states seen span fewer than dim_x directions) is not applied: at a
    truncating rcond the update is then A0 + the fit of the discrepancy on the directions seen."""
    if int(getattr(clock, "measure_freq", 1)) > 1:
        raise ValueError("refit_models_batch needs measure_freq == 1: with measure_freq = %d the unmeasured states of the run are "
                         "predictions of the model, not data" % clock.measure_freq)
    models = np.asarray(models, dtype=np.complex128)
    if models.ndim not in (2, 3):
        raise ValueError("models must be [n, nz] or [B, n, nz], got shape %s" % (models.shape,))
    from .online import _run_arrays
    xs, us = _run_arrays(run, models.shape[-2], layout)
    counts = np.asarray(run["steps_done"])
    if models.ndim == 3 and models.shape[0] == 1 and xs.shape[0] != 1:
        models = models[0]
    if reference:
        fn = dmdc_fit_qr_reference if _method(method) == "qr" else dmdc_fit_reference
        return fn(xs, us, order, rcond, A0=models, discount=discount, counts=counts)
    return dmdc_fit_batch(xs, us, order, rcond, method=method, A0=models, discount=discount, counts=counts)
