"""Batched recursive DMDc updates: trajectories and controls of B members in, their streaming models out, in ONE launch
(m4q_online_dmdc_batch) - `OnlineDMDc.fit_iteration` (model.py: recursive least squares with a forgetting factor) fed with every
snapshot of an ensemble, which is what `mpc(..., streaming=True)` does to the model of one closed loop.

This module is the normative definition of what the kernel computes (csrc/m4q_online.h reproduces it, in the same order of
operations), as fit.py is for the fit.  Per member, with E experiments of N steps (xs [E, N + 1, n] complex, u [E, N, m] real,
optional u_scale [m]: the member sees u_scale[k] u[t][k], one fp64 product):

  snapshots   exactly fit.stack_snapshots: z = [x_t ; lift(u_t) (x) x_t], y = x_{t+1} for every (e, t), e outer, t inner,
              nz = n (1 + P); with counts, only t < count of every experiment.
  state       A [n, nz] and P [nz, nz] complex, from A0 and P0 (or P0 = alpha I).
  one update  every sum runs over its index in ASCENDING order, from zero (r: from y_i, subtracting term by term):
                Pz_i = sum_j P[i][j] z_j
                w_j  = Pz_j                                   (hermitian: w_j = sum_i conj(z_i) P[i][j])
                s    = sum_j w_j z_j                          (= z^T P z, unconjugated; hermitian: z^H P z)
                gamma = 1 / (1 + s) = conj(d) / |d|^2 with d = 1 + s: (Re d / (Re d^2 + Im d^2), -Im d / (Re d^2 + Im d^2))
                r_i  = y_i - sum_j A[i][j] z_j;  the innovation of the snapshot is sum_i |r_i|^2, BEFORE the update
                A[i][j] = A[i][j] + (gamma r_i) w_j
                P[i][j] = (P[i][j] - (gamma Pz_i) w_j) * (1 / discount)
              `/ discount` is a PRODUCT with the reciprocal 1 / discount, formed once per member (what numpy's complex division by
              a real number does, too).

This is OnlineDMDc.fit_iteration as model.py writes it: gamma (y - A z) Pz^T and (P - gamma Pz Pz^T) / discount, the plain
transposes on complex data kept.  hermitian=True is the conjugated recursion, an extension in the spirit of the "hermitian" noise
kind: its P is the inverse of the Gram matrix sum z z^H that dmdc_fit_batch accumulates (plus the discounted prior), and with
discount = 1, A0 = 0 and a large alpha it tends to the least-squares fit.

With M = P^-1 and T = A M one update is M <- discount (M + z z^T) and T <- discount (T + y z^T) (z z^H, y z^H when hermitian),
so after K updates M = discount^K P0^-1 + sum_k discount^(K - k + 1) z_k z_k^T and T likewise from A0 P0^-1: the closed form the
tests hold the recursion to.

hist_every = k > 0: "hist" holds A after updates k, 2k, ... (the reference's iA); E N // k records, those a member with a smaller
count never reaches are zero.  "innov" [E N] at e N + t, zero beyond the count.
status per member: 0 ok; 3 if a snapshot taken, the final A or the final P holds a non-finite entry: A, P and hist are zero
(the innovations are left as computed)."""
import numpy as np

from . import _lib, fit
from .library import size_of_library


def _check(xs, us, order, A0, P0, alpha, discount, u_scale, counts, hist_every):
    """Shapes and values of an online call, before the library is touched.  Returns a dict of contiguous arrays and flags."""
    xs, us, u_per, u_scale, _, _, order = fit._check(xs, us, order, fit.RCOND_MIN, u_scale)
    B, E, N1, n = xs.shape
    N = N1 - 1
    nz = n * size_of_library(order, us.shape[3])
    def per(a):                                 # [B, ...] and not [...] (which was reshaped to [1, ...])
        return a.shape[0] == B and B > 1
    A0 = np.ascontiguousarray(A0, dtype=np.complex128)
    if A0.shape not in ((n, nz), (B, n, nz)):
        raise ValueError("A0 must be [n, nz] = (%d, %d) or [B, n, nz] with B = %d, got %s" % (n, nz, B, A0.shape))
    if P0 is not None:
        if alpha is not None:
            raise ValueError("give P0 or alpha, not both")
        P0 = np.ascontiguousarray(P0, dtype=np.complex128)
        if P0.shape not in ((nz, nz), (B, nz, nz)):
            raise ValueError("P0 must be [nz, nz] = (%d, %d) or [B, nz, nz] with B = %d, got %s" % (nz, nz, B, P0.shape))
        alpha = 0.0
    else:
        if alpha is None or not (np.ndim(alpha) == 0 and np.isfinite(alpha) and alpha > 0):
            raise ValueError("without P0, alpha must be a positive number (P0 = alpha I), got %r" % (alpha,))
        alpha = float(alpha)
    discount = np.asarray(discount, dtype=np.float64)
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
    if isinstance(hist_every, bool) or int(hist_every) != hist_every or hist_every < 0:
        raise ValueError("hist_every must be a non-negative integer, got %r" % (hist_every,))
    A0 = A0.reshape((-1, n, nz))
    if P0 is not None:
        P0 = P0.reshape((-1, nz, nz))
    return dict(xs=xs, us=us, u_per=u_per, u_scale=u_scale, order=order, B=B, E=E, N=N, n=n, m=us.shape[3], nz=nz, A0=A0,
                A0_per=int(per(A0)), P0=P0, P0_per=int(P0 is not None and per(P0)), alpha=alpha,
                discount=np.ascontiguousarray(discount.reshape(-1)), discount_per=int(discount.ndim == 1), counts=counts, hist_every=int(hist_every))


def _result(models, P, hist, innov, status):
    out = {"models": models, "P": P, "hist": hist, "status": status}
    if innov is not None:
        out["innov"] = innov
    return out


def update(A, P, z, y, inv_discount, hermitian):
    """One update of the module docstring, in place; returns the innovation sum_i |r_i|^2 of the snapshot."""
    n, nz = A.shape
    Pz = np.zeros(nz, dtype=np.complex128)
    r = y.astype(np.complex128)
    for j in range(nz):
        Pz += P[:, j] * z[j]
        r -= A[:, j] * z[j]
    if hermitian:
        w = np.zeros(nz, dtype=np.complex128)
        for i in range(nz):
            w += z[i].conjugate() * P[i, :]
    else:
        w = Pz
    s = 0j
    for j in range(nz):
        s += w[j] * z[j]
    d = 1.0 + s
    den = d.real * d.real + d.imag * d.imag
    gamma = complex(d.real / den, -d.imag / den)
    innov = 0.0
    for i in range(n):
        innov += r[i].real * r[i].real + r[i].imag * r[i].imag
    A += np.outer(gamma * r, w)
    P[:] = (P - np.outer(gamma * Pz, w)) * inv_discount
    return innov


def online_dmdc_reference(xs, us, order, A0, P0=None, alpha=None, discount=1.0, u_scale=None, counts=None, hermitian=False,
                          hist_every=0, innovations=False):
    """The definition above in NumPy, member by member.  Arguments and result as online_dmdc_batch."""
    c = _check(xs, us, order, A0, P0, alpha, discount, u_scale, counts, hist_every)
    B, E, N, n, nz, k = c["B"], c["E"], c["N"], c["n"], c["nz"], c["hist_every"]
    H = (E * N) // k if k else 0
    models = np.zeros((B, n, nz), dtype=np.complex128)
    Ps = np.zeros((B, nz, nz), dtype=np.complex128)
    hist = np.zeros((H, B, n, nz), dtype=np.complex128)
    innov = np.zeros((B, E * N)) if innovations else None
    status = np.zeros(B, dtype=np.int32)
    for b in range(B):
        u = c["us"][b if c["u_per"] else 0]
        if c["u_scale"] is not None:
            u = c["u_scale"][b] * u
        steps = N if c["counts"] is None else int(c["counts"][b])
        A = c["A0"][b if c["A0_per"] else 0].copy()
        P = c["P0"][b if c["P0_per"] else 0].copy() if c["P0"] is not None else c["alpha"] * np.identity(nz, dtype=np.complex128)
        inv_discount = 1.0 / float(c["discount"][b if c["discount_per"] else 0])
        done = 0
        with np.errstate(all="ignore"):
            Z, Y = fit.stack_snapshots(c["xs"][b], u, c["order"])
            Z, Y = Z.T.reshape(E, N, nz), Y.T.reshape(E, N, n)
            finite = True
            for e in range(E):
                for t in range(steps):
                    finite = finite and bool(np.all(np.isfinite(Z[e, t])) and np.all(np.isfinite(Y[e, t])))
                    v = update(A, P, Z[e, t], Y[e, t], inv_discount, hermitian)
                    if innovations:
                        innov[b, e * N + t] = v
                    done += 1
                    if k and done % k == 0:
                        hist[done // k - 1, b] = A
        if not (finite and np.all(np.isfinite(A)) and np.all(np.isfinite(P))):
            status[b] = 3
            hist[:, b] = 0.0
            continue
        models[b], Ps[b] = A, P
    return _result(models, Ps, hist, innov, status)


def online_dmdc_batch(xs, us, order, A0, P0=None, alpha=None, discount=1.0, u_scale=None, counts=None, hermitian=False,
                      hist_every=0, innovations=False):
    """Update B DMDc models recursively on the device in one launch: OnlineDMDc.fit_iteration for every snapshot of every member.

    xs [B, N + 1, n] or [B, E, N + 1, n] complex and us, u_scale as dmdc_fit_batch takes them; counts [B] integers: member b uses
    only t < counts[b] of each experiment; A0 [n, nz] or [B, n, nz]; P0 [nz, nz] / [B, nz, nz], or alpha > 0 for P0 = alpha I;
    discount a scalar or [B], in (0, 1]; hermitian: the conjugated recursion (module docstring); hist_every = k > 0: also A after
    updates k, 2k, ...; innovations: also sum |y - A z|^2 of every snapshot before its update.
    Returns a dict: "models" [B, n, nz] in the layout sessions and rollouts take, "P" [B, nz, nz], "hist" [E N // k, B, n, nz]
    ([0, B, n, nz] for k = 0), "innov" [B, E N] (when asked for; zero beyond counts) and "status" [B] (0 ok, 3 non-finite data or
    state: zero A, P and hist)."""
    c = _check(xs, us, order, A0, P0, alpha, discount, u_scale, counts, hist_every)
    B, E, N, n, nz, k = c["B"], c["E"], c["N"], c["n"], c["nz"], c["hist_every"]
    H = (E * N) // k if k else 0
    models = np.empty((B, n, nz), dtype=np.complex128)
    Ps = np.empty((B, nz, nz), dtype=np.complex128)
    hist = np.empty((H, B, n, nz), dtype=np.complex128)
    innov = np.empty((B, E * N), dtype=np.float64) if innovations else None
    status = np.empty(B, dtype=np.int32)
    dp, ip = _lib._dp, _lib._ip

    def ptr(a, kind=dp):
        return None if a is None or a.size == 0 else a.ctypes.data_as(kind)
    L = _lib.lib()
    _lib.check(L.m4q_online_dmdc_batch(B, n, c["m"], c["order"], E, N, ptr(c["xs"]), ptr(c["us"]), c["u_per"], ptr(c["u_scale"]),
                                       ptr(c["counts"], ip), ptr(c["A0"]), c["A0_per"], ptr(c["P0"]), c["P0_per"], c["alpha"],
                                       ptr(c["discount"]), c["discount_per"], _lib.ONLINE_HERMITIAN if hermitian else 0, k,
                                       ptr(models), ptr(Ps), ptr(hist), ptr(innov), ptr(status, ip)))
    return _result(models, Ps, hist, innov, status)


def _run_arrays(run, n, layout):
    """xs [B, ns + 1, n], us [B, ns, m] from a result dict: mpc_batch returns the time axis last, a session's results() second."""
    xs, us = np.asarray(run["xs"]), np.asarray(run["us"])
    if xs.ndim != 3 or us.ndim != 3 or xs.shape[0] != us.shape[0]:
        raise ValueError("run['xs'] and run['us'] must be 3-D with one leading ensemble axis, got %s and %s" % (xs.shape, us.shape))
    if layout == "auto":
        last = xs.shape[1] == n and xs.shape[2] == us.shape[2] + 1
        second = xs.shape[2] == n and xs.shape[1] == us.shape[1] + 1
        if last == second:
            raise ValueError("cannot tell the time axis of xs %s / us %s for n = %d: pass layout='time_last' (mpc_batch) or "
                             "'time_second' (EnsembleSession.results)" % (xs.shape, us.shape, n))
        layout = "time_last" if last else "time_second"
    if layout == "time_last":
        xs, us = np.swapaxes(xs, 1, 2), np.swapaxes(us, 1, 2)
    elif layout != "time_second":
        raise ValueError("layout is 'auto', 'time_last' or 'time_second', got %r" % (layout,))
    if xs.shape[2] != n or xs.shape[1] != us.shape[1] + 1:
        raise ValueError("the run's xs %s and us %s do not fit models of n = %d" % (xs.shape, us.shape, n))
    return np.ascontiguousarray(xs), np.ascontiguousarray(us)


def stream_models_batch(run, models, order, clock, alpha=None, P0=None, discount=1.0, hermitian=False, hist_every=0,
                        innovations=False, layout="auto", reference=False):
    """`streaming=True` for an ensemble: the models an OnlineDMDc per member would hold after the closed loops of `run`, in one
    call of online_dmdc_batch with counts = steps_done.

    run: the result dict of mpc_batch (xs [B, n, n_steps + 1], us [B, m, n_steps]) or of a session's results() (time axis second);
    models [n, nz] or [B, n, nz]: what the loops were handed (the A0 of every member); clock: the run's StepClock; alpha / P0,
    discount, hermitian, hist_every, innovations as online_dmdc_batch.  reference=True evaluates the NumPy definition instead.
    The loop linearises the model it was handed at entry (mpc.py:156), so at measure_freq == 1 the refit never feeds back into the
    controls and the streaming model is a function of the stored run alone.  ValueError for clock.measure_freq > 1: there the
    reference predicts the unmeasured states with the refitted model (mpc.py:267), the run itself would depend on the refit.
    One difference to the reference: when an exit condition stops a loop (exit code 1) the reference has already fed the step it
    then drops; this helper uses the steps the run kept (steps_done)."""
    if int(getattr(clock, "measure_freq", 1)) > 1:
        raise ValueError("stream_models_batch needs measure_freq == 1: with measure_freq = %d the unmeasured states are predicted "
                         "by the refitted model (mpc.py:267), the run depends on the refit" % clock.measure_freq)
    models = np.asarray(models, dtype=np.complex128)
    if models.ndim not in (2, 3):
        raise ValueError("models must be [n, nz] or [B, n, nz], got shape %s" % (models.shape,))
    xs, us = _run_arrays(run, models.shape[-2], layout)
    counts = np.asarray(run["steps_done"])
    fn = online_dmdc_reference if reference else online_dmdc_batch
    return fn(xs, us, order, models[0] if models.ndim == 3 and models.shape[0] == 1 and xs.shape[0] != 1 else models, P0=P0,
              alpha=alpha, discount=discount, counts=counts, hermitian=hermitian, hist_every=hist_every, innovations=innovations)
