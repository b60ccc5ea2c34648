"""Generate tests/golden/dmdc_refit.npz: what ONE update of the REFERENCE's DiscrepDMDc against a prior model gives for the
training data of tests/golden/dmdc_fit.npz.

Run once where the reference checkout exists (it is loaded by file path, as make_golden_dmdc_fit.py loads it; CPU only):
    python tests/golden/make_golden_dmdc_refit.py
The cases are a-e of dmdc_fit.npz, their shapes and - for b to e - their xs / us, read from that file and not stored again.  Case a
of dmdc_fit.npz is a resonantly driven qubit whose states span three of the four directions, so the reference's rank gate
(matrix_rank(X) >= dim_x) never opens and its update is A0 itself: here case a is the same shape and recipe off resonance, and the
file holds its xs / us.  Per case:
  A0        [B, n, nz]: the reference's plain fit (dmdc_fit.npz: A at its lowest cut-off) of the NEXT member of the case (for case
            a: DiscrepDMDc.from_data of the next member, rcond 1e-3): as far from the member's own as the two plants differ;
  discount  0.9 for cases b and c, 1 elsewhere; counts [B]: ragged for case c, N elsewhere;
  A         [R, B, n, nz]: DiscrepDMDc(n, n, nz - n, A0, Y=, X=, U=, discount=, rcond=) whose stacks hold all but the last snapshot
            the member takes, weighted discount^(S-2-s), after ONE fit_iteration with the last snapshot: the stacks then carry
            the weights discount^(S-1-s);
  svals, rank of the weighted stack Z w, sens (how far the reference's own A moves under a relative 1e-15 jitter of the data), and
  rconds chosen from the training grid by make_golden_dmdc_fit.py's margin rule on the WEIGHTED singular values.
Asserted: the rank gate opened for every member; every cut-off is a factor 1.2 clear of every singular value; in every case a
cut-off truncates, and wherever one does the update differs from the plain fit Y pinv(Z w, rcond) of the same data by more than
1e-3, so that a test that ignored the prior would fail."""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden_dmdc_fit as base  # noqa: E402

DISCOUNT = {"a": 1.0, "b": 0.9, "c": 0.9, "d": 1.0, "e": 1.0}
COUNTS = {"c": [20, 12, 16]}


def member_stacks(ref, xs_b, u_b, order, count, discount):
    """(X2, X1, UX1, w) of the snapshots t < count of every experiment, in the (e, t) order, and their weights."""
    X2, X1, UX1 = base.stacked(ref, xs_b[:, :count + 1], u_b[:, :count], order)
    S = X1.shape[1]
    return X2, X1, UX1, discount ** np.arange(S - 1, -1, -1.0)


def one_update(Model, A0, X2, X1, UX1, w, discount, rcond):
    """The reference's update: the stacks without the last snapshot, one fit_iteration with it.  Returns (A, gate open)."""
    n, nu = X1.shape[0], UX1.shape[0]
    pre = w[:-1] / discount                                   # discount^(S-2-s): the iteration multiplies the stacks by discount
    mdl = Model(n, n, nu, A0.copy(), Y=X2[:, :-1] * pre, X=X1[:, :-1] * pre, U=UX1[:, :-1] * pre, discount=discount, rcond=rcond)
    mdl.fit_iteration(X2[:, -1], X1[:, -1], UX1[:, -1])
    return mdl.A, np.linalg.matrix_rank(mdl.X) >= mdl.min_rank


def record(ref, name, case, A0, discount, counts, rng, store_data):
    xs, us, order = case["xs"], case["us"], case["order"]
    u_scale = case.get("u_scale")
    B, n = xs.shape[0], xs.shape[-1]
    Model = ref["model"].DiscrepDMDc
    data, svals = [], []
    for b in range(B):
        u_b = us[b] if us.ndim == 4 else us
        if u_scale is not None:
            u_b = u_scale[b] * u_b
        X2, X1, UX1, w = member_stacks(ref, xs[b], u_b, order, int(counts[b]), discount)
        data.append((X2, X1, UX1, w))
        svals.append(np.linalg.svd(np.vstack([X1, UX1]) * w, compute_uv=False))
    svals = np.stack(svals)
    nz = data[0][1].shape[0] + data[0][2].shape[0]
    assert svals.shape[1] == nz, "fewer snapshots than rows"
    rconds, rank = base.choose_rconds(svals)
    for rc in rconds:
        ratio = svals / (rc * svals[:, :1])
        assert np.all((ratio >= base.MARGIN) | (ratio <= 1 / base.MARGIN))
    assert (rank < nz).any(), "%s: no admissible cut-off truncates (ranks %s)" % (name, np.unique(rank))
    A = np.zeros((len(rconds), B, n, nz), dtype=complex)
    sens = np.zeros((len(rconds), B))
    apart = np.zeros((len(rconds), B))
    for b, (X2, X1, UX1, w) in enumerate(data):
        def jitter(M):
            return M * (1 + 1e-15 * rng.standard_normal(M.shape))
        pert = (jitter(X2), jitter(X1), jitter(UX1))
        Z = np.vstack([X1, UX1])
        for r, rc in enumerate(rconds):
            A[r, b], gate = one_update(Model, A0[b], X2, X1, UX1, w, discount, rc)
            assert gate, "%s member %d: the reference's rank gate stayed shut, its A is A0" % (name, b)
            assert np.linalg.matrix_rank(Z * w, tol=rc * svals[b, 0]) == rank[r, b]
            sens[r, b] = np.abs(one_update(Model, A0[b], *pert, w, discount, rc)[0] - A[r, b]).max()
            apart[r, b] = np.abs(A[r, b] - (X2 * w) @ np.linalg.pinv(Z * w, rcond=rc)).max()
    assert np.all(apart[rank < nz] > 1e-3), "%s: a truncated update within 1e-3 of the plain fit: %s" % (name, apart)
    out = {"A0": A0, "discount": np.float64(discount), "counts": np.asarray(counts, dtype=np.int32), "rconds": rconds, "A": A,
           "svals": svals, "rank": rank.astype(np.int32), "sens": sens}
    if store_data:
        out.update(xs=xs, us=us, order=np.int64(order))
    print("%s: n = %d, nz = %d, B = %d; discount %g, counts %s; rconds %s; ranks %s; |A - A0| up to %.3g; |A - plain fit| where "
          "truncated %.3g .. %.3g; sens up to %.3g" % (name, n, nz, B, discount, list(counts), rconds, [sorted(set(r)) for r in rank.tolist()],
                                                      np.abs(A - A0[None]).max(), apart[rank < nz].min(), apart[rank < nz].max(), sens.max()))
    return {"%s_%s" % (name, k): v for k, v in out.items()}


def main():
    ref = base.load_reference()
    g = np.load(os.path.join(OUT, "dmdc_fit.npz"))
    out = {}
    for i, name in enumerate("abcde"):
        if name == "a":                                  # off resonance (the module docstring); the first draw with a truncating cut-off
            for attempt in range(200):
                rng = np.random.default_rng([20240612, i, attempt])
                case = base.case_qubit(rng, 1, B=3, E=1, N=12, amp=0.6)
                rank = base.choose_rconds(base.spectrum(ref, case)[1])[1]
                if rank.size and (rank < 8).any():
                    break
            print("case a: draw %d" % attempt)
            data = base.spectrum(ref, case)[0]
            plain = np.stack([ref["model"].DiscrepDMDc.from_data(*d, rcond=1e-3).A for d in data])
        else:
            rng = np.random.default_rng([20240612, i])
            case = {k: g["%s_%s" % (name, k)] for k in ("xs", "us")}
            case["order"] = int(g[name + "_order"])
            if name + "_u_scale" in g.files:
                case["u_scale"] = g[name + "_u_scale"]
            plain = g[name + "_A"][0]
        B, N = case["xs"].shape[0], case["xs"].shape[2] - 1
        A0 = np.ascontiguousarray(np.roll(plain, -1, axis=0))           # member b gets the fit of member b + 1
        out.update(record(ref, name, case, A0, DISCOUNT[name], COUNTS.get(name, [N] * B), rng, store_data=name == "a"))
    path = os.path.join(OUT, "dmdc_refit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
