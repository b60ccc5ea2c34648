"""The map of the rollout's pair form (csrc/m4q_rollout_pair.h), compiled for the CPU and replayed trip by trip the way
rollout_forward_pair (csrc/m4q_mpc.h) walks it, for T = 1 .. 9 and T = 40, for rows that shift their solution into the next
step's guess and rows that do not.

A row is two halves of eight lanes; trip p rolls index 2 p in the lower half and 2 p + 1 in the upper.  The expectations are
written here from the invariant and from rollout_forward's stores, not from the header's code:
  * the guess operands of index t (u_g, the node, ubar, the affine gain entries) are loaded exactly once into half t % 2, the
    gain row K_t exactly once into half 1 - t % 2, where x_t lives, each one trip ahead of its use or before the first trip;
  * every x_{t+1} and u_t is stored exactly once where rollout_forward leaves it: node t + 1 and slot t, or - shifting - node t
    and slot t - 1 (u_0 has no slot) with the last column repeated at node T and slot T - 1; x_0 at node 0 of a row that does
    not shift;
  * nothing is stored for the upper half's index T of an odd horizon;
  * every load index lies in [0, T - 1], so the node elements read lie in [0, 8 T - 1] of the (T + 1) 8."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HORIZONS = tuple(range(1, 10)) + (40,)

_DRIVER = r'''
#include <cstdio>
#include "m4q_rollout_pair.h"
namespace rp = m4q::rollout_pair;
// argv: T shift.  The walk of rollout_forward_pair, both halves:
//   F p half tl tk        a fetch of trip p's operands: own-index loads from tl, the gain row from tk
//   C p half t src        the chain of index t runs in trip p: operands in `half`, DPP source lanes from src
//   X half t node         x_{t+1} stored at `node`;   U half t slot: u_t stored at `slot`;   Z half: x_0 stored at node 0
static void fetch(int T, int p) {
  for (int h = 0; h < 2; ++h) std::printf("F %d %d %d %d\n", p, h, rp::load_index(T, p, h), rp::gain_index(T, p, h));
}
static void store(int T, bool shift, bool first, int p, bool live_lower, bool live_upper) {
  for (int h = 0; h < 2; ++h) {
    const int t = rp::own_index(p, h);
    if (!(h ? live_upper : live_lower)) continue;
    std::printf("X %d %d %d\n", h, t, rp::node_slot(t, shift));
    bool uok = true;
    if (first) uok = rp::ctrl_stored(t, shift);
    if (uok) std::printf("U %d %d %d\n", h, t, rp::ctrl_slot(t, shift));
  }
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  int T = 0, sh = 0;
  if (std::sscanf(argv[1], "%d", &T) != 1 || std::sscanf(argv[2], "%d", &sh) != 1) return 3;
  const bool shift = sh != 0;
  std::printf("G %d %d %d %d\n", rp::HALF, rp::full_pairs(T), rp::odd_tail(T) ? 1 : 0, rp::trips(T));
  for (int jj = 0; jj < 16; ++jj) std::printf("L %d %d %d\n", jj, rp::half_of_lane(jj), rp::coord_of_lane(jj));
  for (int h = 0; h < 2; ++h)
    if (rp::stores_x0(h, shift)) std::printf("Z %d\n", h);
  fetch(T, 0);
  const int nf = rp::full_pairs(T);
  for (int p = 0; p < nf; ++p) {
    fetch(T, p + 1);
    for (int h = 0; h < 2; ++h) std::printf("C %d %d %d %d\n", p, h, rp::own_index(p, h), rp::first_source_lane(rp::own_index(p, h)));
    store(T, shift, p == 0, p, true, true);
  }
  if (rp::odd_tail(T)) {
    std::printf("C %d 0 %d %d\n", nf, rp::own_index(nf, 0), rp::first_source_lane(rp::own_index(nf, 0)));
    store(T, shift, nf == 0, nf, rp::index_live(T, rp::own_index(nf, 0)), rp::index_live(T, rp::own_index(nf, 1)));
  }
  for (int h = 0; h < 2; ++h)
    if (rp::repeats(T, T - 1, shift) && h == rp::owner_half(T - 1))
      std::printf("R %d %d %d %d\n", h, T - 1, rp::repeat_node_slot(T), rp::repeat_ctrl_slot(T));
  return 0;
}
'''


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    """The header compiled with the plain host compiler; returns (T, shift) -> the walk's records by kind."""
    tmp = tmp_path_factory.mktemp("rpair")
    (tmp / "driver.cpp").write_text(_DRIVER)
    exe = str(tmp / "rpair_host")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "mpc4quantum_amd", "csrc"), str(tmp / "driver.cpp"),
                    "-o", exe], check=True)
    out = {}
    for T in HORIZONS:
        for shift in (0, 1):
            rec = {k: [] for k in "GLZFCXUR"}
            for ln in subprocess.run([exe, str(T), str(shift)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines():
                f = ln.split()
                rec[f[0]].append(tuple(int(v) for v in f[1:]))
            out[T, shift] = rec
    return out


CASES = [(T, s) for T in HORIZONS for s in (0, 1)]


def test_lane_map(walks):
    rec = walks[1, 0]
    assert rec["G"][0][0] == 8
    assert rec["L"] == [(jj, jj // 8, jj % 8) for jj in range(16)]


@pytest.mark.parametrize("T,shift", CASES)
def test_trips(T, shift, walks):
    half, nf, odd, trips = walks[T, shift]["G"][0]
    assert (nf, odd, trips) == (T // 2, T % 2, (T + 1) // 2)
    # every index runs exactly once, in order, its operands in half t % 2 and its state - the DPP source lanes - in the other
    chains = walks[T, shift]["C"]
    assert [c[2] for c in chains] == list(range(T))
    for p, h, t, src in chains:
        assert (p, h) == (t // 2, t % 2) and src == 8 * (1 - t % 2)


@pytest.mark.parametrize("T,shift", CASES)
def test_loads(T, shift, walks):
    rec = walks[T, shift]
    fetched = {}
    for p, h, tl, tk in rec["F"]:
        assert 0 <= tl <= T - 1 and 0 <= tk <= T - 1, (p, h, tl, tk)
        assert 0 <= 8 * tl and 8 * tl + 7 <= 8 * (T + 1) - 1
        assert (p, h) not in fetched, "trip %d fetched twice" % p
        fetched[p, h] = (tl, tk)
    # a trip's operands are there before it starts: fetched before the first trip or during the one before
    order = [p for p, h, _, _ in rec["F"] if h == 0]
    assert order == list(range(len(order))) and len(order) >= (T + 1) // 2
    own, rows = {}, {}
    for p, h, t, _src in rec["C"]:
        # the chain of index t takes its guess operands from half t % 2 and the gain row from the half that holds x_t
        tl, _ = fetched[p, t % 2]
        _, tk = fetched[p, 1 - t % 2]
        own.setdefault(tl, []).append((p, t % 2))
        rows.setdefault(tk, []).append((p, 1 - t % 2))
        assert tl == t and tk == t
    assert sorted(own) == list(range(T)) and all(len(v) == 1 for v in own.values())
    assert sorted(rows) == list(range(T)) and all(len(v) == 1 for v in rows.values())


def _today(T, shift):
    """What rollout_forward leaves in the destination arrays: {("x", node): t + 1 of x_{t+1} (0: x_0), ("u", slot): t}."""
    mem = {}
    if not shift:
        mem["x", 0] = 0
    for t in range(T):
        mem["x", t + (0 if shift else 1)] = t + 1
        mem["u", max(t - 1, 0) if shift else t] = t
        if shift and t == T - 1:
            mem["x", T] = t + 1
            mem["u", T - 1] = t
    return mem


@pytest.mark.parametrize("T,shift", CASES)
def test_stores(T, shift, walks):
    rec = walks[T, shift]
    mem = {}

    def put(key, val):
        assert key not in mem, "%s stored twice" % (key,)
        mem[key] = val
    for (h,) in rec["Z"]:
        assert h == 0
        put(("x", 0), 0)
    stored_x, stored_u = [], []
    for h, t, node in rec["X"]:
        assert h == t % 2 and t < T, "index %d stored by half %d" % (t, h)
        put(("x", node), t + 1)
        stored_x.append(t)
    for h, t, slot in rec["U"]:
        assert h == t % 2 and t < T and slot >= 0
        put(("u", slot), t)
        stored_u.append(t)
    for h, t, node, slot in rec["R"]:
        assert shift and t == T - 1 and h == t % 2
        put(("x", node), t + 1)
        put(("u", slot), t)
    assert len(rec["R"]) == (1 if shift else 0)
    assert sorted(stored_x) == list(range(T))
    assert sorted(stored_u) == [t for t in range(T) if not shift or t >= 1]
    assert mem == _today(T, bool(shift))
    assert all(0 <= node <= T for kind, node in mem if kind == "x") and all(0 <= s <= T - 1 for kind, s in mem if kind == "u")
