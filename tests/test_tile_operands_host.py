"""The LDS operand image of the clipped tile sweep (csrc/m4q_tile_opnd.h), compiled for the CPU: every write and every read of
every lane replayed on the map's own address functions, for the three tile shapes (n, m) = (3, 1), (3, 2), (8, 2) and for m = 3.

Lane = 16 r + 4 mb + q writes its double of a tile (column q = time tb - q); the expectations are written here from the sweep's
layout (m4q_tile.h), not from the header's code:
  * the W read of lane (r, mb, q) for index j returns element (r, mb, j) of tile q of [BT[0][K] .. BT[m - 1][K], CT[K], zero ..];
  * the broadcast reads return element (r, mb, j) of their tile in all four q;
  * no read has two distinct addresses on one bank within a 32-lane half (ds_read_b64: banks (a / 4) mod 64 and the next);
  * every address lies inside bytes(), tiles do not overlap, and the image leaves the workgroups of the three shapes at or under
    an eighth of a CU's 160 KB, given what they used before it (session.info() of the library before it: 3,504, 3,832 and 11,880 B;
    m4q_kernels.hip asserts the same on the sum it really allocates)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

SHAPES = ((1, 1), (2, 1), (2, 2), (3, 4))          # (m, tiles per side): n = 3 with m = 1, 2; n = 8; n = 15 or 16 with m = 3
WORKGROUP_BEFORE = {(1, 1): 3504, (2, 1): 3832, (2, 2): 11880}
WORKGROUP_LIMIT = 20480

_DRIVER = r'''
#include <cstdio>
#include "m4q_tile_opnd.h"
namespace o = m4q::tile_opnd;
// argv: nu nt.  Prints: PITCH bytes tiles; then one line per access: kind tile K j lane address
//   kind 0: write of `tile`; 1: W read of group K, index j; 2: broadcast read of `tile`, index j
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  int nu = 0, nt = 0;
  if (std::sscanf(argv[1], "%d", &nu) != 1 || std::sscanf(argv[2], "%d", &nt) != 1) return 3;
  std::printf("%d %d %d\n", o::PITCH, o::bytes(nu, nt), o::tiles(nu, nt));
  for (int K = 0; K < nt; ++K) {
    for (int s = 0; s < nu; ++s) std::printf("N b %d %d %d\n", s, K, o::tile_b(nu, s, K));
    std::printf("N c 0 %d %d\n", K, o::tile_c(nu, K));
    std::printf("N z 0 %d %d\n", K, o::tile_zero(nu, K));
  }
  for (int p = 0; p < nu; ++p) std::printf("N u %d 0 %d\n", p, o::tile_u(nu, nt, p));
  for (int lane = 0; lane < 64; ++lane) {
    for (int t = 0; t < o::tiles(nu, nt); ++t) std::printf("A 0 %d 0 0 %d %d\n", t, lane, o::write_addr(lane) + o::write_imm(t));
    for (int K = 0; K < nt; ++K)
      for (int j = 0; j < 4; ++j) std::printf("A 1 0 %d %d %d %d\n", K, j, lane, o::w_addr(nu, lane) + o::w_imm(nu, K, j));
    for (int t = 0; t < o::tiles(nu, nt); ++t)
      for (int j = 0; j < 4; ++j) std::printf("A 2 %d 0 %d %d %d\n", t, j, lane, o::bcast_addr(lane) + o::bcast_imm(t, j));
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """The header compiled with the plain host compiler (no HIP include path); returns shape -> parsed accesses."""
    tmp = tmp_path_factory.mktemp("opnd")
    (tmp / "driver.cpp").write_text(_DRIVER)
    exe = str(tmp / "opnd_host")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "mpc4quantum_amd", "csrc"), str(tmp / "driver.cpp"),
                    "-o", exe], check=True)
    out = {}
    for nu, nt in SHAPES:
        lines = subprocess.run([exe, str(nu), str(nt)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
        pitch, nbytes, ntiles = (int(v) for v in lines[0].split())
        names, acc = {}, []
        for ln in lines[1:]:
            f = ln.split()
            if f[0] == "N":
                names[f[1], int(f[2]), int(f[3])] = int(f[4])
            else:
                acc.append(tuple(int(v) for v in f[1:]))
        out[nu, nt] = {"pitch": pitch, "bytes": nbytes, "tiles": ntiles, "names": names, "acc": np.array(acc)}
    return out


def _geo(lane):
    return lane >> 4, (lane >> 2) & 3, lane & 3          # r, mb, q (m4q_tile.h)


def _memory(lay):
    """address -> (tile, r, mb, q) from the writes; no two writes share a byte."""
    mem = {}
    for kind, tile, _, _, lane, a in lay["acc"]:
        if kind == 0:
            assert a % 8 == 0 and 0 <= a and a + 8 <= lay["bytes"], (tile, lane, a)
            assert a not in mem, "tiles overlap at byte %d" % a
            mem[a] = (tile,) + _geo(lane)
    assert len(mem) == 64 * lay["tiles"]
    return mem


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_order(shape, layout):
    nu, nt = shape
    lay = layout[shape]
    assert lay["pitch"] == 520
    want = []
    for K in range(nt):
        want += [("b", s, K) for s in range(nu)] + [("c", 0, K), ("z", 0, K)]
    want += [("u", p, 0) for p in range(nu)]
    assert [lay["names"][w] for w in want] == list(range(len(want))) and lay["tiles"] == len(want)


@pytest.mark.parametrize("shape", SHAPES)
def test_w_read_returns_column_j_of_tile_q(shape, layout):
    nu, nt = shape
    lay = layout[shape]
    mem = _memory(lay)
    seen = 0
    for kind, _, K, j, lane, a in lay["acc"]:
        if kind != 1:
            continue
        r, mb, q = _geo(lane)
        tile = lay["names"]["b", q, K] if q < nu else lay["names"]["c" if q == nu else "z", 0, K]
        assert mem[a] == (tile, r, mb, j), (K, j, lane, a)
        seen += 1
    assert seen == 64 * 4 * nt


@pytest.mark.parametrize("shape", SHAPES)
def test_broadcast_read_returns_element_r_mb_j(shape, layout):
    lay = layout[shape]
    mem = _memory(lay)
    seen = 0
    for kind, tile, _, j, lane, a in lay["acc"]:
        if kind != 2:
            continue
        r, mb, _q = _geo(lane)
        assert mem[a] == (tile, r, mb, j), (tile, j, lane, a)
        seen += 1
    assert seen == 64 * 4 * lay["tiles"]


@pytest.mark.parametrize("shape", SHAPES)
def test_no_read_has_a_bank_conflict(shape, layout):
    """A ds_read_b64 is served in two halves of 32 lanes; a lane takes banks (a / 4) mod 64 and the next one.  Lanes with the
    same address share one access (a broadcast); two DIFFERENT addresses on one bank serialise."""
    lay = layout[shape]
    acc = lay["acc"]
    reads = acc[acc[:, 0] != 0]
    checked = 0
    for key in {tuple(k) for k in reads[:, :4]}:
        rows = reads[(reads[:, :4] == key).all(axis=1)]
        assert len(rows) == 64
        for half in (0, 1):
            owner = {}
            for lane, a in rows[(rows[:, 4] >> 5) == half][:, 4:]:
                for bank in ((a // 4) % 64, (a // 4 + 1) % 64):
                    assert owner.setdefault(bank, a) == a, "read %s: addresses %d and %d on bank %d" % (key, owner[bank], a, bank)
            checked += 1
    assert checked == 2 * 4 * (shape[1] + lay["tiles"])


@pytest.mark.parametrize("shape", SHAPES)
def test_reads_stay_inside_the_image(shape, layout):
    lay = layout[shape]
    a = lay["acc"][:, 5]
    assert a.min() >= 0 and a.max() + 8 <= lay["bytes"] and (a % 8 == 0).all()
    assert lay["bytes"] == lay["tiles"] * lay["pitch"]


@pytest.mark.parametrize("shape", sorted(WORKGROUP_BEFORE))
def test_workgroup_keeps_eight_per_cu(shape, layout):
    assert WORKGROUP_BEFORE[shape] + layout[shape]["bytes"] <= WORKGROUP_LIMIT
