"""The weight table of the node-per-lane line search (csrc/m4q_ls_table.h), compiled for the CPU: the table and its reads replayed on
the header's own functions, at d = 3 (n = 9) - the shape whose tile kernels use it.

The expectations are written here from line_search_tl_nodes as it forms the weights without the table (m4q_mpc.h), not from the
header's code:
  * weight(q) = (wqf if q // 2n == T else wq)[q % 2n]; the entry of off-diagonal slot c = a d + b of node t is
    0.5 * (weight(c (T + 1) + t + off) + weight((b d + a)(T + 1) + t + off)), off = n (T + 1) where a > b, and of diagonal slot a
    weight((a d + a)(T + 1) + t): bit for bit, on weights that are all different;
  * the table takes what 20,480 B leave behind the 17,080 B the (9, 2, 1) tile workgroup used before it: 47 nodes, so T = 46 is
    tabled and T = 47 is not, and the workgroup stays at or under the limit;
  * a lane of a row reads node jj + 16 trip (past the end: node T) at a pitch of 72 B; no ds_read_b64 has two distinct addresses on
    one bank within a 32-lane half (banks (a / 4) mod 64 and the next), the four rows reading the same addresses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

NX, D = 9, 3
TABLE_HORIZONS = (1, 2, 3, 15, 16, 17, 40, 46)
WORKGROUP_BEFORE = 17080
WORKGROUP_LIMIT = 20480

_DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "m4q_ls_table.h"
namespace l = m4q::ls_table;
// argv: mode ...
//   table nx d T w0 w1 ..  -> one line "t s <entry as %a>" per entry (w: the 4 nx staged weights, hex floats)
//   cap nx used            -> "pitch capacity bytes"
//   tabled T nodes         -> "0" or "1"
//   reads nx T             -> one line "trip s lane address" per read of the nodes loop
//   slots nx d             -> "c slot" per off-diagonal c, then "a slot" per diagonal a
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  auto is = [&](const char* m) { return std::strcmp(argv[1], m) == 0; };
  if (is("table")) {
    const int nx = std::atoi(argv[2]), d = std::atoi(argv[3]), T = std::atoi(argv[4]);
    if (argc != 5 + 4 * nx) return 3;
    double* w = new double[4 * nx];
    for (int i = 0; i < 4 * nx; ++i) w[i] = std::strtod(argv[5 + i], nullptr);
    for (int t = 0; t <= T; ++t)
      for (int s = 0; s < nx; ++s) std::printf("%d %d %a\n", t, s, l::entry(w, nx, d, T, t, s));
    delete[] w;
  } else if (is("cap")) {
    const int nx = std::atoi(argv[2]), used = std::atoi(argv[3]);
    std::printf("%d %d %d\n", l::pitch_bytes(nx), l::capacity(nx, used), l::bytes(nx, l::capacity(nx, used)));
  } else if (is("tabled")) {
    std::printf("%d\n", l::tabled(std::atoi(argv[2]), std::atoi(argv[3])) ? 1 : 0);
  } else if (is("reads")) {
    const int nx = std::atoi(argv[2]), T = std::atoi(argv[3]);
    for (int trip = 0; 16 * trip <= T; ++trip)
      for (int s = 0; s < nx; ++s)
        for (int lane = 0; lane < 64; ++lane)
          std::printf("%d %d %d %d\n", trip, s, lane, 8 * l::index(nx, l::read_node(T, (lane & 15) + 16 * trip), s));
  } else if (is("slots")) {
    const int nx = std::atoi(argv[2]), d = std::atoi(argv[3]);
    for (int i = 0; i < nx - d; ++i) std::printf("%d %d\n", l::offdiag_c(d, i), l::offdiag_slot(d, l::offdiag_c(d, i)));
    for (int a = 0; a < d; ++a) std::printf("%d %d\n", a, l::diag_slot(nx, d, a));
  } else {
    return 4;
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The header compiled with the plain host compiler (no HIP include path); returns a function that runs the driver."""
    tmp = tmp_path_factory.mktemp("ls_table")
    (tmp / "driver.cpp").write_text(_DRIVER)
    exe = str(tmp / "ls_table_host")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "mpc4quantum_amd", "csrc"), str(tmp / "driver.cpp"),
                    "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


def _weights():
    """4 n staged weights [wq | wqf], all different, none a sum that rounds."""
    return [0.3 + 0.0173 * i + 1.0 / (7 + i) for i in range(4 * NX)]


def _weight(w, T, q):
    blk = q // (2 * NX)
    r = q - blk * (2 * NX)
    return (w[2 * NX:] if blk == T else w[:2 * NX])[r]


def test_slot_order(host):
    lines = [(int(a), int(b)) for a, b in host("slots", NX, D)]
    offd = [c for c in range(1, NX) if c // D != c % D]
    assert lines[:NX - D] == [(c, i) for i, c in enumerate(offd)]
    assert lines[NX - D:] == [(a, NX - D + a) for a in range(D)]


@pytest.mark.parametrize("T", TABLE_HORIZONS)
def test_entries_equal_the_direct_expression(T, host):
    w = _weights()
    assert len(set(w)) == len(w)
    lines = host("table", NX, D, T, *[x.hex() for x in w])
    got = {(int(t), int(s)): float.fromhex(v) for t, s, v in lines}
    assert len(got) == (T + 1) * NX
    nxt = NX * (T + 1)
    offd = [c for c in range(1, NX) if c // D != c % D]
    for t in range(T + 1):
        for s, c in enumerate(offd):
            a, b = c // D, c % D
            off = nxt if a > b else 0
            want = 0.5 * (_weight(w, T, c * (T + 1) + t + off) + _weight(w, T, (b * D + a) * (T + 1) + t + off))
            assert got[t, s].hex() == want.hex(), (T, t, s)
        for a in range(D):
            want = _weight(w, T, (a * D + a) * (T + 1) + t)
            assert got[t, NX - D + a].hex() == want.hex(), (T, t, a)


def test_capacity(host):
    (pitch, nodes, nbytes), = [[int(v) for v in ln] for ln in host("cap", NX, WORKGROUP_BEFORE)]
    assert pitch == 8 * NX == 72
    assert nodes == (WORKGROUP_LIMIT - WORKGROUP_BEFORE) // 72 == 47
    assert nbytes == 47 * 72 and WORKGROUP_BEFORE + nbytes <= WORKGROUP_LIMIT
    assert host("tabled", 46, nodes) == [["1"]] and host("tabled", 47, nodes) == [["0"]]
    assert host("tabled", 1, nodes) == [["1"]] and host("tabled", 80, nodes) == [["0"]]
    assert [int(v) for v in host("cap", NX, WORKGROUP_LIMIT)[0]][1:] == [0, 0]           # a full workgroup: no table
    assert [int(v) for v in host("cap", NX, WORKGROUP_LIMIT + 8)[0]][1:] == [0, 0]


@pytest.mark.parametrize("T", TABLE_HORIZONS)
def test_reads_hit_their_node_without_a_bank_conflict(T, host):
    reads = [tuple(int(v) for v in ln) for ln in host("reads", NX, T)]
    trips = T // 16 + 1
    assert len(reads) == trips * NX * 64
    by = {}
    for trip, s, lane, a in reads:
        t = (lane & 15) + 16 * trip
        assert a == 72 * (t if t <= T else T) + 8 * s and 0 <= a and a + 8 <= 72 * (T + 1), (T, trip, s, lane, a)
        by.setdefault((trip, s, lane >> 5), []).append(a)
    assert len(by) == trips * NX * 2
    for key, addrs in by.items():
        owner = {}
        for a in addrs:
            for bank in ((a // 4) % 64, (a // 4 + 1) % 64):
                assert owner.setdefault(bank, a) == a, "read %s at T = %d: addresses %d and %d on bank %d" % (key, T, owner[bank], a, bank)
