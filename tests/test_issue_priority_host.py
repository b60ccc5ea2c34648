"""Where the compiled closed-loop kernels change their issue priority (no GPU: disassembly of the built object only).

mpc_kernel sets the wavefront's issue priority by phase of its main loop (m4q_kernels.hip: prio_map; m4q_device.h: issue_prio).
s_setprio is scalar and ignores EXEC, so a switch placed inside a lane-dependent branch runs for the whole wavefront anyway, and a
wavefront that polls for a head, or leaves, at a raised level outranks the wavefront it shares the SIMD with for nothing.  For
every mpc_kernel instantiation of the headline shape's object this checks, on the instructions the compiler emitted:

- no s_setprio inside a horizon loop (the loops tools/hot_loops.py reports), nor in any other loop nested in the main loop;
- no s_setprio at all in a kernel whose table is all zeros (RAISED below mirrors prio_map);
- a kernel with levels has them, and on no path of its control-flow graph does a raised level reach the poll's s_sleep or
  s_endpgm without passing an s_setprio 0.

Skipped where the object has not been built."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "mpc4quantum_amd", "csrc", "build", "kernels_9_2_1.o")
LLVM = "/opt/rocm/lib/llvm/bin/"

pytestmark = pytest.mark.skipif(not os.path.exists(OBJ), reason="kernels_9_2_1.o has not been built")


def RAISED(s, plant, exact, tl, tile, sg):
    """prio_map of m4q_kernels.hip: the instantiations whose table has a level above 0."""
    return plant == 1 and tile and not exact   # (PLANT_HAMILTONIAN; this object's shape is the one with levels: n = 9)


@functools.lru_cache(maxsize=None)
def _kernels():
    """{symbol: [(address, instruction text)]} of the object's code."""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=%s/fat.bin" % tmp, OBJ])
        subprocess.check_call([LLVM + "clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=%s/fat.bin" % tmp, "--output=%s/k.co" % tmp, "--unbundle"])
        dis = subprocess.check_output([LLVM + "llvm-objdump", "-d", "%s/k.co" % tmp], text=True)
    out, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        m = re.match(r"\s+(\S.*?)\s*//\s*([0-9A-F]{12}):", line)
        if cur and m:
            out[cur].append((int(m.group(2), 16), m.group(1)))
    return out


def _mpc_kernels():
    return {k: v for k, v in _kernels().items() if "mpc_kernel" in k}


def _template_args(name):
    m = re.search(r"mpc_kernelI([a-zA-Z0-9_]+?)Li(\d+)ELb([01])ELb([01])ELb([01])ELb([01])E", name)
    assert m, name
    return (m.group(1), int(m.group(2))) + tuple(g == "1" for g in m.groups()[2:])


def _graph(ins):
    """Successors of every instruction (index into ins): fall-through and branch target.  A call (s_swappc_b64) comes back: the
    functions of this object hold no s_setprio and no s_sleep (test_only_the_closed_loop_kernels_switch).  An indirect jump is not
    followed: a kernel with levels must not have one."""
    at = {a: i for i, (a, _) in enumerate(ins)}
    succ = []
    for i, (a, text) in enumerate(ins):
        s = []
        m = re.match(r"(s_cbranch_\w+|s_branch)\s+(\d+)", text)
        assert not text.startswith("s_setpc"), "indirect jump: the graph does not follow it"
        if m:
            off = int(m.group(2))
            off = off - 65536 if off > 32767 else off
            t = a + 4 + 4 * off
            assert t in at, (hex(a), text)
            s.append(at[t])
        if not text.startswith("s_branch") and not text.startswith("s_endpgm") and i + 1 < len(ins):
            s.append(i + 1)
        succ.append(s)
    return succ


def _on_inner_cycle(ins, succ, i):
    """Is instruction i on a cycle that does not pass the watchdog's clock read?  Every pass of the main loop reads that clock
    (s_memrealtime), so such a cycle is a loop inside the main loop: the horizon loops tools/hot_loops.py reports are among them,
    wherever the compiler laid their blocks out."""
    seen, todo = set(), list(succ[i])
    while todo:
        k = todo.pop()
        if k == i:
            return True
        if k in seen or "s_memrealtime" in ins[k][1]:
            continue
        seen.add(k)
        todo.extend(succ[k])
    return False


def test_the_object_holds_the_closed_loop_kernels():
    ks = _mpc_kernels()
    assert len(ks) >= 10, sorted(ks)
    assert any(_template_args(k)[1:] == (1, False, True, True, False) for k in ks), "the headline kernel is one of them"


def test_only_the_closed_loop_kernels_switch():
    for name, ins in _kernels().items():
        if "mpc_kernel" not in name:
            assert not any(t.startswith("s_setprio") for _, t in ins), name


@pytest.mark.parametrize("which", ["horizon_loops", "zero_tables", "paths"])
def test_priority_switches(which):
    for name, ins in _mpc_kernels().items():
        args = _template_args(name)
        prio = [(i, int(t.split()[1])) for i, (_, t) in enumerate(ins) if t.startswith("s_setprio")]
        if which == "zero_tables":
            if not RAISED(*args):
                assert not prio, (name, prio)
            else:
                assert any(p > 0 for _, p in prio) and any(p == 0 for _, p in prio), (name, prio)
            continue
        if not prio:
            continue
        succ = _graph(ins)
        if which == "horizon_loops":
            assert sum("s_memrealtime" in t for _, t in ins) == 2, name          # the deadline at entry, the check of every pass
            mfma = [i for i, (_, t) in enumerate(ins) if "v_mfma_f64" in t or "v_fmac_f64_dpp" in t]
            assert any(_on_inner_cycle(ins, succ, i) for i in mfma[:50]), name   # (the walk does find the sweeps' loops)
            for i, _ in prio:
                assert not _on_inner_cycle(ins, succ, i), (name, hex(ins[i][0]), ins[i][1])
            continue
        # paths: walk forward from every raised switch; a walk ends at the next s_setprio (the level is then that one's)
        for start, level in prio:
            if level == 0:
                continue
            seen, todo = set(), list(succ[start])
            while todo:
                i = todo.pop()
                if i in seen:
                    continue
                seen.add(i)
                text = ins[i][1]
                if text.startswith("s_setprio"):
                    continue
                assert not text.startswith("s_sleep") and not text.startswith("s_endpgm"), \
                    (name, "level %d set at %#x reaches %s at %#x" % (level, ins[start][0], text, ins[i][0]))
                todo.extend(succ[i])
