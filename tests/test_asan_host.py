"""AddressSanitizer build of the host side of the C ABI ("Race detection / sanitizers").

m4q_capi.hip - 1,350 lines of pointer / size handling (field tables, bind_output, put_state, the one-shot entry points'
temporary buffers, the communicator) - is compiled host-only with -fsanitize=address, linked with the product's kernel
objects and tests/asan/capi_driver.cpp, and run with the devices hidden: every entry point on its argument-validation paths and
on its no-device path (leak check on).  The sanitizer is for host code only: the compile of m4q_capi.hip is host-only and the
kernel objects come from the normal build, and every line that enables the sanitizer also says -fno-gpu-sanitize, so that its
host-only scope is stated where it is used (the driver's with-device branch is there for a workstation with a GPU:
M4Q_ASAN_WITH_DEVICE=1 python -m pytest tests/test_asan_host.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc4quantum_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"


def build_driver(tmp):
    from mpc4quantum_amd.csrc import build as hip_build
    hip_build.build()                                             # the kernel objects the driver links with
    objs = sorted(os.path.join(hip_build.OBJ, f) for f in os.listdir(hip_build.OBJ) if f.startswith("kernels_") and f.endswith(".o"))
    capi = os.path.join(tmp, "capi_asan.o")
    drv = os.path.join(tmp, "capi_driver.o")
    exe = os.path.join(tmp, "capi_asan_driver")
    host_asan = ["-fsanitize=address", "-fno-gpu-sanitize", "-Wno-unused-command-line-argument"]
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-fPIC"] + host_asan +
                   ["-c", os.path.join(CSRC, "m4q_capi.hip"), "-o", capi], check=True)
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17"] + host_asan + ["-c", os.path.join(ROOT, "tests", "asan", "capi_driver.cpp"),
                                                                     "-o", drv], check=True)
    subprocess.run([CLANG] + host_asan + [drv, capi] + objs + ["-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl",
                                                               "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.timeout(600)
def test_capi_host_side_under_asan_without_a_device(tmp_path):
    exe = build_driver(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    if os.environ.get("M4Q_ASAN_WITH_DEVICE") != "1":
        env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        if os.path.exists("/dev/kfd"):
            # a node with an AMD GPU: there the ROCm runtime keeps two small process-lifetime allocations (144 bytes, made in
            # libhsa-runtime64) even with every device hidden.  LSan matches a suppression against every frame of a stack, so
            # this exempts any leak allocated through libhsa-runtime64.  With every device hidden the C ABI can create no stream,
            # event or device buffer (each such HIP call fails), and its own new / malloc calls are still checked.  Without the
            # driver (no GPU) nothing is exempt.
            supp = os.path.join(str(tmp_path), "lsan.supp")
            with open(supp, "w") as f:
                f.write("leak:libhsa-runtime64.so\n")
            env["LSAN_OPTIONS"] = "suppressions=" + supp
    else:
        env["ASAN_OPTIONS"] = "detect_leaks=0:halt_on_error=1"      # (the HIP runtime keeps process-lifetime allocations)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout[-3000:] + out.stderr[-6000:]
    assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
