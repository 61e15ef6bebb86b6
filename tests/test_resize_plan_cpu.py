"""The resolver of the resample work list (csrc/pjd_resize_plan.cpp: what a batch was asked for -> the records the resize kernels read)
under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: the unit is plain C++ and needs no device.

tools/resize_plan_host.cpp holds the checks: every limit on both sides of its boundary with the picture it names, the full cross of
pads, orientations, windows, filters and layouts against statements written out from include/pjd.h, and the request grown call by
call, as the setters of pjd_api.hip grow it, against the same request resolved in one go."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_resolver_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "resize_plan_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__host__=", "-D__device__=",
           os.path.join(ROOT, "tools", "resize_plan_host.cpp"), os.path.join(ROOT, "pim-jpeg-decoder_amd", "csrc", "pjd_resize_plan.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("this toolchain has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout and " 0 checks failed" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
