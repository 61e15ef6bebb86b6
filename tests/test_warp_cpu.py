"""The affine warp of include/pjd.h (pjd_batch_set_resize_affine) on the CPU: the exported tap against a Python-integer model
(tests/warp_model.py) at seeded matrices and at every limit; the model against the same filter in float64 and against torch's
grid_sample, within the 1 level the header derives; and tools/warp_host.cpp -- the kernel body run on the host over the resolver's
records, all twelve forms, and the resolver's rules for an affine request -- built with AddressSanitizer + UndefinedBehaviorSanitizer
and run as a process of its own, the way tests/test_resize_plan_cpu.py runs tools/resize_plan_host.cpp.  No device is needed."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pjd_amd
import warp_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

IDENT = [1, 0, 0, 0, 1, 0]


def rng_maps(n, sw, sh, tw, th, seed):
    """seeded maps; each is first held against the library at the corners and the middle of its target, so that what the tests below
    say about the model they say about the exported arithmetic"""
    rng = np.random.default_rng(seed)
    maps = [M.similarity(rng, sw, sh, tw, th) for _ in range(n)]
    for m in maps:
        for i, j in [(0, 0), (tw - 1, 0), (0, th - 1), (tw - 1, th - 1), (tw // 2, th // 2)]:
            assert pjd_amd.warp_tap(m, i, j) == M.tap(m, i, j), (m, i, j)
    return maps


def test_warp_tap_equals_the_model_on_seeded_matrices():
    rng = np.random.default_rng(20240)
    for k in range(300):
        lin = rng.uniform(-16, 16, 4) if k % 3 else rng.uniform(-1.5, 1.5, 4)
        sh = rng.uniform(-262144, 262144, 2) if k % 2 else rng.uniform(-300, 300, 2)
        m = [lin[0], lin[1], sh[0], lin[2], lin[3], sh[1]]
        for i, j in [(0, 0), (65534, 65534), (65534, 0), (0, 65534), (int(rng.integers(65535)), int(rng.integers(65535)))]:
            assert pjd_amd.warp_tap(m, i, j) == M.tap(m, i, j), (m, i, j)


def test_warp_tap_at_the_limits():
    big, far = 16.0, 262144.0
    # every limit met exactly, either sign, at the last pixel: the largest sums the 64-bit arithmetic sees
    for s0 in (1, -1):
        for s1 in (1, -1):
            m = [s0 * big, s0 * big, s1 * far, -s0 * big, s0 * big, -s1 * far]
            for i, j in [(0, 0), (65534, 65534), (65534, 0)]:
                assert pjd_amd.warp_tap(m, i, j) == M.tap(m, i, j)
            assert pjd_amd.resize_affine_check(65535, 65535, 65535, 65535, m)
    # the limits are on the QUANTISED values: 16 + 1 ulp quantises to 16 * 2^40 and passes, the next quantised value 16 + 2^-40 does not
    assert M.quantise([math.nextafter(big, 17)] + IDENT[1:])[0] == 16 << 40
    assert pjd_amd.warp_tap([math.nextafter(big, 17)] + IDENT[1:], 3, 4) == pjd_amd.warp_tap([big] + IDENT[1:], 3, 4)
    for k in range(6):
        lim = far if k in (2, 5) else big
        for sign in (1, -1):
            ok = list(IDENT); ok[k] = sign * lim
            assert pjd_amd.resize_affine_check(40, 30, 20, 10, ok) and pjd_amd.warp_tap(ok, 1, 2) == M.tap(ok, 1, 2)
            # the next quantised value; beside 2^18 the next double is already 2^-34 away
            over = list(IDENT); over[k] = sign * (lim + 2.0 ** -40) if lim == big else sign * math.nextafter(lim, 2 * lim)
            assert not pjd_amd.resize_affine_check(40, 30, 20, 10, over), (k, sign)
            with pytest.raises(ValueError):
                pjd_amd.warp_tap(over, 1, 2)
            with pytest.raises(ValueError):
                M.quantise(over)
        for bad in (float("nan"), float("inf"), float("-inf"), 1e300):
            m = list(IDENT); m[k] = bad
            assert not pjd_amd.resize_affine_check(40, 30, 20, 10, m)
            with pytest.raises(ValueError):
                pjd_amd.warp_tap(m, 0, 0)
    # i, j: 65534 is the last pixel there can be
    assert pjd_amd.warp_tap(IDENT, 65534, 65534) == (65534, 65534, 0, 0)
    for i, j in [(65535, 0), (0, 65535), (2 ** 32 - 1, 0)]:
        with pytest.raises(ValueError):
            pjd_amd.warp_tap(IDENT, i, j)
    # dimensions 1..65535
    assert pjd_amd.resize_affine_check(1, 1, 1, 1, IDENT) and pjd_amd.resize_affine_check(65535, 65535, 65535, 65535, IDENT)
    for dims in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (65536, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 65536, 1), (1, 1, 1, 65536)]:
        assert not pjd_amd.resize_affine_check(*dims, IDENT)
    # null: the matrix, and every output
    L = pjd_amd.dev_lib()
    import ctypes as C
    assert L.pjd_warp_tap(None, 0, 0, None, None, None, None) == -3         # PJD_E_ARG
    assert L.pjd_resize_affine_check(4, 4, 4, 4, None) == -3
    assert L.pjd_warp_tap((C.c_double * 6)(*IDENT), 5, 6, None, None, None, None) == 0


def test_rounding_is_to_nearest_even_and_negative_positions_floor():
    # 2^-41 is half a unit of Q40: ties go to the even neighbour
    assert M.quantise([2.0 ** -41, 3 * 2.0 ** -41, 0, 0, 0, 0])[:2] == [0, 2]
    m = [1, 0, -2.75, 0, 1, -0.25]                          # u - 1/2 = i - 2.75: x0 = -3 at i = 0, weight 64
    assert M.tap(m, 0, 0) == (-3, -1, 64, 192) == pjd_amd.warp_tap(m, 0, 0)
    # 1/512 of a pixel is half a unit of fx: (X + 2^32) >> 33 rounds it up, towards +inf, also below zero: -1/512 becomes 0
    assert pjd_amd.warp_tap([1, 0, 1 / 512, 0, 1, -1 / 512], 0, 0) == (0, 0, 1, 0) == M.tap([1, 0, 1 / 512, 0, 1, -1 / 512], 0, 0)


PIC = (np.random.default_rng(7).integers(0, 2, (3, 23, 37)) * 255).astype(np.uint8)       # 37 x 23, samples 0 / 255
FILL = (255, 0, 128)


def test_the_consequences_the_header_states():
    sw, sh = 37, 23
    assert pjd_amd.warp_tap([0, -1, sw, 1, 0, 0], 3, 4) == (sw - 1 - 4, 3, 0, 0)
    assert np.array_equal(M.warp(PIC, IDENT, sw, sh, FILL), PIC)
    assert np.array_equal(M.warp(PIC, [0, -1, sw, 1, 0, 0], sh, sw, FILL), np.rot90(PIC, 1, (1, 2)))       # D[j][i] = P[i][sw - 1 - j]: counter-clockwise
    assert np.array_equal(M.warp(PIC, [0, 1, 0, -1, 0, sh], sh, sw, FILL), np.rot90(PIC, -1, (1, 2)))
    assert np.array_equal(M.warp(PIC, [-1, 0, sw, 0, 1, 0], sw, sh, FILL), PIC[:, :, ::-1])
    moved = M.warp(PIC, [1, 0, -5, 0, 1, 3], sw, sh, FILL)
    assert np.array_equal(moved[:, :sh - 3, 5:], PIC[:, 3:, :sw - 5])
    for c in range(3):
        assert (moved[c, :, :5] == FILL[c]).all() and (moved[c, sh - 3:, :] == FILL[c]).all()
    const = np.full((3, 23, 37), 77, np.uint8)
    inside = M.warp(const, [0.31, -0.2, 12, 0.17, 0.4, 4], 20, 20, FILL)
    assert (inside == 77).all()
    # the vectorised model and the per-pixel one through tap() are one model
    for m in rng_maps(3, sw, sh, 19, 17, 5):
        assert np.array_equal(M.warp(PIC, m, 19, 17, FILL), M.warp_scalar(PIC, m, 19, 17, FILL))


def test_model_within_one_level_of_float64_bilinear():
    worst = 0
    for m in rng_maps(40, 37, 23, 31, 29, 99):
        got = M.warp(PIC, m, 31, 29, FILL).astype(np.int64)
        want = np.rint(M.warp_float64(PIC, m, 31, 29, FILL)).astype(np.int64)
        worst = max(worst, int(np.abs(got - want).max()))
    print("largest difference to the float64 filter:", worst)
    assert worst <= 1


def test_model_within_one_level_of_grid_sample():
    import torch
    F = torch.nn.functional
    sw, sh, tw, th = 37, 23, 31, 29
    img = torch.from_numpy(PIC.astype(np.float64))[None]
    fill = torch.tensor(FILL, dtype=torch.float64).view(1, 3, 1, 1)
    worst = 0
    for m in rng_maps(40, sw, sh, tw, th, 99):
        theta = torch.tensor([[m[0] * tw / sw, m[1] * th / sw, (m[0] * tw + m[1] * th + 2 * m[2]) / sw - 1],
                              [m[3] * tw / sh, m[4] * th / sh, (m[3] * tw + m[4] * th + 2 * m[5]) / sh - 1]], dtype=torch.float64)[None]
        grid = F.affine_grid(theta, (1, 3, th, tw), align_corners=False)
        out = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        mask = F.grid_sample(torch.ones(1, 1, sh, sw, dtype=torch.float64), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        want = torch.round(out + (1 - mask) * fill)[0].numpy().astype(np.int64)
        got = M.warp(PIC, m, tw, th, FILL).astype(np.int64)
        worst = max(worst, int(np.abs(got - want).max()))
    print("largest difference to grid_sample:", worst)
    assert worst <= 1


def host_clang():
    """a clang++ for the host: the store header of the resample uses clang's vector extensions and 16-bit float types"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (shutil.which("clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    return None


def test_kernel_body_and_resolver_under_asan_ubsan(tmp_path):
    cxx = host_clang()
    assert cxx, "no clang++ beside hipcc: the compiler that builds the library is needed"
    exe = tmp_path / "warp_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-omit-frame-pointer", "-D__host__=", "-D__device__=",
           os.path.join(ROOT, "tools", "warp_host.cpp"), os.path.join(ROOT, "pim-jpeg-decoder_amd", "csrc", "pjd_resize_plan.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ALL EQUAL" in r.stdout and "no sanitizer report" in r.stdout and " 0 checks failed" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
