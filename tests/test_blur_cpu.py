"""The Gaussian blur of include/pjd.h (pjd_batch_set_blur) on the CPU: the exported taps, border rule and entry check against a model in
integers (tests/blur_model.py); what the header says of the identity, of a constant picture and of its sums; its bound against float64;
and the host tool -- the kernel body run on the host over the resolver's records, with the resolver's rules for a blurred request --
built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a process of its own, its outputs held against the model.  No
device is needed."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import blur_model as M
import pjd_amd
from pjd_amd import tensors

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KSIZES = (1, 3, 5, 23, 63)
SIGMAS = (0.1, 0.5, 1, 2, 3.7, 10, 100, 1e308, 5e-324)


def test_exports_exist_and_the_version_stays_6():
    L = pjd_amd.dev_lib()
    assert all(hasattr(L, f) for f in ("pjd_batch_set_blur", "pjd_blur_taps", "pjd_blur_index", "pjd_blur_check"))
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert callable(pjd_amd.Batch.set_blur) and callable(pjd_amd.blur_taps) and callable(pjd_amd.blur_index) and callable(pjd_amd.blur_check)
    assert pjd_amd.BLUR_MAX_TAPS == 63 == M.MAX_TAPS and C.sizeof(pjd_amd.Blur) == 16
    q, src = (C.c_uint32 * 3)(), C.c_uint32()
    assert L.pjd_blur_taps(3, 1.0, None) == -3 and L.pjd_blur_taps(3, 1.0, q) == 0 and sum(q) == 65536
    assert L.pjd_blur_taps(0, 0.0, q) == -3 and L.pjd_blur_taps(2, 1.0, q) == -3 and L.pjd_blur_taps(3, 0.0, q) == -3
    assert L.pjd_blur_index(5, 7, None) == -3 and L.pjd_blur_index(0, 0, src) == -3 and L.pjd_blur_index(65536, 0, src) == -3
    assert L.pjd_blur_index(65535, -(2 ** 63), src) == 0 and src.value == M.index(65535, -(2 ** 63))
    assert L.pjd_blur_index(65535, 2 ** 63 - 1, src) == 0 and src.value == M.index(65535, 2 ** 63 - 1)
    assert L.pjd_blur_check(None) == 0 and L.pjd_batch_set_blur(None, None) == -3


@pytest.mark.parametrize("ksize", KSIZES)
def test_taps_are_symmetric_sum_to_65536_and_follow_the_formula(ksize):
    for sigma in SIGMAS:
        q = pjd_amd.blur_taps(ksize, sigma)
        assert len(q) == ksize and q == q[::-1] and min(q) >= 0 and sum(q) == 65536, (ksize, sigma, q)
        assert max(q) == q[ksize // 2]
        # the two libms may differ in the last bit of exp: one unit, not equality
        assert max(abs(a - b) for a, b in zip(q, M.taps_float(ksize, sigma))) <= 1, (ksize, sigma)
    assert pjd_amd.blur_taps(ksize, 0.1)[ksize // 2] == 65536 == pjd_amd.blur_taps(ksize, 5e-324)[ksize // 2]      # the centre alone
    box = pjd_amd.blur_taps(ksize, 1e308)
    assert min(box) == 65536 // ksize and max(box) - min(box) <= ksize // 2 + 1                                    # a box: the centre takes the remainder


def test_the_border_rule_against_the_model():
    for n in (1, 2, 3, 7):
        for i in range(-200, 201):
            assert pjd_amd.blur_index(n, i) == M.index(n, i), (n, i)
    assert [pjd_amd.blur_index(4, i) for i in range(-7, 11)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert [pjd_amd.blur_index(2, i) for i in range(-3, 4)] == [1, 0, 1, 0, 1, 0, 1]
    with pytest.raises(ValueError):
        pjd_amd.blur_index(0, 0)
    with pytest.raises(ValueError):
        pjd_amd.blur_index(65536, 0)


def seeded_pictures(rng, h, w):
    yield "random", rng.integers(0, 256, (h, w), dtype=np.uint8)
    yield "black/white", (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    yield "constant", np.full((h, w), int(rng.integers(0, 256)), np.uint8)


def test_the_model_is_within_one_level_of_float64():
    """Derived bound (include/pjd.h): 0.5 + 2^-9 + 2 * ksize * 255 / 65536, below one level at 63 taps.  Worst found here: 0.5063 levels
    (7 rows x 9 columns, 41 taps, sigma 100, black/white)."""
    rng = np.random.default_rng(2025)
    sizes = [(1, 1), (1, 2), (2, 1), (3, 5), (7, 9), (33, 37), (41, 70)]
    worst = (0.0, None)
    for h, w in sizes:
        for ksize in (1, 3, 5, 11, 23, 41, 63):
            for sigma in (0.1, 0.5, 1.0, 2.0, 3.7, 10.0, 100.0):
                for kind, u in seeded_pictures(rng, h, w):
                    d = float(np.abs(M.blur(u, (ksize, sigma)).astype(np.float64) - M.blur_float(u, (ksize, sigma))).max())
                    assert d <= 0.5 + 2.0 ** -9 + 2 * ksize * 255 / 65536 < 1.0, (h, w, ksize, sigma, kind, d)
                    if d > worst[0]:
                        worst = (d, (h, w, ksize, sigma, kind))
    print("worst difference from float64:", worst)
    assert worst[0] <= 1.0


def test_identity_tables_and_constant_pictures():
    rng = np.random.default_rng(7)
    u = rng.integers(0, 256, (3, 9, 13), dtype=np.uint8)
    for entry in (None, (1, 1.0), (1, 100.0), (3, 0.1), (23, 0.1), (63, 0.1), (63, 5e-324)):
        if entry is not None:
            assert M.is_identity(M.taps(*entry)), entry
        assert np.array_equal(M.blur(u, entry), u), entry
    assert not M.is_identity(M.taps(3, 0.8))
    for v in (0, 1, 127, 254, 255):
        for entry in ((3, 0.8), (23, 2.0), (63, 10.0), (63, 1e308)):
            assert np.array_equal(M.blur(np.full((5, 4), v, np.uint8), entry), np.full((5, 4), v, np.uint8)), (v, entry)
    hwc = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)
    assert np.array_equal(M.interleaved(hwc, (5, 1.0))[:, :, 1], M.blur(hwc[:, :, 1], (5, 1.0)))


def test_the_worst_case_sums():
    assert 255 * 65536 == 16711680 < 1 << 24                                        # the row sum, as a 24-bit operand
    assert (255 * 65536 + 128) >> 8 == 65280 < 1 << 16                              # the row sample, 16 bits
    assert 65536 * 65280 + (1 << 23) == 4286578688 < 1 << 32                        # the column sum with its rounding term
    assert (65536 * 65280 + (1 << 23)) >> 24 == 255
    assert 65536 < 1 << 24 and 65280 < 1 << 24                                      # both operands of every 24-bit multiply
    white = np.full((70, 41), 255, np.uint8)
    for entry in ((63, 1e308), (63, 0.1), (1, 1.0), (23, 2.0)):
        assert np.array_equal(M.blur(white, entry), white), entry


def test_every_refusal_of_blur_check():
    for ksize, sigma, ok in (
            (0, 0.0, True), (1, 1.0, True), (3, 0.1, True), (63, 100.0, True), (63, 5e-324, True), (63, 1.7976931348623157e308, True),
            (2, 1.0, False), (62, 1.0, False), (64, 1.0, False), (65, 1.0, False), (2 ** 32 - 1, 1.0, False),
            (3, 0.0, False), (3, -0.0, False), (3, -1.0, False), (3, float("nan"), False), (3, float("inf"), False), (3, float("-inf"), False),
            (0, 0.5, False), (0, -1.0, False), (0, float("nan"), False), (0, -0.0, True)):
        assert pjd_amd.blur_check(ksize, sigma) is ok and M.check(ksize, sigma) is ok, (ksize, sigma)
    assert not pjd_amd.blur_check(3, 1.0, reserved=1) and not pjd_amd.blur_check(0, 0.0, reserved=1) and not M.check(3, 1.0, 1)
    for ksize, sigma in ((0, 0.0), (2, 1.0), (65, 1.0), (3, 0.0), (3, float("nan"))):
        with pytest.raises(ValueError):
            pjd_amd.blur_taps(ksize, sigma)


def test_blurs_keyword_is_checked_before_anything_is_created():
    sc = pjd_amd.Scanned(open(os.path.join(HERE, "golden", "env_61x45_422_q30.jpg"), "rb").read())
    for fn, extra in ((tensors.decode_resized_batch_tensor, ()), (tensors.decode_normalized_batch_tensor, ((0.5,) * 3, (0.25,) * 3))):
        with pytest.raises(ValueError, match="blurs= has one"):
            fn(None, [sc.desc], (8, 8), *extra, blurs=[(3, 1.0), None])
        with pytest.raises(ValueError, match="blurs= has one"):
            fn(None, [sc.desc, sc.desc], (8, 8), *extra, views=[0, 1, 1], blurs=[(3, 1.0), None])
        with pytest.raises(ValueError, match="blurs= excludes letterbox="):
            fn(None, [sc.desc], (8, 8), *extra, letterbox="center", blurs=[(3, 1.0)])


# ---- the host tool, under the sanitizers ---------------------------------------------------------------------------------------------
def host_clang():
    """a clang++ for the host: the store header of the resample uses clang's vector extensions and 16-bit float types"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (shutil.which("clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    return None


def test_blur_body_and_resolver_rules_under_asan_ubsan(tmp_path):
    """tools/blur_host.cpp: the blur body over the resolver's records, all twelve forms, its own expectation and the guards; the resolver's
    rules (shared tap rows, identity flags, the pad refusal in both orders, the faults that name the view); then its planar uint8 outputs
    -- widths 1, 2, 5, 37, 259 x heights 1, 7, 9, 33, 70 x 1, 3, 23, 63 taps and the identities -- against the model"""
    cxx = host_clang()
    assert cxx, "no clang++ beside hipcc: the compiler that builds the library is needed"
    exe, dump = tmp_path / "blur_host", tmp_path / "blur_host.bin"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-omit-frame-pointer", "-D__host__=", "-D__device__=",
           os.path.join(ROOT, "tools", "blur_host.cpp"), os.path.join(ROOT, "pim-jpeg-decoder_amd", "csrc", "pjd_resize_plan.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = r.stdout
    assert "ALL EQUAL" in out and "no sanitizer report" in out and " 0 checks failed" in out and "MISMATCH" not in out, out[-3000:]
    assert "blurred request: resolver rules checked" in out
    assert out.count("equal, guards intact") == 3 + 4 * 9, out[-3000:]
    raw, pos, seen = dump.read_bytes(), 0, set()
    while pos < len(raw):
        w, h, ksize, sigma = struct.unpack_from("<IIId", raw, pos)
        pos += 20
        u = np.frombuffer(raw, np.uint8, 3 * w * h, pos).reshape(3, h, w)
        got = np.frombuffer(raw, np.uint8, 3 * w * h, pos + 3 * w * h).reshape(3, h, w)
        pos += 6 * w * h
        assert np.array_equal(got, M.blur(u, (ksize, sigma) if ksize else None)), (w, h, ksize, sigma)
        seen.add((w, h, ksize))
    assert pos == len(raw)
    assert {(w, h, k) for w in (1, 2, 5, 37, 259) for h in (1, 7, 9, 33, 70) for k in (1, 3, 23, 63)} <= seen and any(k == 0 for _, _, k in seen)
