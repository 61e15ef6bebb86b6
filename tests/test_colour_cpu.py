"""The colour map of include/pjd.h (pjd_batch_set_colour) on the CPU: the exported arithmetic against a Python-integer model
(tests/colour_model.py) on seeded matrices, at the worst-case sums and at every limit; what the header says is exact, and its bound
against float64; the pure helper pjd_amd.tensors.colour_matrix factor by factor; and the three host tools -- the resample and warp
bodies run on the host over the resolver's records with a colour map per output, and the resolver's rules for a coloured request --
built with AddressSanitizer + UndefinedBehaviorSanitizer and run as processes of their own.  No device is needed."""
import ctypes as C
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import colour_model as M
import pjd_amd
from pjd_amd import tensors

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
IDENT = list(M.IDENTITY)
CORNERS = list(itertools.product((0, 255), repeat=3))
PERMS = list(itertools.permutations(range(3)))


def seeded_matrix(rng, k):
    """within the limits: every third one over the whole range of weights and offsets, the others of a jitter's size"""
    if k % 3 == 0:
        return [float(rng.uniform(-4096, 4096)) if i % 4 == 3 else float(rng.uniform(-16, 16)) for i in range(12)]
    return list(M.jitter(rng))


def test_exports_exist_and_the_version_stays_6():
    L = pjd_amd.dev_lib()
    assert hasattr(L, "pjd_batch_set_colour") and hasattr(L, "pjd_colour_value") and hasattr(L, "pjd_colour_check")
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert callable(pjd_amd.Batch.set_colour) and callable(pjd_amd.colour_value) and callable(pjd_amd.colour_check) and callable(tensors.colour_matrix)
    # null pointers
    m, rgb, out = (C.c_double * 12)(*IDENT), (C.c_uint8 * 3)(1, 2, 3), (C.c_uint8 * 3)()
    assert L.pjd_colour_check(None) == 0 and L.pjd_colour_check(m) == 1
    assert L.pjd_colour_value(None, rgb, out) == -3 and L.pjd_colour_value(m, None, out) == -3 and L.pjd_colour_value(m, rgb, None) == -3
    assert L.pjd_colour_value(m, rgb, out) == 0 and list(out) == [1, 2, 3]
    assert L.pjd_batch_set_colour(None, None) == -3


def test_colour_value_equals_the_model_on_seeded_matrices():
    rng = np.random.default_rng(20250)
    for k in range(300):
        m = seeded_matrix(rng, k)
        assert pjd_amd.colour_check(m) and M.check(m)
        for rgb in CORNERS + [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(64)]:
            assert pjd_amd.colour_value(m, rgb) == M.value(m, rgb), (m, rgb)


def test_the_worst_case_sums():
    """every weight +16 or -16 with the offset +4096 or -4096, at white and at black: the largest sums the 32-bit arithmetic sees"""
    for signs in itertools.product((1, -1), repeat=4):
        m = [s * (4096.0 if i == 3 else 16.0) for _ in range(3) for i, s in enumerate(signs)]
        for rgb in ((255, 255, 255), (0, 0, 0)):
            assert pjd_amd.colour_value(m, rgb) == M.value(m, rgb), (signs, rgb)
    assert pjd_amd.colour_value([16, 16, 16, 4096] * 3, (255, 255, 255)) == (255, 255, 255)
    assert pjd_amd.colour_value([-16, -16, -16, -4096] * 3, (255, 255, 255)) == (0, 0, 0)
    assert 3 * 255 * (1 << 20) + (1 << 28) + (1 << 15) == 1070628864 < 1 << 31


def test_the_limits_are_on_the_quantised_values():
    for slot in range(12):
        lim = 4096.0 if slot % 4 == 3 else 16.0
        for sign in (1, -1):
            ok = list(IDENT); ok[slot] = sign * lim
            assert pjd_amd.colour_check(ok) and M.check(ok)
            assert pjd_amd.colour_value(ok, (200, 100, 50)) == M.value(ok, (200, 100, 50))
            nxt = list(IDENT); nxt[slot] = sign * math.nextafter(lim, 2 * lim)      # quantises to the limit itself
            assert pjd_amd.colour_check(nxt) and M.quantise(nxt) == M.quantise(ok)
            assert pjd_amd.colour_value(nxt, (200, 100, 50)) == pjd_amd.colour_value(ok, (200, 100, 50))
            over = list(IDENT); over[slot] = sign * (lim + 2.0 ** -16)            # the next quantised value
            assert not pjd_amd.colour_check(over) and not M.check(over), (slot, sign)
            with pytest.raises(ValueError):
                pjd_amd.colour_value(over, (1, 2, 3))
        for bad in (float("nan"), float("inf"), float("-inf"), 1e300, -1e300):
            m = list(IDENT); m[slot] = bad
            assert not pjd_amd.colour_check(m) and not M.check(m), (slot, bad)
            with pytest.raises(ValueError):
                pjd_amd.colour_value(m, (0, 0, 0))
    with pytest.raises(ValueError):
        pjd_amd.colour_check(IDENT[:11])
    assert pjd_amd.colour_check([IDENT[0:4], IDENT[4:8], IDENT[8:12]])             # three rows of four


def test_rounding_is_to_nearest_even_and_the_shift_is_arithmetic():
    assert M.quantise([2.0 ** -17, 3 * 2.0 ** -17, -2.0 ** -17, 0] + IDENT[4:])[:3] == [0, 2, 0]
    half_down = [1, 0, 0, -0.5] + IDENT[4:]                 # v - 0.5 + 0.5 rounding: (65536 v - 32768 + 32768) >> 16 = v
    assert pjd_amd.colour_value(half_down, (7, 0, 0))[0] == 7 == M.value(half_down, (7, 0, 0))[0]
    below = [1, 0, 0, -0.5 - 2.0 ** -16] + IDENT[4:]        # one unit below the tie: rounds down
    assert pjd_amd.colour_value(below, (7, 0, 0))[0] == 6 == M.value(below, (7, 0, 0))[0]
    neg = [-1, 0, 0, 0.25] + IDENT[4:]                      # a negative sum: the arithmetic shift floors, then the clamp
    assert pjd_amd.colour_value(neg, (3, 0, 0))[0] == 0 == M.value(neg, (3, 0, 0))[0]


@pytest.fixture(scope="module")
def cube():
    """all 2^24 triples, as three uint8 planes"""
    v = np.arange(1 << 24, dtype=np.uint32)
    c = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255]).astype(np.uint8)
    c.setflags(write=False)
    return c


def test_what_the_header_says_is_exact(cube):
    """the identity and one permutation over all 2^24 triples (the model, vectorised; the library at a seeded sample of them); the other
    permutations, 0/1 selections and integer offsets over a seeded sample"""
    rng = np.random.default_rng(5)
    assert np.array_equal(M.apply(IDENT, cube), cube) and M.is_identity(IDENT)
    bgr = M.permutation((2, 1, 0))
    assert np.array_equal(M.apply(bgr, cube), cube[::-1])
    sample = cube[:, rng.integers(0, 1 << 24, 4000)]
    for rgb in sample.T[:500]:
        rgb = tuple(int(v) for v in rgb)
        assert pjd_amd.colour_value(IDENT, rgb) == rgb and pjd_amd.colour_value(bgr, rgb) == rgb[::-1]
    for order in PERMS:
        m = M.permutation(order)
        got = M.apply(m, sample)
        assert np.array_equal(got, sample[list(order)]), order
        for rgb in sample.T[:40]:
            rgb = tuple(int(v) for v in rgb)
            assert pjd_amd.colour_value(m, rgb) == tuple(rgb[k] for k in order)
    for _ in range(20):                                       # a 0/1 selection (rows may repeat or be empty) and integer offsets
        sel = rng.integers(0, 2, (3, 3))
        off = rng.integers(-300, 300, 3)
        m = [float(v) for c in range(3) for v in (*sel[c], off[c])]
        want = np.clip(sel @ sample.astype(np.int64) + off[:, None], 0, 255)
        assert np.array_equal(M.apply(m, sample), want)
        for rgb, w in list(zip(sample.T, want.T))[:40]:
            assert pjd_amd.colour_value(m, tuple(int(v) for v in rgb)) == tuple(int(v) for v in w)


def test_within_half_a_level_and_2_to_the_minus_7_of_float64():
    rng = np.random.default_rng(77)
    worst = 0.0
    for k in range(200):
        m = seeded_matrix(rng, k)
        px = np.concatenate([np.asarray(CORNERS, np.uint8).T, rng.integers(0, 256, (3, 2000), dtype=np.uint8)], axis=1)
        err = np.abs(M.apply(m, px).astype(np.float64) - M.float64(m, px)).max()
        worst = max(worst, float(err))
        for rgb in px.T[:12]:                                 # the model is the library here too
            assert pjd_amd.colour_value(m, tuple(int(v) for v in rgb)) == M.value(m, rgb)
    print("largest distance to the clamped float64 value:", worst)
    assert worst <= 0.5 + 2.0 ** -7
    assert (3 * 255 + 1) * 2.0 ** -17 < 2.0 ** -7


# ---- tensors.colour_matrix ------------------------------------------------------------------------------------------------------------------
LUMA = np.array([0.299, 0.587, 0.114])
YIQ = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]])


def hom(lin, off=(0, 0, 0)):
    h = np.eye(4)
    h[:3, :3] = lin
    h[:3, 3] = off
    return h


def factor(name, v, pivot=128.0):
    if name == "brightness":
        return hom(v * np.eye(3))
    if name == "contrast":
        return hom(v * np.eye(3), [(1 - v) * pivot] * 3)
    if name == "saturation":
        return hom(v * np.eye(3) + (1 - v) * np.tile(LUMA, (3, 1)))
    a = 2 * np.pi * v
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    return hom(np.linalg.inv(YIQ) @ rot @ YIQ)


def as34(m):
    return np.asarray(m, np.float64).reshape(3, 4)


def test_colour_matrix_defaults_are_the_identity_exactly():
    assert tensors.colour_matrix() == M.IDENTITY == pjd_amd.COLOUR_IDENTITY
    assert M.is_identity(tensors.colour_matrix())


def test_colour_matrix_each_factor_alone():
    for name, v in (("brightness", 1.3), ("brightness", 0.6), ("contrast", 0.7), ("contrast", 1.6), ("saturation", 0.0), ("saturation", 1.5), ("hue", 0.1), ("hue", -0.25), ("hue", 0.5)):
        got = as34(tensors.colour_matrix(**{name: v}))
        assert np.allclose(got, factor(name, v)[:3], rtol=0, atol=1e-12), (name, v)
    assert np.allclose(as34(tensors.colour_matrix(contrast=0.5, pivot=100.0)), factor("contrast", 0.5, 100.0)[:3], rtol=0, atol=1e-12)
    # what each does to a pixel: grey stays grey under saturation and hue, the pivot stays under contrast
    grey = np.array([90.0, 90.0, 90.0, 1.0])
    for kw in (dict(saturation=0.3), dict(hue=0.2), dict(saturation=1.7, hue=-0.4)):
        assert np.allclose(as34(tensors.colour_matrix(**kw)) @ grey, 90.0, atol=1e-9)
    assert np.allclose(as34(tensors.colour_matrix(contrast=0.3)) @ np.array([128.0, 128.0, 128.0, 1.0]), 128.0, atol=1e-12)
    assert np.allclose(as34(tensors.colour_matrix(hue=1.0)), as34(M.IDENTITY), atol=1e-12)      # a whole turn
    sat0 = as34(tensors.colour_matrix(saturation=0.0))
    assert np.allclose(sat0[:, :3], np.tile(LUMA, (3, 1)), atol=1e-15) and np.all(sat0[:, 3] == 0)


def test_colour_matrix_composes_in_the_order_given():
    vals = dict(brightness=1.2, contrast=0.8, saturation=1.4, hue=0.05)
    for order in itertools.permutations(vals):
        want = np.eye(4)
        for name in order:
            want = factor(name, vals[name]) @ want            # applied in order: the later factor on the left
        got = as34(tensors.colour_matrix(order=order, **vals))
        assert np.allclose(got, want[:3], rtol=0, atol=1e-10), order
    a = as34(tensors.colour_matrix(brightness=1.5, contrast=0.5))
    b = as34(tensors.colour_matrix(brightness=1.5, contrast=0.5, order=("contrast", "brightness", "saturation", "hue")))
    assert np.allclose(a[:, 3], 64.0) and np.allclose(b[:, 3], 96.0)                # c(bx) + (1 - c) p against b(cx + (1 - c) p)
    with pytest.raises(ValueError):
        tensors.colour_matrix(order=("brightness", "contrast", "saturation"))
    with pytest.raises(ValueError):
        tensors.colour_matrix(order=("brightness", "contrast", "saturation", "gamma"))
    with pytest.raises(ValueError):
        tensors.colour_matrix(channel_order="grb")
    with pytest.raises(ValueError):
        tensors.colour_matrix(brightness=float("nan"))


def test_colour_matrix_grayscale_and_bgr():
    g = as34(tensors.colour_matrix(grayscale=True))
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[1], g[2]) and abs(g[0, :3].sum() - 1.0) < 1e-15 and g[0, 3] == 0
    assert np.allclose(g[0, :3], LUMA, atol=0)
    j = dict(brightness=1.1, contrast=1.3, saturation=0.6, hue=-0.03)
    gj = as34(tensors.colour_matrix(grayscale=True, **j))
    assert np.allclose(gj[0], gj[1]) and np.allclose(gj[1], gj[2]) and np.allclose(gj[0], LUMA @ as34(tensors.colour_matrix(**j)), atol=1e-12)
    assert np.array_equal(as34(tensors.colour_matrix(channel_order="bgr")), as34(M.permutation((2, 1, 0))))
    rgb, bgr = as34(tensors.colour_matrix(**j)), as34(tensors.colour_matrix(channel_order="bgr", **j))
    assert np.array_equal(bgr, rgb[::-1])
    # a jitter of ColorJitter's usual size is far inside the limits
    assert pjd_amd.colour_check(tensors.colour_matrix(brightness=1.4, contrast=1.4, saturation=1.4, hue=0.1))


# ---- the host tools, under the sanitizers -----------------------------------------------------------------------------------------------------
def host_clang():
    """a clang++ for the host: the store header of the resample uses clang's vector extensions and 16-bit float types"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (shutil.which("clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    return None


def build_and_run(tmp_path, tool, args=(), alignment_check=True, defines=()):
    cxx = host_clang()
    assert cxx, "no clang++ beside hipcc: the compiler that builds the library is needed"
    exe = tmp_path / tool
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined"] + ([] if alignment_check else ["-fno-sanitize=alignment"]) + ["-fno-omit-frame-pointer", "-D__host__=", "-D__device__=", *defines,
           os.path.join(ROOT, "tools", tool + ".cpp"), os.path.join(ROOT, "pim-jpeg-decoder_amd", "csrc", "pjd_resize_plan.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


# the checks of coloured() in tools/resize_plan_host.cpp: identity maps 1; per slot 2 signs x (at the limit 1 + the next double 1 + the next
# quantised value refused 2) + 5 values refused x 2 + the text 1 = 19, x 12; a grey batch 1; the records 1 + 9 + 3 + 1; six shaped members
# x 7 and six unshaped x 9; the fault that names the view 1
COLOURED_PLAN_CHECKS = 1 + 12 * 19 + 1 + 14 + 6 * 7 + 6 * 9 + 1


def test_resolver_rules_for_a_coloured_request_under_asan_ubsan(tmp_path):
    """tools/resize_plan_host.cpp: the limits in every slot, the records, the identity flag, the padded form, the fault that names the view"""
    out = build_and_run(tmp_path, "resize_plan_host")
    assert "no sanitizer report" in out and " 0 checks failed" in out, out[-3000:]
    # the coloured block ran, whole
    m = re.search(r"^coloured: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) == COLOURED_PLAN_CHECKS, out[-3000:]


def test_coloured_resample_bodies_under_asan_ubsan(tmp_path):
    """tools/resize_host.cpp, the coloured set: the three resample bodies with COL over the resolver's records, all element types and layouts"""
    out = build_and_run(tmp_path, "resize_host", alignment_check=False, defines=["-DPJD_HOST_COLOURED_ONLY"])
    assert "ALL EQUAL" in out and "MISMATCH" not in out and out.count("coloured") == 3 * 4 * 8, out[-3000:]


def test_coloured_warp_body_under_asan_ubsan(tmp_path):
    """tools/warp_host.cpp: the warp body with COL, a map per output, and a coloured affine request in the resolver"""
    out = build_and_run(tmp_path, "warp_host", alignment_check=False)
    assert "ALL EQUAL" in out and "no sanitizer report" in out and " 0 checks failed" in out, out[-3000:]
    # the eight coloured forms at four shifts of the buffer each ran and were equal, and the resolver's rules for a coloured affine request
    assert out.count("coloured warp") == 8 * 4 == len(re.findall(r"^coloured warp PLANAR=[01] DT=[0-3] shift=[0-3]: 25 outputs, equal, guards intact$", out, re.M)), out[-3000:]
    assert "coloured affine request: resolver rules checked" in out
