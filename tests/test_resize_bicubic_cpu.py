"""The bicubic resize on the host (no GPU): pjd_resize_bicubic_taps -- the inline the batch's weight table is built with -- against
tests/resize_bicubic_model.py, exhaustively for small axes and on a seeded sample up to 65535; the gain sum |q_j| that keeps the
kernel's accumulators in 32 bits; the model itself against the float64 filter (numpy, and torch's mode="bicubic" with
antialias=True), with the one clamp driven at both ends; Pillow's BICUBIC where its 8-bit intermediate does not clip; the error
returns; the `interpolation` keyword of pjd_amd.tensors.

Figures this file measures (python -m pytest tests/test_resize_bicubic_cpu.py -s prints them):
  largest gain A = sum |q_j|            83152 (1.2688), the axis 14 -> 13 at i = 6; the refusal of pjd_batch_set_resize_filter is at 92681
  largest |model - float64| before the final rounding    0.0276 levels (bound of include/pjd.h: 0.716)
  Pillow BICUBIC against the float64 filter, smooth picture   at most 1 level; random 0/255 picture 161x97 -> 150x90: 30.5 levels (its 8-bit intermediate is clipped)"""
import ctypes as C
import types

import numpy as np
import pytest

import resize_bicubic_model as bc
from test_resize_aa_cpu import SHAPES as AA_SHAPES, _Recorder, _pictures

E_ARG = -3
MAX_TAPS = 64
MAX_GAIN = 92681
# the shapes of the triangle filter's test, an upscale on both axes, a mixed one
SHAPES = AA_SHAPES + [(9, 7, 31, 25), (40, 6, 7, 19)]
BOUND = (2 * 255 * 64 / 65536 + 1 / 128) * MAX_GAIN / 65536      # include/pjd.h, ERROR BOUND: 0.716 levels before the final rounding


def _lib():
    import pjd_amd
    return pjd_amd.dev_lib()


def _lib_taps(sn, dn, i, L=None, buf=(C.c_uint32(), C.c_uint32(), (C.c_int32 * MAX_TAPS)())):
    first, count, q = buf
    assert (L or _lib()).pjd_resize_bicubic_taps(sn, dn, i, C.byref(first), C.byref(count), q) == 0, (sn, dn, i)
    return first.value, list(q[:count.value])


def test_exports_exist_and_the_abi_version_is_unchanged():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert hasattr(L, "pjd_resize_bicubic_taps")
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert (pjd_amd.RESIZE_BILINEAR, pjd_amd.RESIZE_ANTIALIAS, pjd_amd.RESIZE_BICUBIC) == (0, 1, 3)
    assert pjd_amd.BICUBIC_MAX_TAPS == MAX_TAPS == bc.MAX_TAPS and pjd_amd.BICUBIC_MAX_GAIN == MAX_GAIN == bc.MAX_GAIN
    assert callable(pjd_amd.resize_bicubic_taps)


def test_taps_equal_the_model_for_every_small_axis():
    """Every i of every pair (sn, dn) with both at most 64 and sn <= 16 * dn: the library's taps are the model's; they sum to 65536
    exactly, lie inside the source, and no sample has more than ceil(4 * S / dn) of them."""
    L = _lib()
    for sn in range(1, 65):
        for dn in range(1, 65):
            if sn > 16 * dn:
                continue
            for i in range(dn):
                f, w = _lib_taps(sn, dn, i, L)
                assert (f, w) == bc.taps(sn, dn, i), (sn, dn, i)
                assert sum(w) == 65536 and 1 <= len(w) <= min(MAX_TAPS, -(-4 * max(sn, dn) // dn)) and f + len(w) <= sn, (sn, dn, i)
                assert max(abs(v) for v in w) < 1 << 18


def test_the_tap_limit_is_attained_and_zero_weights_stay_inside_the_run():
    """96 -> 6 (exactly 16x) at i = 3: 64 taps, the most the limit admits.  Same size: (0, 65536, 0) -- the run is the support, not
    the samples with a weight."""
    f, w = _lib_taps(96, 6, 3)
    assert (f, len(w)) == (24, MAX_TAPS) and (f, w) == bc.taps(96, 6, 3)
    assert max(len(_lib_taps(96, 6, i)[1]) for i in range(6)) == MAX_TAPS
    assert _lib_taps(7, 7, 3) == (2, [0, 65536, 0]) and _lib_taps(7, 7, 0) == (0, [65536, 0]) and _lib_taps(7, 7, 6) == (5, [0, 65536])
    assert _lib_taps(1, 1, 0) == (0, [65536])
    import pjd_amd
    assert pjd_amd.resize_bicubic_taps(5, 5, 2) == (1, [0, 65536, 0])
    f, w = pjd_amd.resize_bicubic_taps(30, 90, 44)         # an upscale, between two samples: four taps, the outer two negative
    assert len(w) == 4 and w[0] < 0 < w[1] and w[3] < 0 < w[2] and sum(w) == 65536


def test_taps_equal_the_model_on_large_axes():
    """A seeded sample of pairs up to 65535 (r_j * 2^17 passes 64 bits: the 128-bit quantisation), the named ones first -- 65535 ->
    4096 has 64 taps --; per pair the first and last samples and a seeded sample between."""
    rng = np.random.default_rng(22)
    L = _lib()
    pairs = [(65535, 65535), (65535, 40000), (65535, 4096), (8, 65535), (65535, 65534), (65520, 4095)]
    while len(pairs) < 40:
        dn = int(rng.integers(1, 65536))
        pairs.append((int(rng.integers(1, min(65535, 16 * dn) + 1)), dn))
    most = 0
    for sn, dn in pairs:
        idx = sorted({0, 1, dn // 2, dn - 2, dn - 1} & set(range(dn)) | {int(v) for v in rng.integers(0, dn, 40)})
        for i in idx:
            f, w = _lib_taps(sn, dn, i, L)
            assert (f, w) == bc.taps(sn, dn, i), (sn, dn, i)
            assert sum(w) == 65536 and len(w) <= MAX_TAPS and f + len(w) <= sn
            most = max(most, len(w))
    assert most == MAX_TAPS


def test_the_gain_stays_below_the_refusal():
    """A = sum |q_j| of every target sample of every admitted axis with sn, dn < 130, and of 200 000 seeded samples (sn, dn, i) up to
    65535: never above PJD_BICUBIC_MAX_GAIN, the value above which pjd_batch_set_resize_filter refuses an axis (the kernel's 32-bit
    accumulators hold up to it: include/pjd.h, RANGE).  The largest A seen is recorded."""
    L = _lib()
    buf = (C.c_uint32(), C.c_uint32(), (C.c_int32 * MAX_TAPS)())
    best = (0, 0, 0, 0)
    for dn in range(1, 130):
        for sn in range(1, min(129, 16 * dn) + 1):
            for i in range(dn):
                _, w = _lib_taps(sn, dn, i, L, buf)
                a = sum(abs(v) for v in w)
                best = (a, sn, dn, i) if a > best[0] else best     # the first axis that attains it
    rng = np.random.default_rng(23)
    dns = rng.integers(1, 65536, 200000)
    sns = (rng.random(200000) * np.minimum(65535, 16 * dns)).astype(np.int64) + 1
    idx = (rng.random(200000) * dns).astype(np.int64)
    sampled = (0, 0, 0, 0)
    for sn, dn, i in zip(sns.tolist(), dns.tolist(), idx.tolist()):
        _, w = _lib_taps(sn, dn, i, L, buf)
        sampled = max(sampled, (sum(abs(v) for v in w), sn, dn, i))
    print(f"largest gain: exhaustive {best[0]} ({best[0] / 65536:.4f}) at {best[1]} -> {best[2]}, i = {best[3]}; "
          f"sampled {sampled[0]} at {sampled[1]} -> {sampled[2]}, i = {sampled[3]}")
    assert sampled[0] <= best[0] <= MAX_GAIN
    assert best[0] == bc.gain(best[1], best[2])             # the model sees the same axis the same way
    # the bounds of the header's RANGE paragraph, from the refusal's value alone
    h6 = (255 * MAX_GAIN + 512) >> 10
    assert h6 == 23080 and MAX_GAIN * h6 + (1 << 21) < 1 << 31


def test_identity_and_constant_pictures_are_byte_exact():
    rng = np.random.default_rng(4)
    for sw, sh in ((37, 29), (1, 1), (64, 3)):
        P = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        assert np.array_equal(bc.resize(P, sw, sh), P)
    for sw, sh, tw, th in SHAPES:
        for level in (0, 1, 127, 254, 255):
            P = np.full((sh, sw, 3), level, np.uint8)
            assert np.all(bc.resize(P, tw, th) == level), (sw, sh, tw, th, level)


def test_model_is_within_one_level_of_the_float64_filter():
    """The integer model against the separable float64 filter clamped ONCE at the end and rounded to nearest, computed in numpy and by
    torch on the CPU (mode="bicubic", antialias=True: Keys' a = -0.5): at most 1 level apart; before its final rounding the model is
    within the header's bound of the exact value; the two float64 filters agree to 1e-9.  The 0/255 checkerboards overshoot on both
    sides: the one clamp is met at 0 and at 255."""
    torch = pytest.importorskip("torch")
    stats, worst = {}, 0.0
    for shape in SHAPES:
        sw, sh, tw, th = shape
        for name, P in _pictures(sw, sh, seed=sw * 131 + tw).items():
            st = stats if name == "checkerboard" else {}
            got = bc.resize(P, tw, th, st).astype(np.int64)
            exact = bc.cubic_f64(P, tw, th)
            x = torch.from_numpy(P.astype(np.float64)).permute(2, 0, 1)[None]
            ref = torch.nn.functional.interpolate(x, size=(th, tw), mode="bicubic", align_corners=False, antialias=True)[0].permute(1, 2, 0).numpy()
            assert np.abs(exact - ref).max() < 1e-9, (shape, name)
            err = float(np.abs(st["pre"] - exact).max())
            worst = max(worst, err)
            print(f"{shape} {name}: |model - float64| before the rounding, max {err:.4f}")
            assert err < BOUND, (shape, name)
            for f64 in (exact, ref):
                assert np.abs(got - np.rint(np.clip(f64, 0, 255)).astype(np.int64)).max() <= 1, (shape, name)
    print(f"largest |model - float64| before the final rounding: {worst:.4f} levels (bound {BOUND:.4f}); "
          f"clamped below 0: {stats['below']} samples, above 255: {stats['above']}")
    assert BOUND < 1 and stats["below"] > 0 and stats["above"] > 0


def _smooth(sw, sh):
    yy, xx = np.mgrid[0:sh, 0:sw].astype(np.float64)
    img = np.stack([127 + 90 * np.sin(xx / 9.0) * np.cos(yy / 13.0), 127 + 80 * np.cos(yy / 17.0 + xx / 31.0), 20 + (xx + yy) * 215 / (sw + sh)], -1)
    return np.rint(img).astype(np.uint8)


def test_pillow_bicubic_agrees_where_its_8_bit_intermediate_does_not_clip():
    """Pillow's BICUBIC is this filter, but its uint8 path rounds and CLIPS the horizontal pass to 8 bits.  On a smooth picture whose
    float64 horizontal pass stays inside 0..255 (asserted) the model is within 1 level of Pillow; on a random 0/255 picture, where
    that pass overshoots, Pillow leaves the float64 filter by tens of levels -- recorded, a property of its 8-bit intermediate."""
    Image = pytest.importorskip("PIL.Image")
    for sw, sh, tw, th in ((500, 375, 224, 224), (161, 97, 10, 7), (97, 200, 13, 13), (40, 30, 96, 64)):
        P = _smooth(sw, sh)
        hz = bc.horizontal_f64(P, tw)
        assert hz.min() >= 0.5 and hz.max() <= 254.5, "the horizontal pass stays inside 0..255 with room for its rounding"
        pil = np.asarray(Image.fromarray(P, "RGB").resize((tw, th), Image.BICUBIC)).astype(np.int64)
        got = bc.resize(P, tw, th).astype(np.int64)
        assert np.abs(got - pil).max() <= 1, (sw, sh, tw, th)
    rng = np.random.default_rng(9)
    P = rng.integers(0, 2, (97, 161, 3)).astype(np.uint8) * 255
    hz = bc.horizontal_f64(P, 150)
    assert hz.min() < 0 and hz.max() > 255
    pil = np.asarray(Image.fromarray(P, "RGB").resize((150, 90), Image.BICUBIC)).astype(np.int64)
    exact = np.clip(bc.cubic_f64(P, 150, 90), 0, 255)
    print(f"random 0/255 picture 161x97 -> 150x90: |Pillow - float64| max {np.abs(pil - exact).max():.1f} levels, "
          f"|model - float64| max {np.abs(bc.resize(P, 150, 90) - exact).max():.2f}")
    assert np.abs(bc.resize(P, 150, 90).astype(np.int64) - np.rint(exact)).max() <= 1
    assert np.abs(pil - exact).max() > 1.5                  # the clipped intermediate is visible: Pillow is not the yardstick there


def test_bicubic_taps_error_returns():
    import pjd_amd
    L = pjd_amd.dev_lib()
    first, count, q = C.c_uint32(7), C.c_uint32(7), (C.c_int32 * MAX_TAPS)()
    args = (C.byref(first), C.byref(count), q)
    for sn, dn, i in ((0, 4, 0), (4, 0, 0), (65536, 65535, 0), (4, 65536, 0), (4, 4, 4), (4, 4, 2 ** 32 - 1), (65, 4, 0), (17, 1, 0),
                      (65535, 4095, 0)):
        assert L.pjd_resize_bicubic_taps(sn, dn, i, *args) == E_ARG, (sn, dn, i)
    assert (first.value, count.value) == (7, 7)
    assert L.pjd_resize_bicubic_taps(64, 4, 0, *args) == 0 and L.pjd_resize_bicubic_taps(16, 1, 0, *args) == 0      # exactly 16x is inside
    assert L.pjd_resize_bicubic_taps(64, 4, 1, None, None, None) == 0                                                # each output may be NULL
    with pytest.raises(ValueError):
        pjd_amd.resize_bicubic_taps(65, 4, 0)


def test_window_check_applies_the_16x_rule_to_the_bicubic_filter():
    import pjd_amd
    BC, BL = pjd_amd.RESIZE_BICUBIC, pjd_amd.RESIZE_BILINEAR
    assert pjd_amd.resize_window_check(200, 120, 4, 4, (100, 40, 64, 64), BC)           # exactly 16x
    assert not pjd_amd.resize_window_check(200, 120, 4, 4, (100, 40, 65, 64), BC)       # past it along x
    assert not pjd_amd.resize_window_check(200, 120, 4, 4, (100, 40, 64, 65), BC)       # along y
    assert pjd_amd.resize_window_check(200, 120, 4, 4, (100, 40, 65, 64), BL)           # the bilinear filter has no such limit
    assert pjd_amd.resize_window_check(200, 120, 4, 4, (100, 40, 65, 65, 5, 5), BC)     # the limit is against the VIRTUAL target
    assert not pjd_amd.resize_window_check(200, 120, 4, 4, None, BC)                    # no window: the whole picture, 50x along x
    assert pjd_amd.resize_window_check(64, 64, 4, 4, None, BC)
    assert not pjd_amd.resize_window_check(64, 64, 4, 4, (0, 0, 65, 64), BC)            # the other rules hold as before
    assert not pjd_amd.resize_window_check(64, 64, 4, 4, None, 2) and not pjd_amd.resize_window_check(64, 64, 4, 4, None, 4) and not pjd_amd.resize_window_check(64, 64, 4, 4, None, -1)


def test_tensor_helpers_set_the_filter_only_when_asked(monkeypatch):
    """interpolation defaults to "bilinear" in both helpers, and then the calls are what they were (set_resize_filter only with
    antialias=True, with RESIZE_ANTIALIAS); "bicubic" sets RESIZE_BICUBIC once, after set_resize and before set_normalize and
    bind_output, whatever antialias says; any other string raises ValueError before a batch is created."""
    torch = pytest.importorskip("torch")
    import inspect
    import pjd_amd
    from pjd_amd import tensors
    for fn in (tensors.decode_resized_batch_tensor, tensors.decode_normalized_batch_tensor):
        assert inspect.signature(fn).parameters["interpolation"].default == "bilinear"
        assert "bicubic" in fn.__doc__ and "prescale=True" in fn.__doc__ and "prescale=False" in fn.__doc__ and "16x" in fn.__doc__
    fake = types.SimpleNamespace(device=lambda *a: "cpu", float16=torch.float16, bfloat16=torch.bfloat16, float32=torch.float32, uint8=torch.uint8,
                                 empty=lambda n, dtype, device: torch.empty(n, dtype=dtype),
                                 cuda=types.SimpleNamespace(current_stream=lambda d: types.SimpleNamespace(synchronize=lambda: None)))
    monkeypatch.setattr(tensors, "_torch", lambda: fake)
    descs = [pjd_amd.ImageDesc() for _ in range(2)]
    for d in descs:
        d.width, d.height = 40, 30
    AA, BC = pjd_amd.RESIZE_ANTIALIAS, pjd_amd.RESIZE_BICUBIC
    for kw, want in (({}, None), ({"interpolation": "bilinear"}, None), ({"interpolation": "bilinear", "antialias": True}, AA),
                     ({"interpolation": "bicubic"}, BC), ({"interpolation": "bicubic", "antialias": True}, BC),
                     ({"interpolation": "bicubic", "antialias": False, "prescale": False}, BC)):
        for normalized in (False, True):
            log = []
            ctx = types.SimpleNamespace(device=0, batch=lambda ds, fmt: _Recorder(len(ds), log))
            if normalized:
                t, st = tensors.decode_normalized_batch_tensor(ctx, descs, (8, 8), (0.5, 0.5, 0.5), (0.2, 0.2, 0.2), **kw)
            else:
                t, st = tensors.decode_resized_batch_tensor(ctx, descs, (8, 8), **kw)
            assert tuple(t.shape) == (2, 3, 8, 8) and st == [0, 0]
            names = [c[0] for c in log]
            assert names.count("set_resize_filter") == (want is not None), (kw, normalized, names)
            if want is not None:
                assert ("set_resize_filter", want) in log
                k = names.index("set_resize_filter")
                assert names.index("set_resize") < k < names.index("bind_output")
                if normalized:
                    assert k < names.index("set_normalize")
    created = []
    ctx = types.SimpleNamespace(device=0, batch=lambda ds, fmt: created.append(1) or _Recorder(len(ds), []))
    for bad in ("nearest", "BICUBIC", "", None, 2):
        with pytest.raises(ValueError):
            tensors.decode_resized_batch_tensor(ctx, descs, (8, 8), interpolation=bad)
        with pytest.raises(ValueError):
            tensors.decode_normalized_batch_tensor(ctx, descs, (8, 8), (0.5, 0.5, 0.5), (0.2, 0.2, 0.2), interpolation=bad)
    assert not created
