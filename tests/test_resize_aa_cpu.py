"""The antialiased resize on the host (no GPU): pjd_resize_aa_taps -- the inline the batch's weight table is built with -- against
tests/resize_aa_model.py, exhaustively for small axes and on a seeded sample up to 65535; the model itself against the float64
triangle filter (numpy, and torch's antialias=True) on the shapes the arithmetic was validated on; the stripe picture that shows
what the filter is for; the error returns; the keyword defaults of pjd_amd.tensors."""
import ctypes as C
import types

import numpy as np
import pytest

import resize_aa_model as aa
import resize_model

E_ARG = -3
MAX_TAPS = 32
# (sw, sh, tw, th): the shapes include/pjd.h's bound was checked on, the identity last
SHAPES = [(500, 375, 224, 224), (33, 17, 2, 1), (64, 64, 4, 4), (161, 97, 10, 7), (255, 3, 16, 3), (97, 200, 13, 13), (48, 48, 3, 47),
          (13, 11, 30, 20), (1, 1, 5, 5), (37, 29, 37, 29)]


def _lib_taps(sn, dn, i):
    import pjd_amd
    L = pjd_amd.dev_lib()
    first, count, q = C.c_uint32(), C.c_uint32(), (C.c_uint32 * MAX_TAPS)()
    assert L.pjd_resize_aa_taps(sn, dn, i, C.byref(first), C.byref(count), q) == 0, (sn, dn, i)
    return first.value, list(q[:count.value])


def _pictures(sw, sh, seed):
    """A random picture and 0/255 checkerboard noise (every sample an extreme: the worst case for weight errors)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:sh, 0:sw]
    board = (((xx + yy) & 1)[:, :, None] ^ rng.integers(0, 2, (sh, sw, 3))).astype(np.uint8) * 255
    return {"random": rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8), "checkerboard": board}


def test_exports_exist_and_the_abi_version_is_unchanged():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert hasattr(L, "pjd_batch_set_resize_filter") and hasattr(L, "pjd_resize_aa_taps")
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert (pjd_amd.RESIZE_BILINEAR, pjd_amd.RESIZE_ANTIALIAS) == (0, 1)
    assert pjd_amd.AA_MAX_TAPS == MAX_TAPS
    assert callable(pjd_amd.Batch.set_resize_filter) and callable(pjd_amd.resize_aa_taps)


def test_the_two_forms_of_the_model_agree():
    """axis_taps (a window of candidates, vectorised) against taps (every source sample looked at), for every i of every small pair."""
    for sn in range(1, 49):
        for dn in range(1, 49):
            if sn > 16 * dn:
                continue
            first, count, q = aa.axis_taps(sn, dn)
            for i in range(dn):
                f, w = aa.taps(sn, dn, i)
                assert (f, w) == (int(first[i]), [int(v) for v in q[i, :count[i]]]) and not q[i, count[i]:].any(), (sn, dn, i)


def test_taps_equal_the_model_for_every_small_axis():
    """Every i of every pair (sn, dn) with both at most 48 and sn <= 16 * dn: the library's taps are the model's; they sum to 65536,
    lie inside the source, and no sample has more than PJD_AA_MAX_TAPS of them -- a count that is attained."""
    most = 0
    for sn in range(1, 49):
        for dn in range(1, 49):
            if sn > 16 * dn:
                continue
            first, count, q = aa.axis_taps(sn, dn)
            for i in range(dn):
                f, w = _lib_taps(sn, dn, i)
                assert f == first[i] and w == [int(v) for v in q[i, :count[i]]], (sn, dn, i)
                assert sum(w) == 65536 and 0 <= min(w) and max(w) <= 65536 and 1 <= len(w) <= MAX_TAPS and f + len(w) <= sn, (sn, dn, i)
                most = max(most, len(w))
    assert most == MAX_TAPS                                 # attained at exactly 16x: 16 -> 1, 32 -> 2, 48 -> 3, and
    assert max(len(_lib_taps(64, 4, i)[1]) for i in range(4)) == MAX_TAPS
    assert int(aa.axis_taps(64, 4)[1].max()) == MAX_TAPS
    assert _lib_taps(7, 7, 3) == (3, [65536])               # a single tap needs 17 bits


def test_taps_equal_the_model_on_large_axes():
    """A seeded sample of pairs up to 65535 (the 64-bit range: (2i + 1) * sn reaches 2^33), the named ones first; per pair the first
    and last samples and a seeded sample between."""
    rng = np.random.default_rng(21)
    pairs = [(65535, 65535), (65535, 40000), (65535, 4096), (8, 65535)]
    while len(pairs) < 40:
        dn = int(rng.integers(1, 65536))
        sn = int(rng.integers(1, min(65535, 16 * dn) + 1))
        pairs.append((sn, dn))
    most = 0
    for sn, dn in pairs:
        first, count, q = aa.axis_taps(sn, dn)
        assert np.all(q.sum(axis=1) == 65536) and q.min() >= 0 and np.all(first + count <= sn) and count.max() <= MAX_TAPS, (sn, dn)
        most = max(most, int(count.max()))
        idx = sorted({0, 1, dn // 2, dn - 2, dn - 1} & set(range(dn)) | {int(v) for v in rng.integers(0, dn, 60)})
        for i in idx:
            f, w = _lib_taps(sn, dn, i)
            assert f == first[i] and w == [int(v) for v in q[i, :count[i]]], (sn, dn, i)
    assert most == MAX_TAPS                                 # 65535 -> 4096 (just under 16x)


def test_aa_taps_error_returns():
    import pjd_amd
    L = pjd_amd.dev_lib()
    first, count, q = C.c_uint32(7), C.c_uint32(7), (C.c_uint32 * MAX_TAPS)()
    args = (C.byref(first), C.byref(count), q)
    for sn, dn, i in ((0, 4, 0), (4, 0, 0), (65536, 65535, 0), (4, 65536, 0), (4, 4, 4), (4, 4, 2 ** 32 - 1), (65, 4, 0), (17, 1, 0),
                      (65535, 4095, 0)):
        assert L.pjd_resize_aa_taps(sn, dn, i, *args) == E_ARG, (sn, dn, i)
    assert (first.value, count.value) == (7, 7)
    assert L.pjd_resize_aa_taps(64, 4, 0, *args) == 0 and L.pjd_resize_aa_taps(16, 1, 0, *args) == 0      # exactly 16x is inside
    assert L.pjd_resize_aa_taps(64, 4, 1, None, None, None) == 0                                            # each output may be NULL
    with pytest.raises(ValueError):
        pjd_amd.resize_aa_taps(65, 4, 0)
    assert pjd_amd.resize_aa_taps(5, 5, 2) == (2, [65536])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_model_is_within_one_level_of_the_float64_filter(shape):
    """The integer model against the float64 triangle filter rounded to nearest, computed in numpy and by torch on the CPU: at most 1
    level apart (include/pjd.h, ERROR BOUND: under 0.252 + 0.5 from the exact value); the two float64 filters agree to 1e-9."""
    torch = pytest.importorskip("torch")
    sw, sh, tw, th = shape
    for name, P in _pictures(sw, sh, seed=sw * 131 + tw).items():
        got = aa.resize(P, tw, th).astype(np.int64)
        exact = aa.triangle_f64(P, tw, th)
        x = torch.from_numpy(P.astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.interpolate(x, size=(th, tw), mode="bilinear", align_corners=False, antialias=True)[0].permute(1, 2, 0).numpy()
        assert np.abs(exact - ref).max() < 1e-9, (shape, name)
        # the model rounds the value it has once: it may differ from the exact value by the bound plus that rounding
        print(f"{shape} {name}: |model - float64| max {np.abs(got - exact).max():.4f}")
        assert np.abs(got - exact).max() < 0.252 + 0.5 + 1e-9, (shape, name)
        assert np.abs(got - np.rint(exact).astype(np.int64)).max() <= 1, (shape, name)
        assert np.abs(got - np.rint(ref).astype(np.int64)).max() <= 1, (shape, name)


def test_identity_and_constant_pictures_are_byte_exact():
    rng = np.random.default_rng(4)
    for sw, sh in ((37, 29), (1, 1), (64, 3)):
        P = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        assert np.array_equal(aa.resize(P, sw, sh), P)
    for sw, sh, tw, th in SHAPES:
        for level in (0, 1, 127, 254, 255):
            P = np.full((sh, sw, 3), level, np.uint8)
            assert np.all(aa.resize(P, tw, th) == level), (sw, sh, tw, th, level)


def test_stripes_shrunk_4x_are_flat_antialiased_and_not_bilinear():
    """The point of the feature: stripes of period 4 (0, 0, 255, 255), each row one pixel further along than the row above, shrunk 4x
    along the rows.  A widened triangle covers two whole periods, whatever the phase: every row comes out as the mean, 127.5 -- 127 or
    128, flat to within 1 level (but for the first and the last column, where the clipped filter is renormalised and leans to one
    side).  Plain bilinear reads the two samples around each centre and returns the phase it lands on: black rows, grey rows, white
    rows."""
    sw, sh = 256, 32
    yy, xx = np.mgrid[0:sh, 0:sw]
    P = np.repeat((((xx + yy) % 4 >= 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    flat = aa.resize(P, sw // 4, sh)[:, 1:-1].astype(int)
    assert flat.min() >= 127 and flat.max() <= 128, (flat.min(), flat.max())
    plain = resize_model.resize(P, sw // 4, sh)[:, 1:-1].astype(int)
    assert plain.min() == 0 and plain.max() == 255
    assert sorted(set(plain[:4, 5, 0])) == [0, 127, 255] or sorted(set(plain[:4, 5, 0])) == [0, 128, 255], plain[:4, 5, 0]


class _Recorder:
    """Stands in for a Batch: records the calls pjd_amd.tensors._run makes."""
    def __init__(self, n, log):
        self.n, self.log = n, log

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def call(*a, **k):
            self.log.append((name,) + a)
            return {"packed_size": 0, "statuses": [0] * self.n, "output_offset": 0}.get(name)
        return call


def test_tensor_helpers_set_the_filter_only_when_asked(monkeypatch):
    """antialias defaults to False in both helpers, and then Batch.set_resize_filter is not called at all; with antialias=True it is
    called once, with RESIZE_ANTIALIAS, after set_resize and before set_normalize and bind_output."""
    torch = pytest.importorskip("torch")
    import inspect
    import pjd_amd
    from pjd_amd import tensors
    for fn in (tensors.decode_resized_batch_tensor, tensors.decode_normalized_batch_tensor):
        assert inspect.signature(fn).parameters["antialias"].default is False
        assert "prescale=False" in fn.__doc__ and "16x" in fn.__doc__
    fake = types.SimpleNamespace(device=lambda *a: "cpu", float16=torch.float16, bfloat16=torch.bfloat16, float32=torch.float32, uint8=torch.uint8,
                                 empty=lambda n, dtype, device: torch.empty(n, dtype=dtype),
                                 cuda=types.SimpleNamespace(current_stream=lambda d: types.SimpleNamespace(synchronize=lambda: None)))
    monkeypatch.setattr(tensors, "_torch", lambda: fake)
    descs = [pjd_amd.ImageDesc() for _ in range(2)]
    for d in descs:
        d.width, d.height = 40, 30
    for kw, want in (({}, 0), ({"antialias": False}, 0), ({"antialias": True}, 1)):
        for normalized in (False, True):
            log = []
            ctx = types.SimpleNamespace(device=0, batch=lambda ds, fmt: _Recorder(len(ds), log))
            if normalized:
                t, st = tensors.decode_normalized_batch_tensor(ctx, descs, (8, 8), (0.5, 0.5, 0.5), (0.2, 0.2, 0.2), **kw)
            else:
                t, st = tensors.decode_resized_batch_tensor(ctx, descs, (8, 8), **kw)
            assert tuple(t.shape) == (2, 3, 8, 8) and st == [0, 0]
            names = [c[0] for c in log]
            assert names.count("set_resize_filter") == want, (kw, normalized, names)
            if want:
                assert ("set_resize_filter", pjd_amd.RESIZE_ANTIALIAS) in log
                k = names.index("set_resize_filter")
                assert names.index("set_resize") < k < names.index("bind_output")
                if normalized:
                    assert k < names.index("set_normalize")
