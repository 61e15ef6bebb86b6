"""The exact-kernel fallback of pjd_batch_sync on every back end, scale and sampling (run with -m gpu on an MI355X).

settle() (csrc/pjd_api.hip) is the one place where pictures are decoded by launch lists the planner did not build: it copies the flagged
pictures' ranges, renumbers them into a scratch of its own, sorts them into three lists (default arithmetic, PJD_F_LIBJPEG at full size,
PJD_F_LIBJPEG_SCALE_*), runs the dense kernels, the colour launch and the whole resample again -- and the lane back end has skipped every
such picture, so whatever settle() forgets is stale or poisoned memory in the caller's picture.  The streams of tests/fallback_corpus.py
are known to fall back (their routes are asserted first); every test opens a context of its own under PJD_DEBUG_POISON=0xa5 with 128-byte
lanes, decodes every batch twice from one upload, captures it and replays it, and asserts n_sequential, n_fallback, the status words,
exact_fallback_ms > 0 iff something fell back, and that the defensive flags stay 0.

Nothing expected is something this library delivered: the oracle port's status and picture (default arithmetic), the box filter of
tests/test_gpu_scaled.py over it (PJD_F_SCALE_*), tests/gray_expected.py's planes (grey output), tests/libjpeg_corpus.py's model over the
port's coefficients (PJD_F_LIBJPEG), tests/libjpeg_scaled_model.py over the same coefficients (PJD_F_LIBJPEG_SCALE_*), Pillow's recording
(the one progressive picture) and tests/resize_pad_model.py over those pictures (the resample).  The cases that need caller-owned device
memory -- the mixed batch and the shards, bound at base + 1 into a tensor of 0xA5 -- run in child processes:
tests/fallback_torch_cases.py."""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fallback_corpus as F
import gray_expected as G
import libjpeg_corpus as LC
import libjpeg_model as M
import libjpeg_scaled_model as SM
import nosync_corpus as N
import normalize_model as nm
import resize_pad_model as pm
from conftest import golden_bytes
from test_gpu_libjpeg_corpus import GOOD_BESIDE
from test_gpu_libjpeg_scaled import fmt_of, same
from test_gpu_nosync import REASONS, ROUTES, no_defensive_flag, route
from test_gpu_scaled import box
from test_libjpeg_scaled_cpu import jpeg as ls_jpeg, recording

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LJ, FORCE = 64, 2                                        # PJD_F_LIBJPEG, PJD_F_FORCE_SEQUENTIAL
BOX = {1: 0, 2: 16, 4: 32, 8: 48}                        # PJD_F_SCALE_*
LJS = {1: 0, 2: 128, 4: 256, 8: 384}                     # PJD_F_LIBJPEG_SCALE_*
SCAN_PROGRESSIVE = 1
PROGRESSIVE = "ls_33x31_420_q90_prog"
ERR_FIXTURE = "err_corrupt_3"
ENV = {"PJD_SUB_BYTES": "128", "PJD_DEBUG_POISON": "0xa5"}
ENV_OFF = ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_FORCE_SEQUENTIAL")
# Routes of the new class-1 streams (128-byte lanes, alone in a batch), recorded on the device and explained in DESIGN.md 4.2:
# name -> flagged waves by reason; the number of stale waves (STITCH) also follows from the stream's wave count, see test_routes.
ROUTES_NEW = {"lock_422_288": {"STITCH": 3, "SEGMENT": 2}, "lock_444_384": {"STITCH": 4, "SEGMENT": 3}, "lock_440_288": {"STITCH": 3, "SEGMENT": 2}}
TRUE_GEN0 = {"grey": True, "420": False, "422": True, "444": False, "440": True}


# ---- expectations: computed once per process, never changed --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _port():
    import oracle_lib
    return oracle_lib.Port()


@functools.lru_cache(maxsize=None)
def _oracle(data):
    o = _port().decode(data)
    assert o["valid"]
    o["rgb"].setflags(write=False)
    return o["huff_rc"], o["rgb"]


@functools.lru_cache(maxsize=None)
def _oracle_plane(data):
    st, plane = G.ref_plane(_port(), data)
    plane.setflags(write=False)
    return st, plane


@functools.lru_cache(maxsize=None)
def _lj_coefficients(data):
    return LC.port_coefficients(_port(), data)


@functools.lru_cache(maxsize=None)
def want(data, lj=False, s=1, gray=False):
    """(status, picture) of a descriptor of `data`: H x W x 3, or the H x W plane of a grey batch, at its output scale."""
    if not lj:
        if gray:
            st, plane = _oracle_plane(data)
            out = G.box1(plane, s)
        else:
            st, rgb = _oracle(data)
            out = box(rgb, s)
    else:
        st, coef, (qts, w, h, ncomp, hs, vs) = _lj_coefficients(data)
        if s == 1 and not gray:
            out = LC.decode(coef, qts, w, h, ncomp, hs, vs)
        elif s == 1:
            y = LC.unit_grids(coef, w, h, ncomp, hs, vs)[0]
            out = np.ascontiguousarray(M.plane_from_units(M.idct_units(y, np.asarray(qts[0]).reshape(64)))[:h, :w])
        else:
            out = SM.decode(coef, qts, w, h, ncomp, hs, vs, s, gray)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return st, out


Item = collections.namedtuple("Item", "label data lj s extra options given")


def item(label, data, lj=False, s=1, extra=0, options=0, given=None):
    """One picture of a batch.  given: {gray: (status, picture)} where the expectation is a recording, not a model."""
    return Item(label, data, lj, s, extra, options, given)


def expected(it, gray):
    if it.given is not None:
        return it.given[gray]
    return want(it.data, it.lj, it.s, gray)


def scan(it):
    import pjd_amd
    sc = pjd_amd.Scanned(it.data, options=it.options)
    assert sc.valid, (it.label, sc.log)
    sc.desc.flags = int(sc.desc.flags) | ((LJ | LJS[it.s]) if it.lj else BOX[it.s]) | it.extra
    return sc


def is_sequential(it):
    return bool(it.extra & FORCE) or bool(it.options & SCAN_PROGRESSIVE)


def good(k, lj=False, s=1, extra=0):
    n = GOOD_BESIDE[k % len(GOOD_BESIDE)]
    return item(f"good:{n}", LC.jpeg(n), lj, s, extra)


def falling(name, lj=False, s=1):
    return item(name, F.falling()[name].data, lj, s)


def source(it, gray):
    """The decoded picture the resample reads, as H x W x 3."""
    p = expected(it, gray)[1]
    return np.repeat(p[:, :, None], 3, axis=2) if gray else p


# ---- one batch: decoded twice from one upload, captured and replayed -------------------------------------------------------------------------
def u8_compare(fmt):
    return lambda got, wanted, label: same(got, wanted, fmt, label)


def run_batch(ctx, items, fmt, statuses, wants, n_fallback, prepare=None, compare=None):
    """items -> the batch; wants: one array per output.  Every decode is checked against the expectations, and the three give the same
    bytes.  -> the last info."""
    compare = compare or u8_compare(fmt)
    sc = [scan(it) for it in items]
    n_seq = sum(is_sequential(it) for it in items)
    with ctx.batch([x.desc for x in sc], fmt_of(fmt)) as b:
        if prepare:
            prepare(b)
        b.upload()
        seen = []
        for what in ("first", "second", "replay"):
            if what == "replay":
                b.capture()
            b.decode(); b.sync()
            outs, st = b.download()
            info = b.info()
            assert list(st) == list(statuses), (what, [(it.label, a, w) for it, a, w in zip(items, st, statuses) if a != w])
            assert len(outs) == len(wants)
            for k, (o, w) in enumerate(zip(outs, wants)):
                compare(o, w, (what, k, items[k].label if len(wants) == len(items) else "view"))
            assert (info["n_sequential"], info["n_fallback"]) == (n_seq, n_fallback), (what, info)
            assert (info["exact_fallback_ms"] > 0) == (n_fallback > 0), (what, info["exact_fallback_ms"])
            assert info["sub_bytes"] == 128
            no_defensive_flag(info, what)
            seen.append(([np.asarray(o).tobytes() for o in outs], list(st)))
        assert seen[0] == seen[1] == seen[2]
    return info


def run_items(ctx, items, fmt, alone):
    gray = fmt == "gray"
    exp = [expected(it, gray) for it in items]
    n_fb = sum(alone[it.label] for it in items if it.label in alone and not is_sequential(it))
    return run_batch(ctx, items, fmt, [e[0] for e in exp], [e[1] for e in exp], n_fb)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
def _set_env(mp):
    for k, v in ENV.items():
        mp.setenv(k, v)
    for k in ENV_OFF:
        mp.delenv(k, raising=False)


@pytest.fixture
def fctx(monkeypatch):
    """A fresh context whose allocations start as 0xA5, cut into 128-byte lanes, with the planner's own walker threshold."""
    import pjd_amd
    _set_env(monkeypatch)
    c = pjd_amd.Context(0)
    yield c
    c.close()


def singles():
    """Every stream that some batch below counts on: label -> item (default arithmetic, full size)."""
    out = [falling(n) for n in F.falling()]
    out += [item(f"broken{k}", j) for k, j in enumerate(F.broken())]
    out += [item(n, N.streams()[n].data) for n in ("err_behind_flag", "err_first_wave")]
    return out


@pytest.fixture(scope="module")
def routes():
    """{label: route} of every such stream decoded ALONE in a batch: the route is the device's to tell."""
    import pjd_amd
    with pytest.MonkeyPatch.context() as mp:
        _set_env(mp)
        ctx = pjd_amd.Context(0)
        try:
            out = {}
            for it in singles():
                st, rgb = expected(it, False)
                info = run_batch(ctx, [it], "rgb8", [st], [rgb], n_fallback=_peek_fallback(ctx, it))
                out[it.label] = route(info)
            return out
        finally:
            ctx.close()


def _peek_fallback(ctx, it):
    """n_fallback of the picture alone (0 or 1): read once, then held over three decodes by run_batch."""
    sc = scan(it)
    with ctx.batch([sc.desc]) as b:
        b.upload(); b.decode(); b.sync()
        n = b.info()["n_fallback"]
    assert n in (0, 1), (it.label, n)
    return n


@pytest.fixture(scope="module")
def alone(routes):
    return {label: r["n_fallback"] for label, r in routes.items()}


# ---- 0: routes -------------------------------------------------------------------------------------------------------------------------------
def test_routes(routes):
    """Every stream of fallback_corpus.falling() ends in the exact kernel when decoded alone, and equals the oracle there (run_batch in
    the fixture).  The recorded streams take the routes of tests/test_gpu_nosync.py; the new class-1 streams are one chain over nine
    waves: a wave publishes PJD_GENS = 6 generations, so the waves behind the sixth boundary are stale where generation 0 of the first
    wave is true (lane 63 starts at unit 128: the MCU's first unit in 4:2:2 and 4:4:0, four units an MCU) and behind the fifth where
    it is not (4:4:4, three units an MCU) -- DESIGN.md 4.2."""
    for n in F.FROM_NOSYNC:
        assert (routes[n]["n_fallback"], set(routes[n]["flags"])) == ROUTES[n], (n, routes[n])
    for n, reasons in ROUTES_NEW.items():
        s = F.falling()[n]
        r = routes[n]
        stale = F.waves(s) - (6 if TRUE_GEN0[s.sub] else 5)
        assert r["n_fallback"] == 1 and r["n_sequential"] == 0 and r["n_subsequences"] == s.n_lanes(128), (n, r)
        assert r["n_huff_waves"] == F.waves(s) == 9, (n, r)
        assert r["flags"] == reasons and r["flags"]["STITCH"] == stale, (n, r)
    assert routes["err_behind_flag"]["n_fallback"] == 1 and routes["err_first_wave"]["n_fallback"] == 0
    broken = [r for label, r in routes.items() if label.startswith("broken")]
    assert len(broken) >= 6 and sum(r["n_fallback"] for r in broken) >= 2
    assert all(set(r["flags"]) <= {"SEGMENT"} for r in broken), broken


# ---- 1: every dense kernel by itself ---------------------------------------------------------------------------------------------------------
def solo_items(lj, s):
    """The falling streams first, in the middle and last, good pictures and two broken restart streams between them, all with one
    flag set.  PJD_F_LIBJPEG refuses 4:4:0."""
    names = [n for n in F.falling() if not (lj and F.falling()[n].sub == "440")]
    br = F.broken()
    fall = [falling(n, lj, s) for n in names]
    between = [good(0, lj, s), item("broken0", br[0], lj, s), good(1, lj, s), item(f"broken{len(br) - 1}", br[-1], lj, s), good(0, lj, s)]
    out = []
    for k, f in enumerate(fall):
        out.append(f)
        if k < len(between) and k + 1 < len(fall):
            out.append(between[k])
    assert out[0].label in F.falling() and out[-1].label in F.falling()
    return out


@pytest.mark.parametrize("s", [1, 2, 4, 8])
@pytest.mark.parametrize("fmt", ["rgb8", "planar", "bmp", "gray"])
@pytest.mark.parametrize("arith", ["default", "libjpeg"])
def test_every_dense_kernel_by_itself(fctx, alone, arith, fmt, s):
    """One flag set and one output format a batch: the fallback launches exactly one of the dense kernels (and, for flagged colour
    pictures, the colour launch) on ranges of every sampling.  default: pjd_k_idct_dense* with PJD_F_SCALE_* in RGB8, planar, BMP and
    grey (PJD_GRAY_SCALED); libjpeg: pjd_k_idct_std_dense at full size, pjd_k_idct_std_dense_red / pjd_k_colour_std_red /
    pjd_k_idct_gray_std_dense_red at 1/2, 1/4, 1/8."""
    lj = arith == "libjpeg"
    items = solo_items(lj, s)
    assert {F.falling()[it.label].sub for it in items if it.label in F.falling()} >= {"grey", "420", "422", "444"}
    info = run_items(fctx, items, fmt, alone)
    assert info["n_fallback"] >= (6 if lj else 7)


# ---- 2: all three lists at once --------------------------------------------------------------------------------------------------------------
A, B = "lock_420_130", "lock_422_288"


def _progressive():
    given = {False: (0, recording(PROGRESSIVE, 2, "rgb")), True: (0, recording(PROGRESSIVE, 2, "l8"))}
    return item("progressive", ls_jpeg(PROGRESSIVE), True, 2, options=SCAN_PROGRESSIVE, given=given)


@functools.lru_cache(maxsize=1)
def mixed():
    """The 4:2:0 and the 4:2:2 falling stream under six flag sets each -- unflagged, PJD_F_SCALE_1_2, PJD_F_LIBJPEG, and PJD_F_LIBJPEG
    with each reduced scale -- in an order in which settle()'s three lists (default, full-size libjpeg, reduced) are not the picture
    order; between them a good picture of each kind, two PJD_F_FORCE_SEQUENTIAL pictures (dense ranges of the batch's own exact path,
    which the fallback must leave alone), a progressive picture, an entropy error the parallel decoder settles itself and a flagged
    wave behind an error (no fallback)."""
    return (
        falling(A, True, 4), good(0), falling(B), falling(A, True, 1), good(1, extra=FORCE), falling(B, True, 8), falling(A, False, 2),
        good(0, True, 2), falling(B, True, 1), _progressive(), falling(A), falling(B, True, 2), good(1, True, 1), falling(A, True, 2),
        item(ERR_FIXTURE, golden_bytes(ERR_FIXTURE)), falling(B, False, 2), good(0, False, 2), falling(A, True, 8),
        good(0, True, 4, extra=FORCE), falling(B, True, 4), item("err_first_wave", N.streams()["err_first_wave"].data, True, 1),
        good(1, True, 8),
    )


MIXED_FALLING = 12


def reduced_falling():
    return [k for k, it in enumerate(mixed()) if it.label in (A, B) and it.lj and it.s > 1]


@pytest.mark.parametrize("fmt", ["rgb8", "planar", "gray"])
def test_all_three_lists_at_once(fctx, alone, fmt):
    """n_fallback is the sum of what each falling member shows when decoded alone; every picture -- the re-decoded ones and every
    neighbour -- equals its own expectation."""
    items = list(mixed())
    kinds = [(it.lj, it.s > 1) for it in items if it.label in (A, B)]
    assert len(kinds) == MIXED_FALLING and kinds != sorted(kinds), "list order must differ from picture order"
    assert sum(is_sequential(it) for it in items) == 3 and len(reduced_falling()) == 6
    info = run_items(fctx, items, fmt, alone)
    assert info["n_fallback"] == MIXED_FALLING and info["n_entropy_errors"] >= 2, info
    assert info["flag_waves"][REASONS.index("STITCH")] >= MIXED_FALLING + 1


# ---- 3: flag against error position ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "gray"])
def test_flag_against_error_position_under_libjpeg(fctx, alone, fmt):
    """The chain across five wave boundaries with a run past slot 63 INSIDE the flagged wave (the picture falls back) and with an
    invalid code in the first wave (the flag lies behind the error: it does not), flagged at full size and at 1/4: the port's status
    and the model's partial picture -- zero coefficients behind the error, so 128 there at every scale."""
    items = []
    for s in (1, 4):
        for n in ("err_behind_flag", "err_first_wave"):
            items.append(item(n, N.streams()[n].data, True, s))
    gray = fmt == "gray"
    for it in items:
        st, p = expected(it, gray)
        assert st != 0 and (p[-(8 // it.s):, -(8 // it.s):] == 128).all() and not (p[:8 // it.s] == 128).all(), it.label
    assert alone["err_behind_flag"] == 1 and alone["err_first_wave"] == 0
    info = run_items(fctx, items, fmt, alone)
    assert info["n_fallback"] == 2 and info["n_entropy_errors"] == 2, info


# ---- 4: the resample behind a reduced re-decode ------------------------------------------------------------------------------------------------
TW, TH, PAD, FILL = 40, 24, (1, 1, 1, 1), (7, 130, 251)


def _canvas(it, gray, filt, w=TW, h=TH, pad=PAD, fill=FILL):
    return pm.padded(source(it, gray), None, w, h, pad, fill, 1, filt)


@pytest.mark.parametrize("form", ["bilinear_u8_planar", "antialias_f16_rgb8", "bicubic_u8_gray"])
def test_resample_behind_the_mixed_batch(fctx, alone, form):
    """The mixed batch resampled to 40 x 24 with a border of one sample: settle() runs the resize and border launches again, and they
    read pictures of ceil(W/s) x ceil(H/s) that the reduced dense kernels have just written."""
    import pjd_amd
    from pjd_amd import tensors
    filt, dt, fmt = form.split("_")
    gray = fmt == "gray"
    items = list(mixed())
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)

    def prepare(b):
        b.set_resize([(TH, TW)] * len(items))
        b.set_resize_pad([PAD] * len(items), FILL)
        if filt != "bilinear":
            b.set_resize_filter({"antialias": pjd_amd.RESIZE_ANTIALIAS, "bicubic": pjd_amd.RESIZE_BICUBIC}[filt])
        if dt == "f16":
            b.set_normalize(pjd_amd.DT_F16, scale, bias)

    wants = []
    for it in items:
        C = _canvas(it, gray, filt)
        if dt == "f16":
            wants.append(pm.normalized(C, TW, TH, PAD, nm.DT_F16, scale, bias))
        else:
            wants.append(np.ascontiguousarray(C[..., 0]) if gray else C)

    def compare_f16(got, wanted, label):
        assert got.shape == wanted.shape and got.dtype == np.float16, (label, got.shape, got.dtype)
        bad = np.argwhere(nm.bits(got) != nm.bits(wanted))
        assert bad.size == 0, (label, "first differing element", bad[0].tolist(), "differing", len(bad))

    statuses = [expected(it, gray)[0] for it in items]
    info = run_batch(fctx, items, fmt, statuses, wants, MIXED_FALLING, prepare, compare_f16 if dt == "f16" else None)
    assert info["n_fallback"] == sum(alone[it.label] for it in items if it.label in (A, B))


VIEW_SIZES = [(TH, TW), (17, 23), (9, 31)]          # (h, w)


def test_views_of_the_reduced_falling_pictures(fctx, alone):
    """One view of every picture, three of each falling reduced picture: the re-decoded picture feeds all its views."""
    items = list(mixed())
    views = []
    for k in range(len(items)):
        views.append((k, VIEW_SIZES[0]))
        if k in reduced_falling():
            views += [(k, VIEW_SIZES[1]), (k, VIEW_SIZES[2])]
    assert len(views) == len(items) + 12

    def prepare(b):
        b.set_views([k for k, _ in views])
        b.set_resize([hw for _, hw in views])

    wants = [_canvas(items[k], False, "bilinear", w, h, (0, 0, 0, 0), (0, 0, 0)) for k, (h, w) in views]
    statuses = [expected(it, False)[0] for it in items]
    run_batch(fctx, items, "rgb8", statuses, wants, MIXED_FALLING, prepare)


# ---- 5, 6: shards and caller-owned memory (child processes: torch has to load before the library) ------------------------------------------
def _torch_case(case, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "fallback_torch_cases.py"), case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


@pytest.mark.parametrize("fmt", ["rgb8", "gray"])
def test_shards_that_fall_back(fmt):
    """Each shard of fallback_corpus.shards() as a descriptor with shard_first_seg / shard_n_segs, bound into a tensor of 0xA5: the
    shard's rows equal the oracle's decode of the file that IS the shard, every other byte of the picture and of the tensor keeps the
    0xA5; n_fallback is 1 where the shard holds the broken segment and 0 for the sibling that ends before it."""
    _torch_case("shards_" + fmt)


@pytest.mark.parametrize("fmt", ["planar", "gray"])
def test_mixed_batch_bound_at_base_plus_one_keeps_its_guard_bytes(fmt):
    """The mixed batch bound at base + 1 with odd gaps between the pictures in a 0xA5 tensor: the pictures are the models', and every
    guard byte is intact after each of the three decodes."""
    _torch_case("mixed_" + fmt)
