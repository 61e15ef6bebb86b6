"""Views on decode (pjd_batch_set_views) on the GPU (run with -m gpu on an MI355X): several resampled outputs of one decoded picture.

Every expectation is tests/views_cases.py -- the numpy models of the resize tests over the oracle's picture of each view's fixture --
and every comparison is byte (bit, for floats) equality.  Five fixtures, views = [2, 0, 0, 3, 2, 2, 4, 0]: picture 1 has no view,
pictures 0 and 2 have three, every view has a target, window, flip, orientation and pad of its own, and picture 4 is a broken stream
whose view shows its partial picture."""
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as nm
import views_cases as V
from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_STATE = -3, -5
LAYOUTS = ["planar", "rgb8", "gray"]


def _fmt(layout):
    import pjd_amd
    return {"planar": pjd_amd.OUT_RGB8_PLANAR, "rgb8": pjd_amd.OUT_RGB8, "gray": pjd_amd.OUT_GRAY8}[layout]


def _scanned(data, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(data)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scanned():
    return [_scanned(V.golden_bytes(n)) for n in V.NAMES]


def _prepare(b, filt, dtype, spec=V.SPEC, sizes=None):
    """Every setter, with one entry per output of the batch."""
    import pjd_amd
    b.set_resize(sizes if sizes is not None else [V.canvas(v) for v in range(len(spec))])
    b.set_resize_pad([s[2] for s in spec], V.FILL)
    b.set_orientation([s[1] for s in spec])
    b.set_resize_window([s[3] for s in spec])
    if filt != "bilinear":
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS if filt == "antialias" else pjd_amd.RESIZE_BICUBIC)
    if dtype:
        scale, bias = V.constants()
        b.set_normalize(dtype, scale, bias)
        b.set_pad_value(V.PAD_VALUE)


def _names(b):
    """The launches of one timed decode, in order, duplicates kept."""
    import ctypes as C
    import pjd_amd
    t = pjd_amd.Timings()
    b.ctx._check(b.L.pjd_batch_decode_timed(b._h, C.byref(t)), "pjd_batch_decode_timed")
    b.sync()
    return [t.name[i].value.decode() for i in range(t.n)]


def _check_views(port, outs, filt, layout, dtype, what=""):
    assert len(outs) == len(V.VIEWS)
    for v, o in enumerate(outs):
        V.same(o, V.expected(port, v, filt, layout, dtype, V.PAD_VALUE if dtype else None), dtype, (what, "view", v, filt, layout, dtype))


def _check_statuses(port, st):
    want = [V.oracle(port)[n][0] for n in V.NAMES]
    assert len(st) == len(V.NAMES) and st == want and want[4] != 0 and want[:4] == [0, 0, 0, 0], (st, want)


# ---- 1: every view equals its model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, nm.DT_F16], ids=["u8", "f16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("filt", V.FILTERS)
def test_every_view_equals_its_model(ctx, port, scanned, filt, layout, dtype):
    es = 2 if dtype else 1
    nc = 1 if layout == "gray" else 3
    with ctx.batch([s.desc for s in scanned], _fmt(layout)) as b:
        assert b.n_out == 5 and b.L.pjd_batch_n_outputs(b._h) == 5
        b.set_views(V.VIEWS)
        assert b.n == 5 and b.n_out == 8 and b.L.pjd_batch_n_outputs(b._h) == 8
        _prepare(b, filt, dtype)
        sizes = [nc * V.canvas(v)[0] * V.canvas(v)[1] * es for v in range(8)]
        assert [b.output_size(v) for v in range(8)] == sizes and b.output_size(8) == 0
        assert all(b.output_offset(v) % 256 == 0 for v in range(8)) and b.packed_size() >= b.output_offset(7) + sizes[7]
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
        packed, st_p = b.download_packed()
    _check_statuses(port, st)
    assert st_p == st and [p.size for p in packed] == sizes
    assert info["n_images"] == 5 and info["out_bytes"] == sum(sizes)
    _check_views(port, outs, filt, layout, dtype)
    for v in range(8):
        assert packed[v].tobytes() == outs[v].tobytes(), v
    # the view of the broken stream shows its partial picture: grey where nothing was decoded, and not grey everywhere
    rgb = V.oracle(port)[V.NAMES[4]][1]
    assert (rgb[-1] == 128).all() and not (rgb[0] == 128).all()


# ---- 2: the batch that holds every view's descriptor once more delivers the same bytes ---------------------------------------------------
@pytest.mark.parametrize("layout,dtype", [("planar", 0), ("rgb8", nm.DT_F16), ("gray", 0)], ids=["planar_u8", "rgb8_f16", "gray_u8"])
@pytest.mark.parametrize("filt", V.FILTERS)
def test_equals_the_batch_with_repeated_descriptors(ctx, scanned, filt, layout, dtype):
    got = []
    for views in (V.VIEWS, None):
        descs = [s.desc for s in scanned] if views else [scanned[p].desc for p in V.VIEWS]
        with ctx.batch(descs, _fmt(layout)) as b:
            if views:
                b.set_views(views)
            _prepare(b, filt, dtype)
            b.upload(); b.decode()
            outs, st = b.download()
        got.append((outs, st))
    (a, st_a), (r, st_r) = got
    assert len(a) == len(r) == 8 and len(st_a) == 5 and len(st_r) == 8
    assert [st_a[p] for p in V.VIEWS] == st_r
    for v in range(8):
        assert a[v].shape == r[v].shape and a[v].tobytes() == r[v].tobytes(), (v, filt, layout)


# ---- 3: the decode is paid once ----------------------------------------------------------------------------------------------------------
def test_the_decode_is_paid_once(ctx, scanned):
    import pjd_amd
    keys = ("n_subsequences", "n_huff_workgroups", "n_data_units", "n_huff_waves", "pixels", "ecs_bytes", "n_images")
    infos, names = {}, {}
    for what, descs, views in (("views", [s.desc for s in scanned], V.VIEWS), ("five", [s.desc for s in scanned], None),
                               ("eight", [scanned[p].desc for p in V.VIEWS], None)):
        spec = V.SPEC if what != "five" else V.SPEC[:5]
        with ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR) as b:
            if views:
                b.set_views(views)
            _prepare(b, "bilinear", 0, spec, sizes=[V.canvas(v) for v in range(len(spec))])
            b.upload()
            names[what] = _names(b)
            infos[what] = b.info()
    assert {k: infos["views"][k] for k in keys} == {k: infos["five"][k] for k in keys}
    for k in ("n_subsequences", "n_data_units", "pixels", "ecs_bytes"):
        assert infos["views"][k] < infos["eight"][k], k
    assert infos["views"]["n_huff_workgroups"] <= infos["eight"]["n_huff_workgroups"]
    assert infos["views"]["out_bytes"] == infos["eight"]["out_bytes"]
    assert names["views"].count("resize") == 1 and names["views"].count("pad") <= 1, names["views"]
    assert names["views"] == names["five"], "the launches of the five-picture batch, no more"


# ---- 4: identity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_views_equal_no_call(ctx, scanned, layout):
    spec = V.SPEC[:5]
    got = []
    for views in (None, [0, 1, 2, 3, 4]):
        with ctx.batch([s.desc for s in scanned], _fmt(layout)) as b:
            if views:
                b.set_views(views)
            _prepare(b, "antialias", nm.DT_F16, spec, sizes=[V.canvas(v) for v in range(5)])
            b.upload(); b.decode()
            outs, st = b.download()
            got.append((outs, st, _names(b), b.info()["device_bytes"]))
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] and got[0][3] == got[1][3]
    for v in range(5):
        assert got[0][0][v].tobytes() == got[1][0][v].tobytes(), v


def test_normalize_without_resize_takes_each_views_own_size(ctx, port, scanned):
    import pjd_amd
    scale, bias = V.constants()
    views = [3, 0, 3, 2]
    with ctx.batch([s.desc for s in scanned], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_views(views)
        b.set_normalize(nm.DT_F32, scale, bias)
        assert [b.output_shape(v) for v in range(4)] == [(3, 70, 33), (3, 45, 61), (3, 70, 33), (3, 61, 45)]
        b.upload(); b.decode()
        outs, st = b.download()
    assert len(st) == 5
    for v, p in enumerate(views):
        want = nm.normalize(V.oracle(port)[V.NAMES[p]][1], nm.DT_F32, scale, bias).transpose(2, 0, 1)
        V.same(outs[v], np.ascontiguousarray(want), nm.DT_F32, ("normalize only", v))


@pytest.mark.parametrize("filt", V.FILTERS)
def test_tiles_reassemble_the_decoded_picture(ctx, port, filt):
    """One synthetic 264 x 400 picture cut by tile_views into 64 x 64 tiles (edge tiles 8 wide and 16 high): 35 views of one picture."""
    import pjd_amd
    from pjd_amd import tensors
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth
    w, h = 264, 400
    data = synth.make(w, h, 77, 90, synth.SUB_420)
    rgb = port.decode(data)["rgb"]
    assert rgb.shape == (h, w, 3)
    windows, sizes = tensors.tile_views(h, w, 64, 64)
    assert len(sizes) == 7 * 5 and sizes[4] == (64, 8) and sizes[-1] == (16, 8)
    sc = _scanned(data)
    with ctx.batch([sc.desc], pjd_amd.OUT_RGB8) as b:
        b.set_views([0] * len(sizes))
        b.set_resize(sizes)
        b.set_resize_window(windows)
        if filt != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS if filt == "antialias" else pjd_amd.RESIZE_BICUBIC)
        b.upload(); b.decode()
        outs, st = b.download()
        assert b.info()["n_images"] == 1
    assert st == [0]
    whole = np.zeros_like(rgb)
    for win, o in zip(windows, outs):
        assert o.shape == (win["h"], win["w"], 3)
        whole[win["y"]:win["y"] + win["h"], win["x"]:win["x"] + win["w"]] = o
    assert np.array_equal(whole, rgb)


# ---- 5: placement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, nm.DT_F16], ids=["u8", "f16"])
def test_bound_views_in_reverse_order_between_canaries(ctx, port, scanned, dtype):
    """The eight views bound into caller-owned memory (a donor batch's decoded picture: the canary) in REVERSE view order with gaps of
    1, 3 and 255 elements: every range is the model's and every byte outside the ranges the donor's, after a decode, after a second
    decode over memory the donor has filled again, and after two replays of the captured graph."""
    import pjd_amd
    es = 2 if dtype else 1
    donor_sc = _scanned(V.golden_bytes("big_640x480_420_q85"))
    with ctx.batch([donor_sc.desc], pjd_amd.OUT_RGB8) as donor:
        donor.upload(); donor.decode()
        (pattern,), _ = donor.download()
        pattern = pattern.reshape(-1).copy()
        mem, cap = donor.device_output(0), donor.output_size(0)
        with ctx.batch([s.desc for s in scanned], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_views(V.VIEWS)
            _prepare(b, "bicubic", dtype)
            sizes = [b.output_size(v) for v in range(8)]
            offs, pos = [0] * 8, 5 * es
            for k, v in enumerate(reversed(range(8))):
                offs[v] = pos
                pos += sizes[v] + (1, 3, 255)[k % 3] * es
            assert pos <= cap and offs[7] < offs[0] and (not dtype or any((mem + o) % 4 == 2 for o in offs))
            with pytest.raises(pjd_amd.PjdError, match=r"view 0 \(picture 2\) ends beyond the capacity"):
                b.bind_output(mem, offs[0] + sizes[0] - 1, offs)
            b.bind_output(mem, cap, offs)
            assert [b.output_offset(v) for v in range(8)] == offs
            b.upload()
            inside = np.zeros(cap, bool)
            for o, n in zip(offs, sizes):
                assert not inside[o:o + n].any()
                inside[o:o + n] = True
            for what in ("first", "second", "replay 1", "replay 2"):
                if what == "replay 1":
                    b.capture()
                donor.decode(); donor.sync()                     # the memory is the donor's picture again: nothing of the last decode is left
                b.decode(); b.sync()
                outs, st = b.download()
                (after,), _ = donor.download()
                after = after.reshape(-1)
                _check_statuses(port, st)
                _check_views(port, outs, "bicubic", "planar", dtype, what)
                for v in range(8):
                    assert after[offs[v]:offs[v] + sizes[v]].tobytes() == outs[v].tobytes(), (what, v)
                stray = np.flatnonzero(~inside & (after != pattern))
                assert stray.size == 0, (what, "bytes outside every view's range were written, first at", stray[:8])


# ---- 6: the exact-kernel fallback ------------------------------------------------------------------------------------------------------
def test_views_are_resampled_again_after_the_fallback(port, monkeypatch):
    """A picture forced onto the exact kernel and a stream of tests/nosync_corpus.py that the parallel decoder gives up on (128-byte
    lanes), three views each: after pjd_batch_sync n_fallback is that of the batch without views, and every view is the model's."""
    import nosync_corpus as N
    import pjd_amd
    import resize_pad_model as pm
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    for k in ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE"):
        monkeypatch.delenv(k, raising=False)
    s = N.streams()["chain_x5"]
    o = port.decode(s.data)
    assert o["valid"] and o["huff_rc"] == 0
    pics = [V.oracle(port)[V.NAMES[0]][1], o["rgb"]]
    sc = [_scanned(V.golden_bytes(V.NAMES[0]), pjd_amd.F_FORCE_SEQUENTIAL), pjd_amd.Scanned(s.data)]
    assert sc[1].valid
    sc[1].desc.flags = pjd_amd.F_STANDARD_RESTART if s.fr.standard_restart else 0
    H1, W1 = pics[1].shape[:2]
    win1 = dict(x=0, y=0, w=min(W1, 96), h=min(H1, 64))
    views = [1, 0, 1, 0, 0, 1]
    spec = [((23, 17), 1, (0, 0, 0, 0), win1), ((96, 96), 6, (1, 2, 3, 0), None), ((7, 5), 2, (0, 0, 0, 0), win1),
            ((19, 11), 3, (5, 3, 6, 4), dict(x=3, y=5, w=40, h=30, flags=1)), ((61, 45), 1, (0, 0, 0, 0), None), ((40, 31), 8, (0, 1, 2, 0), win1)]

    def canvas(k, spec=spec):
        (tw, th), o_, pad, _ = spec[k]
        cw, ch = (th, tw) if o_ >= 5 else (tw, th)
        return (ch + pad[1] + pad[3], cw + pad[0] + pad[2])

    plain = [spec[1], spec[0]]                                  # the batch without views: one output per picture, picture 0 first

    c = pjd_amd.Context(0)
    try:
        for filt in ("bilinear", "bicubic"):
            res = {}
            for what in ("views", "plain"):
                with c.batch([x.desc for x in sc], pjd_amd.OUT_RGB8) as b:
                    if what == "views":
                        b.set_views(views)
                        _prepare(b, filt, 0, spec, sizes=[canvas(k) for k in range(6)])
                    else:
                        _prepare(b, filt, 0, plain, sizes=[canvas(k, plain) for k in range(2)])
                    b.upload(); b.decode(); b.sync()
                    outs, st = b.download()
                    res[what] = (outs, st, b.info())
            iv, ip = res["views"][2], res["plain"][2]
            assert (iv["n_fallback"], iv["n_sequential"]) == (ip["n_fallback"], ip["n_sequential"]) == (1, 1), (iv, ip)
            assert res["views"][1] == [0, 0]
            for k, p in enumerate(views):
                (tw, th), o_, pad, win = spec[k]
                h, w = canvas(k)
                want = pm.padded(pics[p], win, w, h, pad, V.FILL, o_, filt)
                V.same(res["views"][0][k], want, 0, ("fallback", filt, k))
    finally:
        c.close()


# ---- 7: errors ---------------------------------------------------------------------------------------------------------------------------
def _refused(b, call, code, text=None):
    import pjd_amd
    with pytest.raises(pjd_amd.PjdError) as e:
        call()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def test_refusals_and_that_the_batch_still_works(ctx, port, scanned):
    import ctypes as C
    import pjd_amd
    L = ctx.L
    descs = [s.desc for s in scanned]
    assert L.pjd_batch_n_outputs(None) == 0
    assert L.pjd_batch_set_views(None, (C.c_uint32 * 1)(0), 1) == E_ARG
    with ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR) as b:
        # PJD_E_ARG: null array, no view, too many, an entry that names no picture; the call stays open
        assert L.pjd_batch_set_views(b._h, None, 3) == E_ARG and b"null" in L.pjd_last_error(ctx._h)
        assert L.pjd_batch_set_views(b._h, (C.c_uint32 * 1)(0), 0) == E_ARG
        big = (C.c_uint32 * 65537)()
        assert L.pjd_batch_set_views(b._h, big, 65537) == E_ARG and b"PJD_MAX_VIEWS" in L.pjd_last_error(ctx._h)
        _refused(b, lambda: b.set_views([0, 1, 5, 2]), E_ARG, "view 2 names picture 5")
        assert b.n_out == 5 and L.pjd_batch_n_outputs(b._h) == 5
        b.set_views(V.VIEWS)
        _refused(b, lambda: b.set_views(V.VIEWS), E_STATE, "already set")
        # views need the resample
        donor_mem = 256
        _refused(b, lambda: b.upload(), E_STATE, "views but no resample")
        _refused(b, lambda: b.decode(), E_STATE, "views but no resample")
        _refused(b, lambda: b.capture(), E_STATE, "views but no resample")
        _refused(b, lambda: b.bind_output(donor_mem, 1 << 20), E_STATE, "views but no resample")
        # the setters name the view
        with pytest.raises(ValueError):
            b.set_resize([(8, 8)] * 5)
        sizes = [V.canvas(v) for v in range(8)]
        _refused(b, lambda: b.set_resize(sizes[:3] + [(0, 9)] + sizes[4:]), E_ARG, "view 3 (picture 3): target width and height must be 1..65535")
        b.set_resize(sizes)
        pads = [s[2] for s in V.SPEC]
        _refused(b, lambda: b.set_resize_pad(pads[:6] + [(40, 0, 1, 0)] + pads[7:], V.FILL), E_ARG, "view 6 (picture 4): left + right")
        b.set_resize_pad(pads, V.FILL)
        _refused(b, lambda: b.set_orientation([1, 6, 1, 3, 9, 2, 4, 1]), E_ARG, "view 4 (picture 2): the orientation must be 1..8")
        b.set_orientation([s[1] for s in V.SPEC])
        wins = [s[3] for s in V.SPEC]
        _refused(b, lambda: b.set_resize_window(wins[:5] + [dict(x=40, y=0, w=10, h=10)] + wins[6:]), E_ARG, "view 5 (picture 2): the window is not inside")
        b.set_resize_window(wins)
        _refused(b, lambda: b.set_resize_filter(2), E_ARG, "unknown filter")
        b.upload(); b.decode()
        outs, st = b.download()
        _check_statuses(port, st)
        _check_views(port, outs, "bilinear", "planar", 0, "after the refusals")
        _refused(b, lambda: b.set_views(V.VIEWS), E_STATE)
    # the 16x limit of the table-driven filters names the view: the 96 rows of picture 1 to 5 rows
    for wins, text in ((None, "view 1 (picture 1) is more than 16x its target"), ([None, dict(flags=1), None], "the window of view 1 (picture 1) is more than 16x")):
        with ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR) as b:
            b.set_views([0, 1, 1])
            b.set_resize([(5, 7), (5, 7), (6, 7)])
            if wins:
                b.set_resize_window(wins)
            _refused(b, lambda: b.set_resize_filter(pjd_amd.RESIZE_BICUBIC), E_ARG, text)
            b.upload(); b.decode()
            assert b.download()[1] == [V.oracle(port)[n][0] for n in V.NAMES]
    # call order: not after a resize, a normalisation, a bind or an upload
    for first, text in ((lambda b: b.set_resize([(8, 8)] * 5), "after set_resize"),
                        (lambda b: b.set_normalize(nm.DT_F16, *V.constants()), "after set_normalize"),
                        (lambda b: b.upload(), "after upload")):
        with ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR) as b:
            first(b)
            _refused(b, lambda: b.set_views([0]), E_STATE, text)
            assert b.n_out == 5
    # a BMP batch takes no views; a view of a shard is refused by set_resize and names the view
    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        _refused(b, lambda: b.set_views([0, 0]), E_ARG, "BMP")
        b.upload(); b.decode()
        assert len(b.download()[0]) == 5
    from pjd_amd import parallel
    whole = _scanned(V.golden_bytes("rst4_128x96_444"))
    segs, ecs = whole.seg_offsets(), whole.ecs()
    f, c = parallel.segment_range(len(segs), 1, 2)
    lo = int(segs[f]); hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
    shard, keep = parallel.shard_descriptor(whole.desc, segs, ecs[lo:hi], lo, 1, 2)
    assert int(shard.shard_n_segs) != 0
    with ctx.batch([scanned[0].desc, shard], pjd_amd.OUT_RGB8) as b:
        b.set_views([0, 0, 1])
        _refused(b, lambda: b.set_resize([(8, 8)] * 3), E_ARG, "view 2 (picture 1) is a shard")
        _refused(b, lambda: b.set_normalize(nm.DT_F16, *V.constants()), E_ARG, "view 2 (picture 1) is a shard")
    with ctx.batch([scanned[0].desc, shard], pjd_amd.OUT_RGB8) as b:
        b.set_views([0, 0])                                                               # the shard has no view: accepted
        b.set_resize([(8, 8), (9, 7)])
        b.upload(); b.decode()
        outs, st = b.download()
        assert len(outs) == 2 and len(st) == 2


# ---- 8: the tensor helpers, each case in a process of its own (torch loads first) --------------------------------------------------------
@pytest.mark.parametrize("case", ["resized_views", "normalized_views", "two_crops_prescaled"])
def test_tensor_helpers(case):
    r = subprocess.run([sys.executable, os.path.join(HERE, "views_torch_cases.py"), case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
