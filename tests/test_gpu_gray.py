"""Grey output (PJD_OUT_GRAY8) on the GPU (run with -m gpu on an MI355X): zero tolerance everywhere.  The expected plane never comes
from the library: under the reference's arithmetic it is channel 0 of the oracle's picture with every chroma coefficient zeroed
(tests/gray_expected.py; tests/test_gray_cpu.py holds its three channels equal), under PJD_F_LIBJPEG Pillow's recorded draft("L")
decode (tests/golden/libjpeg_gray/), through the box model of the scaled tests for a reduced-size picture.

Kernel forms launched here (all of pjd_k_backend_gray.hip): pjd_k_idct_gray_lanes<false> and <true> (tests 1, 2: parallel),
pjd_k_idct_gray<false> and <true> (tests 1, 2: sequential; test 5: the fallback), pjd_k_idct_gray_std_lanes and
pjd_k_idct_gray_std_dense (test 3; test 5: the fallback of a flagged picture); and all of the one-plane resample, which has the
padded (most general) form alone (pjd_k_resize.hip): pjd_k_resize_gray<DT> for DT = uint8, fp16, bf16, fp32 and pjd_k_resize_gray_tab<DT, FILT> for the same four and
FILT = antialias, bicubic -- twelve forms, each launched by test 6, which crosses the three filters with the four element types (and
lists what it launched)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import gray_expected as G
from gray_expected import golden_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
VALID = sorted(k for k, v in MANIFEST.items() if v["rc"] == 0)
SCALES = [(16, 2), (32, 4), (48, 8)]        # (PJD_F_SCALE_*, s)
E_ARG, E_STATE = -3, -5


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planes(port):
    """name -> (status, expected full-size plane) for every decodable fixture: computed once, never changed"""
    out = {}
    for n in VALID:
        st, p = G.ref_plane(port, golden_bytes(n))
        p.setflags(write=False)
        out[n] = (st, p)
    return out


def _scanned(data, flags=0, options=0):
    import pjd_amd
    s = pjd_amd.Scanned(data, options=options)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def _lj(name, extra=0, flag=True):
    import pjd_amd
    data, c = G.lj_bytes(name), G.lj_cases()[name]
    return _scanned(data, (pjd_amd.F_LIBJPEG if flag else 0) | extra, pjd_amd.SCAN_PROGRESSIVE if c["progressive"] else 0)


def _lj_names():
    return sorted(G.lj_cases())


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), "bytes differ")


# ---- 1: every fixture in one grey batch, both front ends ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parallel", "sequential"])
def test_every_fixture_in_one_gray_batch(ctx, planes, mode):
    import pjd_amd
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "sequential" else 0
    sc = [_scanned(golden_bytes(n), extra) for n in VALID]
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.upload(); b.decode()
        outs, st = b.download()
        info = b.info()
        assert [b.output_size(i) for i in range(b.n)] == [int(s.desc.width) * int(s.desc.height) for s in sc]
    for n, o, status in zip(VALID, outs, st):
        assert status == planes[n][0], n
        _same(o, planes[n][1], (n, mode))
    assert info["out_bytes"] == sum(int(s.desc.width) * int(s.desc.height) for s in sc)
    if mode == "parallel":
        assert info["n_fallback"] == 0, info["flag_waves"]
        assert any(st) and {int(s.desc.h_samp) * 2 + int(s.desc.v_samp) for s in sc} >= {3, 4, 5, 6}      # broken streams; all four samplings
    else:
        assert info["n_sequential"] == len(sc)


# ---- 2: the same pictures at the three box scales -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parallel", "sequential"])
def test_every_fixture_at_the_three_scales(ctx, planes, mode):
    import pjd_amd
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "sequential" else 0
    items = [(n, flags, s) for n in VALID for flags, s in SCALES]
    sc = [_scanned(golden_bytes(n), flags | extra) for n, flags, _ in items]
    outs, st = ctx.decode([x.desc for x in sc], pjd_amd.OUT_GRAY8)
    for (n, _, s), o, status in zip(items, outs, st):
        assert status == planes[n][0], (n, s)
        _same(o, G.box1(planes[n][1], s), (n, s, mode))


def test_full_size_and_scaled_pictures_share_a_batch(ctx, planes):
    import pjd_amd
    names = ["env_61x45_420_q100_opt", "gray_33x70", "h1v2_48x64", "env_17x9_422_q30_opt"]
    items = [(n, flags, s) for n in names for flags, s in [(0, 1)] + SCALES]
    sc = [_scanned(golden_bytes(n), flags) for n, flags, _ in items]
    outs, st = ctx.decode([x.desc for x in sc], pjd_amd.OUT_GRAY8)
    for (n, _, s), o in zip(items, outs):
        _same(o, G.box1(planes[n][1], s), (n, s))


# ---- 3: PJD_F_LIBJPEG ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["parallel", "sequential"])
def test_every_libjpeg_fixture_equals_pillows_draft_L(ctx, path):
    import pjd_amd
    names = _lj_names()
    assert len(names) == 17
    sc = [_lj(n, pjd_amd.F_FORCE_SEQUENTIAL if path == "sequential" else 0) for n in names]
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
    assert list(st) == [0] * len(names)
    for n, got in zip(names, outs):
        _same(got, G.l8(n), (n, path))
    assert info["n_fallback"] == 0, info["flag_waves"]
    big = sc[names.index("lj_136x72_420_q90")]
    assert pjd_amd.plan_info([big.desc], pjd_amd.OUT_GRAY8)["n_data_units"] == 270 > 2 * 96     # several back-end ranges


def test_flagged_and_unflagged_pictures_in_one_gray_batch(ctx, planes):
    """Interleaved: the flagged pictures are libjpeg's luma, the others the reference's; the timed decode names the two launches and
    no colour launch; the batch holds no plane buffer -- less device memory than the same batch as PJD_OUT_RGB8_PLANAR by more than the
    smaller pictures alone explain."""
    import pjd_amd
    plain = ["env_64x48_420_q100", "rst4_128x96_444", "env_17x9_444_q85", "env_61x45_422_q30"]
    flagged = ["lj_136x72_420_q90", "lj_40x24_422_q90", "lj_8x8_444_q90", "lj_61x45_grey_q50"]
    items, want = [], []
    for p, f in zip(plain, flagged):
        items.append(_scanned(golden_bytes(p))); want.append(planes[p][1])
        items.append(_lj(f)); want.append(G.l8(f))
    with ctx.batch([s.desc for s in items], pjd_amd.OUT_GRAY8) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        for k, (g, w) in enumerate(zip(outs, want)):
            _same(g, w, k)
        timed, _ = b.decode_timed()
        b.sync()
        again, _ = b.download()
        assert all(np.array_equal(g, w) for g, w in zip(again, want))
        gray_info = b.info()
    assert list(st) == [0] * len(items)
    assert "idct_gray" in timed and "idct_gray_std" in timed and "colour_std" not in timed and "idct_colour" not in timed, timed
    with ctx.batch([s.desc for s in items], pjd_amd.OUT_RGB8_PLANAR) as b:
        planar_info = b.info()
    px = sum(int(s.desc.width) * int(s.desc.height) for s in items)
    assert gray_info["out_bytes"] == px and planar_info["out_bytes"] == 3 * px
    out_saving = 3 * 256 * len(items) + 2 * px                     # at most: two planes of every picture, their 256-byte alignment
    assert gray_info["device_bytes"] < planar_info["device_bytes"] - out_saving - 136 * 72      # ... and the luma plane of the largest flagged one


def test_truncated_libjpeg_stream_is_128_behind_the_error(ctx, port):
    """The expected plane is the libjpeg model over the ORACLE's coefficients of the broken stream (zero behind the error)."""
    import pjd_amd
    data = G.truncated_lj()
    want_st, want = G.model_y_plane(port, data, broken=True)
    assert want_st != 0
    for extra in (0, pjd_amd.F_FORCE_SEQUENTIAL):
        s = _scanned(data, pjd_amd.F_LIBJPEG | extra)
        outs, st = ctx.decode([s.desc], pjd_amd.OUT_GRAY8)
        assert st[0] == want_st
        _same(outs[0], want, extra)
        assert (outs[0][16:] == 128).all() and not (outs[0][:8] == 128).all()


# ---- 4: bound output, poisoned allocations, canaries --------------------------------------------------------------------------------
def _torch_case(case, *args, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(HERE, "gray_torch_cases.py"), case] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


@pytest.mark.parametrize("poison", ["0x00", "0xa5"])
def test_bound_at_an_odd_address_every_byte_inside_none_outside(poison):
    """Widths 3, 4, 5, 17, 33 and 61, flagged and unflagged, full size and scaled, parallel and exact, bound at an odd device address
    with canary bytes before, between and behind the pictures; decoded twice over two canary patterns."""
    _torch_case("bound_canaries", env={"PJD_DEBUG_POISON": poison})


# ---- 5: captured graph, exact-kernel fallback ---------------------------------------------------------------------------------------
def test_captured_graph_replayed_twice(ctx, planes):
    import pjd_amd
    names = [n for n in VALID if not n.startswith("big_")][:40]
    lj = _lj_names()
    sc = [_scanned(golden_bytes(n)) for n in names] + [_lj(n) for n in lj]
    want = [planes[n] for n in names] + [(0, G.l8(n)) for n in lj]
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.upload(); b.capture()
        for _ in range(2):
            b.decode(); b.sync()
            outs, st = b.download()
            for k, (o, (status, p)) in enumerate(zip(outs, want)):
                assert st[k] == status
                _same(o, p, k)


def test_pictures_that_fall_to_the_exact_kernel(ctx, port):
    """Restart markers a byte off (the streams of tests/test_gpu_poisoned_memory.py): the parallel decoder flags them and
    pjd_batch_sync decodes them again through the dense grey kernel, into the same memory."""
    import pjd_amd
    jpegs = G.misplaced_restart_markers(port)
    assert len(jpegs) >= 6
    sc = [_scanned(j) for j in jpegs] + [_scanned(golden_bytes("env_61x45_420_q100_opt"), pjd_amd.F_SCALE_1_2)]
    want = [G.ref_plane(port, j) for j in jpegs] + [(0, G.box1(G.ref_plane(port, golden_bytes("env_61x45_420_q100_opt"))[1], 2))]
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.upload()
        for rep in range(2):
            b.decode()
            outs, st = b.download()
            info = b.info()
            assert info["n_fallback"] >= 1 and info["n_sequential"] == 0, (rep, info)
            for k, (o, (status, p)) in enumerate(zip(outs, want)):
                assert st[k] == status, k
                _same(o, p, (k, rep))


def test_fallback_redecodes_flagged_pictures_of_a_gray_batch(port, monkeypatch):
    """The grey counterpart of tests/test_gpu_libjpeg_corpus.py::test_fallback_redecodes_flagged_pictures: the same broken streams once
    flagged PJD_F_LIBJPEG and once plain, beside a good flagged picture, on a context of its own whose allocations start as 0xA5.
    settle() decodes the flagged ones again through the dense libjpeg grey kernel, the plain ones through the dense grey kernel.  More
    pictures are re-decoded than in the same batch without the flagged broken streams: a flagged one is among them."""
    import pjd_amd
    monkeypatch.setenv("PJD_DEBUG_POISON", "0xa5")
    jpegs = G.misplaced_restart_markers(port)
    assert len(jpegs) >= 6
    good = "lj_8x8_444_q90"
    plain = [(_scanned(j), G.ref_plane(port, j)) for j in jpegs]
    rows = [(_scanned(j, pjd_amd.F_LIBJPEG), G.model_y_plane(port, j, broken=True)) for j in jpegs] + [(_lj(good), (0, G.l8(good)))] + plain
    c = pjd_amd.Context(0)
    try:
        n_fallback = []
        for batch in (rows, rows[len(jpegs):]):
            with c.batch([s.desc for s, _ in batch], pjd_amd.OUT_GRAY8) as b:
                b.upload()
                for rep in range(2):
                    b.decode(); b.sync()
                    outs, st = b.download()
                    for k, (_, (status, p)) in enumerate(batch):
                        assert st[k] == status, (k, rep, len(batch))
                        _same(outs[k], p, (k, rep, len(batch)))
                info = b.info()
            assert info["n_sequential"] == 0, info
            n_fallback.append(info["n_fallback"])
    finally:
        c.close()
    assert n_fallback[0] >= 2 and n_fallback[0] > n_fallback[1], n_fallback


# ---- 6: shards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", [("rst4_128x96_444", 4), ("rstrow_gray_100x60", 3)])
def test_shard_writes_only_its_mcus(ctx, planes, name, world):
    import pjd_amd
    from pjd_amd import parallel
    sc = _scanned(golden_bytes(name))
    segs, ecs, d0 = sc.seg_offsets(), sc.ecs(), sc.desc
    want = planes[name][1]
    got = np.zeros_like(want)
    mcux = (d0.width + 7) // 8
    for r in range(world):
        f, c = parallel.segment_range(len(segs), r, world)
        lo = int(segs[f])
        hi = int(segs[f + c]) if f + c < len(segs) else len(ecs)
        d, keep = parallel.shard_descriptor(d0, segs, ecs[lo:hi], lo, r, world)
        outs, st = ctx.decode([d], pjd_amd.OUT_GRAY8)
        assert st == [0] and outs[0].shape == want.shape
        m0, m1 = f * d0.restart_interval, min((f + c) * d0.restart_interval, mcux * ((d0.height + 7) // 8))
        for k in range(m0, m1):
            y0, x0 = (k // mcux) * 8, (k % mcux) * 8
            got[y0:y0 + 8, x0:x0 + 8] = outs[0][y0:y0 + 8, x0:x0 + 8]
    _same(got, want, name)


# ---- 6: the one-plane resample -------------------------------------------------------------------------------------------------------
RESIZE_NAMES = ["env_61x45_420_q100_opt", "gray_33x70", "h1v2_48x64"]
FORMS = ["plain", "window_hflip", "orientations", "pad"]
LAUNCHED = set()                                # (kernel form, element type, filter) of every NC = 1 launch test 6 made


def _resize_case(ctx, planes, filt, form, dt, k):
    """One batch of the three pictures: ragged targets (widths not divisible by 4; a 1x1 where the filter's 16x limit admits it),
    the form's records, the element type; -> compared bit for bit with the models of the three-channel tests on the picture whose three
    channels are the expected plane, channel 0."""
    import pjd_amd
    import normalize_model as nm
    import resize_pad_model as pm
    sc = [_scanned(golden_bytes(n)) for n in RESIZE_NAMES]
    targets = [(23, 17), (1, 1) if filt == "bilinear" else (9, 7), (41, 30)]          # (w, h) of the content
    wins, oris, pads = [None] * 3, [1] * 3, [(0, 0, 0, 0)] * 3
    fill, pad_value = (0, 0, 0), None
    if form == "window_hflip":
        wins = [dict(x=3, y=2, w=int(s.desc.width) - 7, h=int(s.desc.height) - 5, flags=pjd_amd.RW_HFLIP) for s in sc]
    elif form == "orientations":
        oris = [(3 * k + i) % 8 + 1 for i in range(3)]
    elif form == "pad":
        pads = [(2, 1, 3, 2), (0, 2, 1, 0), (5, 0, 0, 3)]
        fill = (77, 77, 77)
        pad_value = (-1.5, -1.5, -1.5) if dt and k % 2 else None
    canv = [(w + p[0] + p[2], h + p[1] + p[3]) for (w, h), p in zip(targets, pads)]      # delivered (w, h) before the orientation
    canv = [(h, w) if o >= 5 else (w, h) for (w, h), o in zip(canv, oris)]
    scale, bias = np.array([1 / 255 / 0.226, 9.0, 9.0], np.float32), np.array([-0.449 / 0.226, 9.0, 9.0], np.float32)   # [1], [2]: ignored
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.set_resize([(h, w) for w, h in canv])
        if form == "pad":
            b.set_resize_pad(pads, fill)
        if form == "orientations":
            b.set_orientation(oris)
        if form == "window_hflip":
            b.set_resize_window(wins)
        if filt != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_BICUBIC if filt == "bicubic" else pjd_amd.RESIZE_ANTIALIAS)
        if dt:
            b.set_normalize(dt, scale, bias)
            if pad_value is not None:
                b.set_pad_value(pad_value)
        es = nm.ESIZE[dt] if dt else 1
        assert [b.output_size(i) for i in range(3)] == [w * h * es for w, h in canv]
        b.upload(); b.decode()
        outs, st = b.download()
        timed, _ = b.decode_timed()
        b.sync()
    assert st == [0, 0, 0] and "resize" in timed
    LAUNCHED.add(("pjd_k_resize_gray" if filt == "bilinear" else "pjd_k_resize_gray_tab", dt, filt))
    for i, n in enumerate(RESIZE_NAMES):
        p3 = np.repeat(planes[n][1][:, :, None], 3, axis=2)
        (w, h) = canv[i]
        C = pm.padded(p3, wins[i], w, h, pads[i], fill, oris[i], filt)
        assert np.array_equal(C[..., 0], C[..., 1])
        if not dt:
            _same(outs[i], np.ascontiguousarray(C[..., 0]), (n, filt, form, "u8"))
        else:
            want = pm.normalized(C, w, h, pads[i], dt, [scale[0]] * 3, [bias[0]] * 3, pad_value)[..., 0]
            assert outs[i].shape == (h, w), (outs[i].shape, h, w)
            assert np.array_equal(nm.bits(outs[i]), nm.bits(want)), (n, filt, form, dt)


@pytest.mark.parametrize("filt", ["bilinear", "antialias", "bicubic"])
def test_resize_filters_forms_and_element_types(ctx, planes, filt):
    import normalize_model as nm
    k = 0
    for form in FORMS:
        for dt in (0, nm.DT_F16, nm.DT_BF16, nm.DT_F32):
            _resize_case(ctx, planes, filt, form, dt, k)
            k += 1
    kernel = "pjd_k_resize_gray" if filt == "bilinear" else "pjd_k_resize_gray_tab"
    assert {(kn, dt) for kn, dt, f in LAUNCHED if f == filt} == {(kernel, dt) for dt in (0, 1, 2, 3)}


def test_resize_of_flagged_and_scaled_pictures(ctx, planes):
    """The resample reads the plane the back end wrote, whichever kernel wrote it: libjpeg's luma, a box-scaled plane."""
    import pjd_amd
    import resize_pad_model as pm
    lj = "lj_136x72_420_q90"
    sc = [_lj(lj), _scanned(golden_bytes(RESIZE_NAMES[0]), pjd_amd.F_SCALE_1_2)]
    src = [G.l8(lj), G.box1(planes[RESIZE_NAMES[0]][1], 2)]
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.set_resize([(31, 50), (19, 27)])
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.upload(); b.capture()
        for _ in range(2):
            b.decode(); b.sync()
            outs, st = b.download()
            for o, p, (h, w) in zip(outs, src, [(31, 50), (19, 27)]):
                _same(o, np.ascontiguousarray(pm.padded(np.repeat(p[:, :, None], 3, axis=2), None, w, h, (0, 0, 0, 0), (0, 0, 0), 1, "antialias")[..., 0]), (h, w))


# ---- 7: refusals leave the context usable --------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx, planes):
    import pjd_amd
    good = _scanned(golden_bytes("env_61x45_420_q100_opt"))

    def raises(code, fn, *a, **kw):
        with pytest.raises(pjd_amd.PjdError) as e:
            fn(*a, **kw)
        assert f"({code})" in str(e.value), str(e.value)
        return str(e.value)

    rst = _scanned(golden_bytes("rst4_128x96_444"))                  # kept: its descriptor lies in memory the Scanned owns
    raises(E_ARG, pjd_amd.split_decode, rst.desc, [0, 0], pjd_amd.OUT_GRAY8)
    for flag in (pjd_amd.F_SCALE_1_2, pjd_amd.F_SCALE_1_4, pjd_amd.F_SCALE_1_8):
        bad = _lj("lj_136x72_420_q90", flag)
        assert "image 1" in raises(E_ARG, ctx.batch, [good.desc, bad.desc], pjd_amd.OUT_GRAY8)
    h1v2 = _scanned(golden_bytes("h1v2_48x64"), pjd_amd.F_LIBJPEG)
    assert "image 1" in raises(E_ARG, ctx.batch, [good.desc, h1v2.desc], pjd_amd.OUT_GRAY8)
    raises(E_ARG, ctx.batch, [good.desc], 3)                         # 3 stays no format
    # what a planar batch refuses: a resize on a shard, a target of 0, an antialiased shrink beyond 16x, non-finite constants (all six
    # are validated, though entries [1] and [2] are ignored)
    shard = _scanned(golden_bytes("rst4_128x96_444"))
    shard.desc.shard_first_seg, shard.desc.shard_n_segs = 0, 1
    with ctx.batch([shard.desc], pjd_amd.OUT_GRAY8) as b:
        assert "shard" in raises(E_ARG, b.set_resize, [(8, 8)])
        assert "shard" in raises(E_ARG, b.set_normalize, pjd_amd.DT_F16, [1.0] * 3, [0.0] * 3)
    with ctx.batch([good.desc], pjd_amd.OUT_GRAY8) as b:
        raises(E_ARG, b.set_resize, [(0, 8)])
        b.set_resize([(2, 3)])
        raises(E_STATE, b.set_resize, [(2, 3)])
        assert "16x" in raises(E_ARG, b.set_resize_filter, pjd_amd.RESIZE_ANTIALIAS)
        raises(E_ARG, b.set_normalize, pjd_amd.DT_F32, [1.0, 1.0, float("inf")], [0.0] * 3)
        raises(E_ARG, b.set_normalize, 9, [1.0] * 3, [0.0] * 3)
        raises(E_STATE, b.set_pad_value, [0.0] * 3)
    # a misaligned normalised bind: element alignment applies (a child process: the address must be torch's)
    _torch_case("misaligned_bind")
    with ctx.batch([good.desc], pjd_amd.OUT_GRAY8) as b:
        raises(E_STATE, b.set_resize_filter, pjd_amd.RESIZE_ANTIALIAS)      # no resize set
        raises(E_ARG, b.bind_output, 0, 1 << 20)                     # a null pointer
        b.upload()
        raises(E_STATE, b.bind_output, 1 << 12, 1 << 20)             # after upload
        b.decode()
        outs, st = b.download()
        _same(outs[0], planes["env_61x45_420_q100_opt"][1], "after the refusals")
    outs, st = ctx.decode([good.desc], pjd_amd.OUT_GRAY8)
    assert st == [0]
    _same(outs[0], planes["env_61x45_420_q100_opt"][1], "context")


# ---- 8: the pipelined batcher ----------------------------------------------------------------------------------------------------------
def test_pipeline_gray_sink_payloads(planes):
    import pjd_amd
    names = sorted(MANIFEST)
    got, lock = {}, threading.Lock()

    def sink(index, name, log, status, data):
        with lock:
            got[index] = (status, None if data is None else data.copy())

    st = pjd_amd.pipe_run(jpegs=[golden_bytes(n) for n in names], names=[n + ".jpg" for n in names], out_format=pjd_amd.OUT_GRAY8,
                          batch_images=7, slots=2, sink=sink)
    assert st["n_decoded"] == len(VALID) and st["n_batch_failures"] == 0
    assert st["out_bytes"] == sum(p.size for _, p in planes.values())
    for i, n in enumerate(names):
        status, data = got[i]
        if MANIFEST[n]["rc"] != 0:
            assert status == -1 and data is None, n
            continue
        assert status == planes[n][0], n
        assert data.size == planes[n][1].size and np.array_equal(data, planes[n][1].reshape(-1)), n


def test_packed_download_is_a_third(ctx, planes):
    import pjd_amd
    names = [n for n in VALID if n.startswith("env_")][:24]
    sc = [_scanned(golden_bytes(n)) for n in names]
    with ctx.batch([s.desc for s in sc], pjd_amd.OUT_GRAY8) as b:
        b.upload(); b.decode()
        outs, st = b.download_packed()
        offs = [b.output_offset(i) for i in range(b.n)]
        size = b.packed_size()
    assert all(o % 256 == 0 for o in offs) and size % 256 == 0
    for n, o in zip(names, outs):
        assert np.array_equal(o, planes[n][1].reshape(-1)), n


# ---- 9: pjd_amd.tensors ------------------------------------------------------------------------------------------------------------------
def test_tensor_entry_points():
    """decode_to_tensors(gray=True): views (1, h, w); decode_to_batch_tensor(gray=True): uint8 [N, 1, H, W]; with and without libjpeg=True."""
    _torch_case("tensors")


def test_resizing_tensor_entry_points():
    """decode_resized_batch_tensor(gray=True): uint8 [N, 1, H, W]; decode_normalized_batch_tensor(gray=True): fp16 / bf16 / fp32
    [N, 1, H, W] with scalar mean, std, fill and pad_value; crops, flips, orientations, letterbox, the filters and libjpeg=True compose."""
    _torch_case("resized_tensors")
