"""The picture-group form of a decode under every output path (run with -m gpu on an MI355X).

A batch of 64 or more small pictures decoded alone on an idle device forks into three chains of launches on three streams (entropy
decode, pjd_k_group_dc, the back end over a slice of iwg_order), which join the context's stream in front of the exact path and the
resample.  Everything that runs behind that join -- resize in its three filters, windows, orientations, pad and its border launch, the
affine warp, the colour map, normalised output, views, bound output, the exact path, the fallback of pjd_batch_sync -- is pinned
elsewhere on batches of 3 to 20 pictures, which take the single chain.  Here the 85 pictures of tests/group_corpus.py go through each of
them in the grouped form, and the form is asserted, not assumed: Batch.decode_chains() is 3 after the grouped leg and 1 after the same
request is decoded once more as the single chain (decode_timed always takes it), whose bytes must be the same.

Every context is opened with PJD_DEBUG_POISON=0xa5, so a range of the intermediate that no group's back end wrote shows; no case keeps
another batch with groups alive; every output is compared, byte for byte (bit for bit for floats), and no expectation comes from the
library: the oracle port's pictures and status words, gray_expected.ref_plane for grey, the box filters for the scales, and the numpy
models of the resample behind them.  tests/test_group_forms_cpu.py asserts without a GPU that every batch here plans three groups and
that every request is accepted."""
import contextlib

import numpy as np
import pytest

import colour_model
import gray_expected as GE
import group_corpus as G
import normalize_model as nm
import resize_pad_model as pm
import warp_model
from conftest import golden_bytes

pytestmark = pytest.mark.gpu

FILL = G.FILL
DTYPES = (0, nm.DT_F16, nm.DT_BF16, nm.DT_F32)
DT_NAME = {0: "u8", nm.DT_F16: "f16", nm.DT_BF16: "bf16", nm.DT_F32: "f32"}
DONOR = "big_640x480_420_q85"                               # 921 600 bytes of caller-owned memory with a picture in them


@contextlib.contextmanager
def _context(monkeypatch, plan_mode=None, **env):
    """A context of the case's own: poisoned allocations, the planner's switches off, then what the case sets."""
    import pjd_amd
    for k in G.ENV_OFF:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PJD_DEBUG_POISON", "0xa5")
    c = pjd_amd.Context(0) if plan_mode is None else pjd_amd.Context(0, plan_mode=plan_mode)
    try:
        yield c
    finally:
        c.close()


def _constants():
    from pjd_amd import tensors
    return tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)


@pytest.fixture(scope="module")
def oracle(port):
    """data -> (status, H x W x 3 picture, H x W grey plane) of the oracle, computed once per stream and read-only."""
    cache = {}

    def get(data):
        if data not in cache:
            o = port.decode(data)
            st, plane = GE.ref_plane(port, data)
            assert st == o["huff_rc"]
            for a in (o["rgb"], plane):
                a.setflags(write=False)
            cache[data] = (o["huff_rc"], o["rgb"], plane)
        return cache[data]
    for j in G.jpegs():
        get(j)
    assert [get(j)[0] != 0 for j in G.jpegs()] == [False] * 83 + [True] * 2, "the two damaged copies, and only they, end in an error"
    return get


def _source(src, fmt):
    """(status, picture as H x W x 3) for the models: a grey batch's plane three times over"""
    st, rgb, plane = src
    return st, (np.repeat(plane[:, :, None], 3, axis=2) if fmt == "gray" else rgb)


def _layout(hwc, fmt):
    return np.ascontiguousarray(hwc[..., 0] if fmt == "gray" else hwc.transpose(2, 0, 1) if fmt == "planar" else hwc)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(nm.bits(got) != nm.bits(want)) if got.dtype != np.uint8 else np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing sample", bad[0].tolist(), "differing", len(bad), "of", got.size)


def _both_forms(b, wants, want_st, what, groups=3):
    """Decode as the picture groups, then the same request as the single chain: the form of each, every output against `wants`, the
    statuses, and the second leg's bytes equal to the first's.  -> the outputs of the grouped leg"""
    assert b.decode_chains() == 0
    b.decode(); b.sync()
    assert b.decode_chains() == groups, (what, "the decode did not take the picture groups", b.decode_chains(), b.info()["dc_plan"] >> 8)
    outs, st = b.download()
    assert st == want_st, (what, [(i, s, w) for i, (s, w) in enumerate(zip(st, want_st)) if s != w])
    assert len(outs) == len(wants)
    for k, (o, w) in enumerate(zip(outs, wants)):
        _same(o, w, (what, "groups", k))
    b.decode_timed(); b.sync()
    assert b.decode_chains() == 1, what
    outs1, st1 = b.download()
    assert st1 == st
    for k, (o, w) in enumerate(zip(outs1, outs)):
        assert o.tobytes() == w.tobytes(), (what, "the single chain differs from the groups at output", k)
    return outs


# ---- a: grey, the scales cycling ----------------------------------------------------------------------------------------------------------------
def test_grey_with_every_scale_direct_and_replayed(monkeypatch, oracle):
    """PJD_OUT_GRAY8 with PJD_F_SCALE_* cycling 1, 1/2, 1/4, 1/8 per picture: the grey back end behind three chains, direct, and captured
    then replayed twice (the replay launches the graph with the parallel branches)."""
    jp = G.jpegs()
    cyc = G.scale_cycle()
    sc = G.scan(jp, [f for f, _ in cyc])
    wants = [GE.box1(oracle(j)[2], s) for j, (_, s) in zip(jp, cyc)]
    want_st = [oracle(j)[0] for j in jp]
    with _context(monkeypatch) as ctx:
        with ctx.batch([s.desc for s in sc], G.out_format("gray")) as b:
            b.upload()
            _both_forms(b, wants, want_st, "grey direct")
        with ctx.batch([s.desc for s in sc], G.out_format("gray")) as b:
            b.upload(); b.capture()
            assert b.decode_chains() == 0, "a capture is no decode"
            for rep in range(2):
                b.decode(); b.sync()
                assert b.decode_chains() == 3, rep
                outs, st = b.download()
                assert st == want_st
                for k, (o, w) in enumerate(zip(outs, wants)):
                    _same(o, w, ("grey replay", rep, k))


# ---- b, g: resize behind the join -------------------------------------------------------------------------------------------------------------
def _resize_batch(ctx, scanned, fmt, req, filt, dtype=0, pad_value=None):
    b = ctx.batch([s.desc for s in scanned], G.out_format(fmt))
    b.set_resize([r["canvas"] for r in req])
    if any(any(r["pad"]) for r in req):
        b.set_resize_pad([r["pad"] for r in req], FILL)
    if any(r["o"] != 1 for r in req):
        b.set_orientation([r["o"] for r in req])
    if any(r["win"] for r in req):
        b.set_resize_window([r["win"] for r in req])
    if filt != "bilinear":
        b.set_resize_filter(G.filter_id(filt))
    if dtype:
        scale, bias = _constants()
        b.set_normalize(dtype, scale, bias)
        if pad_value is not None:
            b.set_pad_value(pad_value)
    return b


def _resize_want(src, r, fmt, filt, dtype=0, pad_value=None):
    """The model's output for one picture (status, rgb, plane) under the request record r."""
    _, P = _source(src, fmt)
    out_h, out_w = r["canvas"]
    fill = (FILL[0],) * 3 if fmt == "gray" else FILL                       # a grey batch reads the first fill byte
    C = pm.padded(P, r["win"], out_w, out_h, r["pad"], fill, r["o"], filt)
    if dtype:
        scale, bias = _constants()
        if fmt == "gray":                                                  # ... and the first scale, bias and pad value
            scale, bias = [scale[0]] * 3, [bias[0]] * 3
            pad_value = None if pad_value is None else (pad_value[0],) * 3
        C = pm.normalized(C, out_w, out_h, r["pad"], dtype, scale, bias, pad_value)
    return _layout(C, fmt)


def _resize_case(monkeypatch, oracle, filt, fmt, dtype, pad_value=None, plan_mode=None):
    jp = G.jpegs()
    sc = G.scan(jp)
    dims = [(int(s.desc.width), int(s.desc.height)) for s in sc]
    req = G.resize_request(dims, filt)
    wants = [_resize_want(oracle(j), r, fmt, filt, dtype, pad_value) for j, r in zip(jp, req)]
    with _context(monkeypatch, plan_mode) as ctx:
        with _resize_batch(ctx, sc, fmt, req, filt, dtype, pad_value) as b:
            b.upload()
            _both_forms(b, wants, [oracle(j)[0] for j in jp], (filt, fmt, DT_NAME[dtype]))
            info = b.info()
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0
    return info


RESIZE_CASES = [(filt, fmt, DTYPES[(i + j) % 4]) for i, filt in enumerate(G.FILTERS) for j, fmt in enumerate(G.FMTS)]


@pytest.mark.parametrize("filt,fmt,dtype", RESIZE_CASES, ids=["%s-%s-%s" % (f, m, DT_NAME[d]) for f, m, d in RESIZE_CASES])
def test_resize_behind_the_join(monkeypatch, oracle, filt, fmt, dtype):
    """Per picture: targets cycling through widths 1, 5, 37, 259 and heights 7, 9, 33 (a larger one where a table-driven filter's 16x
    limit asks for it), a window with PJD_RW_HFLIP on every third, the eight orientations, four pads of which one is all zero -- the
    padded kernels and the border launch behind three chains.  The element type walks through uint8, fp16, bf16 and fp32 over the nine
    cases: each layout meets three of the four, each type at least two layouts; one float case sets a pad value."""
    assert {d for _, m, d in RESIZE_CASES} == set(DTYPES) and all(len({d for _, m, d in RESIZE_CASES if m == fmt_}) == 3 for fmt_ in G.FMTS)
    pad_value = (0.25, -1.5, 3e-6) if (filt, fmt) == ("antialias", "planar") else None
    assert pad_value is None or dtype
    _resize_case(monkeypatch, oracle, filt, fmt, dtype, pad_value)


def test_resize_behind_the_join_under_the_throughput_plan(monkeypatch, oracle):
    """The bilinear, planar case once more in a context with PJD_PLAN_THROUGHPUT."""
    import pjd_amd
    info = _resize_case(monkeypatch, oracle, "bilinear", "planar", DTYPES[1], plan_mode=pjd_amd.PLAN_THROUGHPUT)
    assert info["plan_mode"] == pjd_amd.PLAN_THROUGHPUT


# ---- c: warp, colour, views, bound output ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["planar-bf16-colour", "rgb8-u8"])
def test_warp_colour_views_into_bound_memory(monkeypatch, oracle, form):
    """Two views per picture (170 outputs, views in a non-monotone order) of 33 x 33 and 37 x 9 under a seeded similarity each, one quarter
    turn and one view wholly outside; planar bf16 with the eight colour maps in turn, and interleaved uint8 without a map.  The outputs
    are bound 1, 2 and 3 elements off a multiple of four into a donor batch's picture, with gaps: every output is the model's and every
    byte outside the outputs is still the donor's, after the groups and after the single chain."""
    import pjd_amd
    fmt, dtype, coloured = ("planar", nm.DT_BF16, True) if form.startswith("planar") else ("rgb8", 0, False)
    es = nm.ESIZE[dtype] if dtype else 1
    jp = G.jpegs()
    sc = G.scan(jp)
    dims = [(int(s.desc.width), int(s.desc.height)) for s in sc]
    wr = G.warp_request(dims)
    scale, bias = _constants()
    wants = []
    for p, (tw, th), m, cm in zip(wr["views"], wr["sizes"], wr["mats"], wr["colours"]):
        u8 = warp_model.warp(np.ascontiguousarray(oracle(jp[p])[1].transpose(2, 0, 1)), m, tw, th, FILL)
        if coloured:
            u8 = colour_model.apply(cm, u8)
        out = np.stack([nm.table(dtype, scale[c], bias[c])[u8[c]] for c in range(3)]) if dtype else u8
        wants.append(np.ascontiguousarray(out if fmt == "planar" else out.transpose(1, 2, 0)))
    flat = wants[9].reshape(3, -1) if fmt == "planar" else wants[9].reshape(-1, 3).T
    assert (flat == flat[:, :1]).all(), "view 9 lies wholly outside its picture: the fill alone"
    with _context(monkeypatch) as ctx:
        donor_sc = G.scan([golden_bytes(DONOR)])
        with ctx.batch([donor_sc[0].desc], pjd_amd.OUT_RGB8) as donor:
            donor.upload(); donor.decode()
            (pattern,), _ = donor.download()
            pattern = pattern.reshape(-1).copy()
            mem, cap = donor.device_output(0), donor.output_size(0)
            with ctx.batch([s.desc for s in sc], G.out_format(fmt)) as b:
                b.set_views(wr["views"])
                b.set_resize([(th, tw) for tw, th in wr["sizes"]])
                b.set_resize_affine(wr["mats"], FILL)
                if coloured:
                    b.set_colour(wr["colours"])
                if dtype:
                    b.set_normalize(dtype, scale, bias)
                sizes = [b.output_size(i) for i in range(len(wants))]
                assert sizes == [w.nbytes for w in wants]
                offs, end = G.bound_offsets(sizes, es)
                assert end <= cap and sorted({(o // es) % 4 for o in offs}) == [1, 2, 3]
                b.bind_output(mem, cap, offs)
                b.upload()
                _both_forms(b, wants, [oracle(j)[0] for j in jp], form)
            (after,), _ = donor.download()
            after = after.reshape(-1)
    covered = np.zeros(cap, bool)
    for k, (w, off, size) in enumerate(zip(wants, offs, sizes)):
        assert after[off:off + size].tobytes() == w.tobytes(), k
        covered[off:off + size] = True
    stray = np.flatnonzero(~covered & (after != pattern))
    assert stray.size == 0, f"bytes outside every output were written, first at {stray[:8]}"


# ---- d: graph replay, idle and busy ------------------------------------------------------------------------------------------------------------
def test_replay_alone_and_beside_another_grouped_decode(monkeypatch, oracle):
    """Planar, bilinear to 37 x 29, normalised fp16, bound and captured.  Replayed alone it launches the graph with the parallel branches;
    after the bound memory was overwritten (the donor decoded again) a second replay rewrites every byte.  Replayed while a second
    grouped batch of another context is decoded and not yet synced, it launches the single chain's graph: the same bytes."""
    import pjd_amd
    jp = G.jpegs()
    sc = G.scan(jp)
    dims = [(int(s.desc.width), int(s.desc.height)) for s in sc]
    req = G.fixed_request(dims, 37, 29, "bilinear")
    wants = [_resize_want(oracle(j), r, "planar", "bilinear", nm.DT_F16) for j, r in zip(jp, req)]
    want_st = [oracle(j)[0] for j in jp]
    blob = b"".join(w.tobytes() for w in wants)

    def bound(donor):
        (a,), _ = donor.download()
        return a.reshape(-1)[:len(blob)].tobytes()
    with _context(monkeypatch) as ctx:
        other = pjd_amd.Context(0)
        try:
            donor_sc = G.scan([golden_bytes(DONOR)])
            with ctx.batch([donor_sc[0].desc], pjd_amd.OUT_RGB8) as donor, _resize_batch(ctx, sc, "planar", req, "bilinear", nm.DT_F16) as b:
                donor.upload(); donor.decode(); donor.sync()
                before = bound(donor)
                offs = np.concatenate([[0], np.cumsum([w.nbytes for w in wants])])[:-1].tolist()
                b.bind_output(donor.device_output(0), donor.output_size(0), offs)
                b.upload(); b.capture()
                assert b.decode_chains() == 0
                b.decode(); b.sync()
                assert b.decode_chains() == 3 and b.statuses() == want_st
                assert bound(donor) == blob and before != blob
                donor.decode(); donor.sync()                               # the bound memory holds the donor's picture again
                assert bound(donor) == before
                b.decode(); b.sync()
                assert b.decode_chains() == 3 and bound(donor) == blob, "the second replay rewrites every byte"
                donor.decode(); donor.sync()
                busy = other.batch([s.desc for s in sc], pjd_amd.OUT_RGB8)
                try:
                    busy.upload()
                    busy.decode()                                          # in flight, counted
                    b.decode()
                    busy.sync(); b.sync()
                    assert busy.decode_chains() == 3 and b.decode_chains() == 1
                    assert bound(donor) == blob and b.statuses() == want_st
                    outs, st = busy.download()
                    assert st == want_st
                    for k, (o, j) in enumerate(zip(outs, jp)):
                        _same(o, oracle(j)[1], ("busy", k))
                finally:
                    busy.destroy()
                b.decode(); b.sync()                                       # and alone again: the count came down
                assert b.decode_chains() == 3 and bound(donor) == blob
        finally:
            other.close()


# ---- e: the exact path inside a grouped batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "gray"])
def test_exact_path_inside_a_grouped_batch(monkeypatch, port, oracle, fmt):
    """Picture 11 flagged PJD_F_FORCE_SEQUENTIAL, a fixture routed up front inserted at 20 and a progressive frame at 60: the exact
    launches and the dense back end run on the main stream behind the join and in front of the resample (antialiased, to 41 x 30)."""
    import pjd_amd
    import progressive_corpus as PC
    from test_gpu_progressive_streams import expected as prog_expected, scan_progressive
    label, prog, fr = G.progressive_member()
    over = golden_bytes("huff_oversub_96x64_444")
    sc = G.scan(G.inserted(G.jpegs(), {20: over}), [pjd_amd.F_FORCE_SEQUENTIAL if k == 11 else 0 for k in range(86)])
    sc.insert(60, scan_progressive(prog))
    pst, pcoef, prgb = prog_expected(port, prog, fr)
    port.standard_zigzag(True)
    try:
        pplane = GE.ref_plane_of_coefficients(port, PC.twin(fr), pcoef)
    finally:
        port.standard_zigzag(False)
    srcs = [oracle(j) for j in G.inserted(G.jpegs(), {20: over})]
    srcs.insert(60, (pst, prgb, pplane))
    assert len(srcs) == len(sc) == 87 and pst == 0
    dims = [(int(s.desc.width), int(s.desc.height)) for s in sc]
    assert dims[20] == (96, 64) and dims[60] == (40, 24)
    req = G.fixed_request(dims, 41, 30, "antialias")
    wants = [_resize_want(s, r, fmt, "antialias") for s, r in zip(srcs, req)]
    with _context(monkeypatch) as ctx:
        with _resize_batch(ctx, sc, fmt, req, "antialias") as b:
            b.upload()
            _both_forms(b, wants, [s[0] for s in srcs], ("exact path", fmt))
            info = b.info()
    assert info["n_sequential"] == 3 and info["n_fallback"] == 0 and info["dc_plan"] >> 8 == 3, info


# ---- f: the fallback of pjd_batch_sync behind a grouped decode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["planar", "gray"])
def test_fallback_behind_a_grouped_decode(monkeypatch, oracle, fmt):
    """A stream the parallel decoder hands to the exact kernel in pjd_batch_sync, inserted at 40, lanes of 128 bytes: settle() decodes
    it again on the main stream and runs the whole resample (bilinear into a pad of one sample) a second time.  Twice over."""
    import fallback_corpus as F
    fall = F.falling()["lock_420_130"].data
    jp = G.inserted(G.jpegs(), {40: fall})
    sc = G.scan(jp)
    dims = [(int(s.desc.width), int(s.desc.height)) for s in sc]
    assert dims[40] == (208, 160)
    req = G.fixed_request(dims, 37, 29, "bilinear", (1, 1, 1, 1))
    wants = [_resize_want(oracle(j), r, fmt, "bilinear") for j, r in zip(jp, req)]
    want_st = [oracle(j)[0] for j in jp]
    with _context(monkeypatch, PJD_SUB_BYTES="128") as ctx:
        with _resize_batch(ctx, sc, fmt, req, "bilinear") as b:
            b.upload()
            for rep in range(2):
                b.decode(); b.sync()
                outs, st = b.download()
                info = b.info()
                assert info["n_fallback"] == 1 and info["n_sequential"] == 0 and info["sub_bytes"] == 128, (rep, info)
                assert b.decode_chains() == 3, (rep, "the fallback leaves the form alone")
                assert st == want_st
                for k, (o, w) in enumerate(zip(outs, wants)):
                    _same(o, w, ("fallback", fmt, rep, k))
            b.decode_timed(); b.sync()
            outs1, st1 = b.download()
            assert b.decode_chains() == 1 and b.info()["n_fallback"] == 1 and st1 == want_st
            for k, (o, w) in enumerate(zip(outs1, outs)):
                assert o.tobytes() == w.tobytes(), (fmt, "the single chain differs from the groups at output", k)
