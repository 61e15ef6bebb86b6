"""PJD_F_LIBJPEG on the GPU (run with -m gpu on an MI355X): every fixture under tests/golden/libjpeg/ equals Pillow's recorded decode byte
for byte -- zero tolerance, no case left out -- on the parallel path and the exact kernel, in the three output formats; flagged and
unflagged pictures in one batch; a truncated stream; int16-extreme hand-built units against pjd_libjpeg_idct; poisoned memory;
every refusal of the envelope; a captured graph.  The cases that need torch (bound output, resize / normalise / orientation on top of
the libjpeg picture) run in child processes: tests/libjpeg_torch_cases.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import libjpeg_model as M
from test_gpu_poisoned_memory import _fmt, _same
from test_libjpeg_cpu import fixture, manifest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(manifest()["cases"])
BIG = "lj_136x72_420_q90"


def scanned(name, extra=0, flag=True):
    import pjd_amd
    data, rgb, c = fixture(name)
    s = pjd_amd.Scanned(data, options=pjd_amd.SCAN_PROGRESSIVE if c["progressive"] else 0)
    assert s.valid, (name, s.log)
    s.desc.flags = int(s.desc.flags) | (pjd_amd.F_LIBJPEG if flag else 0) | extra
    return s, rgb


def desc_qts(desc):
    """The quantisers of a descriptor's components in natural order under the T.81 zigzag (entry 58 from qt_slot48)."""
    out = []
    for c in range(desc.num_components):
        t = desc.comp_qt[c]
        q = np.array(desc.qt[t][:], np.int64)
        q[58] = desc.qt_slot48[t]
        out.append(q)
    return out


@pytest.fixture
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", ["rgb8", "planar", "bmp"])
@pytest.mark.parametrize("path", ["parallel", "sequential"])
def test_every_fixture_equals_pillows_decode(ctx, path, fmt):
    """All 17 fixtures in one batch.  parallel: the lane streams (the progressive file takes the dense path, as always); sequential:
    PJD_F_FORCE_SEQUENTIAL, the exact kernel and the dense front end for every picture."""
    import pjd_amd
    sc = [scanned(n, pjd_amd.F_FORCE_SEQUENTIAL if path == "sequential" else 0) for n in NAMES]
    with ctx.batch([s.desc for s, _ in sc], _fmt(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
    assert list(st) == [0] * len(NAMES)
    for n, (_, rgb), got in zip(NAMES, sc, outs):
        _same(got, rgb, fmt, n)
    assert info["n_fallback"] == 0, info["flag_waves"]
    n_prog = sum(manifest()["cases"][n]["progressive"] for n in NAMES)
    assert info["n_sequential"] == (len(NAMES) if path == "sequential" else n_prog)
    # the 136 x 72 pictures span several back-end ranges (PJD_IDCT_MAX_DU = 96 units each): boundaries inside and between MCU rows
    big = sc[NAMES.index(BIG)][0]                     # (a Scanned owns what its descriptor points to: it has to stay alive)
    assert pjd_amd.plan_info([big.desc])["n_data_units"] == 270 > 2 * 96


def test_flagged_and_unflagged_pictures_in_one_batch(ctx, port):
    """Interleaved in one batch: the flagged pictures are libjpeg's, the unflagged ones the oracle port's, as in a batch without the
    flag; the two launches are named in the timed decode, and only there; the plane buffer is counted."""
    import pjd_amd
    from conftest import golden_bytes
    plain = ["env_64x48_420_q100", "rst4_128x96_444", "env_17x9_444_q85", "env_61x45_422_q30"]
    flagged = [BIG, "lj_40x24_422_q90", "lj_8x8_444_q90", "lj_61x45_grey_q50"]
    items, want = [], []
    for p, f in zip(plain, flagged):
        d = golden_bytes(p)
        s = pjd_amd.Scanned(d)
        items.append(s); want.append(port.decode(d)["rgb"])
        s2, rgb = scanned(f)
        items.append(s2); want.append(rgb)
    with ctx.batch([s.desc for s in items]) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        for k, (g, w) in enumerate(zip(outs, want)):
            assert np.array_equal(g, w), k
        timed, _ = b.decode_timed()
        b.sync()
        again, _ = b.download()
        assert all(np.array_equal(g, w) for g, w in zip(again, want))
        mixed_bytes = b.info()["device_bytes"]
    assert list(st) == [0] * len(items)
    assert "idct_std" in timed and "colour_std" in timed and "idct_colour" in timed, timed
    with ctx.batch([s.desc for s in items[0::2]]) as b:
        b.upload()
        timed0, _ = b.decode_timed()
        b.sync()
        plain_bytes = b.info()["device_bytes"]
    assert not any("_std" in x for x in timed0), timed0
    assert mixed_bytes > plain_bytes + 136 * 72 * 3 // 2


def _truncated():
    """lj_33x31_420_q100 (3 x 2 MCUs, dense) with its entropy-coded data cut to a fifth: the error lies in the first MCU row."""
    data, _, _ = fixture("lj_33x31_420_q100")
    body = data.rfind(b"\xff\xda") + 14
    n = len(data) - 2 - body
    return data[:body + n // 5] + b"\xff\xd9"


def test_truncated_stream(ctx):
    """The status is the default mode's; the picture is the model over the coefficients the decoder kept (zero behind the error), and
    grey (128) in the MCU row behind the one the error lies in (from its third pixel row on: fancy upsampling leans one chroma row up)."""
    import pjd_amd
    data = _truncated()
    for extra in (0, pjd_amd.F_FORCE_SEQUENTIAL):
        s = pjd_amd.Scanned(data)
        s.desc.flags = int(s.desc.flags) | pjd_amd.F_LIBJPEG | extra
        r = pjd_amd.Scanned(data)
        r.desc.flags = int(r.desc.flags) | pjd_amd.F_STANDARD_ZIGZAG | pjd_amd.F_STANDARD_RESTART | extra
        with ctx.batch([s.desc, r.desc]) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            coef = b.coefficients(0)
            assert np.array_equal(coef, b.coefficients(1))
        assert st[0] == st[1] != 0
        d = s.desc
        want = M.decode(coef, desc_qts(d), d.width, d.height, d.num_components, d.h_samp, d.v_samp)
        assert np.array_equal(outs[0], want), extra
        assert (outs[0][18:] == 128).all() and not (outs[0][:8] == 128).all()


@functools.lru_cache(maxsize=1)
def _edge_items():
    """The int16-edge family of tests/symbol_corpus.py inside the mode's envelope: absolute DCs and dequantised products at the int16
    extremes, quantisers up to 65535 -- beyond what libjpeg defines, where the mode is pinned to pjd_libjpeg_idct."""
    import symbol_corpus as SC
    out = []
    for name, (data, fr, it) in sorted(SC.edge_family().items()):
        if (fr.hs, fr.vs) == (1, 2) or len(fr.comps) == 2:
            continue
        if fr.ri and not fr.standard_restart and (fr.hs, fr.vs) != (1, 1):
            continue                                   # written for the reference's restart rule: the flag implies T.81's
        out.append((name, data))
    return out


def _host_picture(coef, d):
    """The picture from the HOST entry points: pjd_libjpeg_idct per unit, then the model's upsampling and colour (which
    tests/test_libjpeg_cpu.py holds equal to pjd_libjpeg_upsample_row and pjd_libjpeg_ycc_to_rgb)."""
    import pjd_amd
    qts = desc_qts(d)
    grids = M.unit_grids(coef, d.width, d.height, d.num_components, d.h_samp, d.v_samp)
    planes = []
    for c, g in enumerate(grids):
        s = np.zeros(g.shape[:2] + (8, 8), np.uint8)
        for y in range(g.shape[0]):
            for x in range(g.shape[1]):
                s[y, x] = pjd_amd.libjpeg_idct(g[y, x], (qts[c] & 0xffff).astype(np.uint16)).reshape(8, 8)
        planes.append(M.plane_from_units(s))
    W, H = d.width, d.height
    yp = planes[0][:H, :W]
    if d.num_components == 1:
        return np.stack([yp, yp, yp], axis=-1)
    return M.ycc_to_rgb(yp, M.upsample(planes[1], W, H, d.h_samp, d.v_samp), M.upsample(planes[2], W, H, d.h_samp, d.v_samp))


@pytest.mark.parametrize("path", ["parallel", "sequential"])
def test_int16_extreme_units_equal_the_host_function(ctx, path):
    import pjd_amd
    items = _edge_items()
    assert len(items) >= 4
    sc = []
    for _, data in items:
        s = pjd_amd.Scanned(data)
        assert s.valid
        s.desc.flags = int(s.desc.flags) | pjd_amd.F_LIBJPEG | (pjd_amd.F_FORCE_SEQUENTIAL if path == "sequential" else 0)
        sc.append(s)
    extreme = 0
    with ctx.batch([s.desc for s in sc]) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        for k, ((name, _), s) in enumerate(zip(items, sc)):
            coef = b.coefficients(k)
            extreme += int((coef == -32768).any() or (coef == 32767).any())
            assert np.array_equal(outs[k], _host_picture(coef, s.desc)), (name, path)
    assert extreme >= 2


@pytest.mark.parametrize("fmt", ["rgb8", "planar", "bmp"])
def test_poisoned_memory_changes_nothing(monkeypatch, fmt):
    """PJD_DEBUG_POISON = 0x00 and 0xA5: every allocation of the context starts filled with the byte; the pictures are the fixtures'
    either way -- the plane buffer and every picture range are written whole by every decode, the second decode included."""
    import pjd_amd
    results = []
    for byte in ("0x00", "0xa5"):
        monkeypatch.setenv("PJD_DEBUG_POISON", byte)
        c = pjd_amd.Context(0)
        try:
            sc = [scanned(n) for n in NAMES]
            with c.batch([s.desc for s, _ in sc], _fmt(fmt)) as b:
                b.upload()
                for _ in range(2):
                    b.decode(); b.sync()
                    outs, st = b.download()
                    assert list(st) == [0] * len(NAMES)
                    for n, (_, rgb), got in zip(NAMES, sc, outs):
                        _same(got, rgb, fmt, (n, byte))
            results.append([np.asarray(o).copy() for o in outs])
        finally:
            c.close()
    assert all(np.array_equal(a, b) for a, b in zip(*results))


def test_refusals_leave_the_context_usable(ctx):
    """PJD_E_ARG (-3) at pjd_batch_create, the picture named: the flag with an output scale, with 4:4:0 sampling, on a shard; and
    pjd_split_decode.  A good batch on the same context afterwards decodes."""
    import pjd_amd
    from conftest import golden_bytes
    good, rgb = scanned(BIG)

    def refused(desc, index_word):
        with pytest.raises(pjd_amd.PjdError) as e:
            ctx.batch([good.desc, desc])
        assert "(-3)" in str(e.value) and index_word in str(e.value), str(e.value)

    for flag in (pjd_amd.F_SCALE_1_2, pjd_amd.F_SCALE_1_4, pjd_amd.F_SCALE_1_8):
        s, _ = scanned(BIG, flag)                     # (a Scanned owns what its descriptor points to: it has to stay alive)
        refused(s.desc, "image 1")
    h1v2 = pjd_amd.Scanned(golden_bytes("h1v2_48x64"))
    assert h1v2.valid and (h1v2.desc.h_samp, h1v2.desc.v_samp) == (1, 2)
    h1v2.desc.flags = int(h1v2.desc.flags) | pjd_amd.F_LIBJPEG
    refused(h1v2.desc, "image 1")
    shard, _ = scanned(BIG + "_rst4")
    assert shard.desc.n_segments >= 2
    shard.desc.shard_first_seg, shard.desc.shard_n_segs = 0, 1
    refused(shard.desc, "image 1")
    whole, _ = scanned(BIG + "_rst4")
    with pytest.raises(pjd_amd.PjdError) as e:
        pjd_amd.split_decode(whole.desc, [0, 0])
    assert "(-3)" in str(e.value)
    outs, st = ctx.decode([good.desc])
    assert st[0] == 0 and np.array_equal(outs[0], rgb)


def test_captured_graph_replayed_twice(ctx):
    import pjd_amd
    sc = [scanned(n) for n in NAMES]
    with ctx.batch([s.desc for s, _ in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.upload(); b.decode(); b.sync()
        direct, st = b.download()
        b.capture()
        for _ in range(2):
            b.decode(); b.sync()
            outs, st2 = b.download()
            assert list(st2) == list(st) == [0] * len(NAMES)
            assert all(np.array_equal(a, c) for a, c in zip(outs, direct))
    for (_, rgb), got in zip(sc, direct):
        _same(got, rgb, "planar", "graph")


def _torch_case(case, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "libjpeg_torch_cases.py"), case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


def test_bound_output_through_decode_to_tensors():
    _torch_case("bound_output")


def test_resize_normalize_and_orientation_read_the_libjpeg_picture():
    _torch_case("composition")
