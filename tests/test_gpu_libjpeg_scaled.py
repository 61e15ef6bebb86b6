"""PJD_F_LIBJPEG_SCALE_* on the GPU (run with -m gpu on an MI355X): every fixture under tests/golden/libjpeg_scaled/ at 1/2, 1/4 and 1/8
equals Pillow's recorded draft decode byte for byte -- zero tolerance -- as RGB8, planar, BMP and GRAY8, on the lane streams and under
PJD_F_FORCE_SEQUENTIAL (the progressive file takes the dense front end either way).  The "model only" scales (an axis shorter than s:
Pillow cannot be made to take them; the list is fixed in tests/test_libjpeg_scaled_cpu.py) equal the model of include/pjd.h over the
decoder's own coefficients.  A mixed batch, a truncated stream, a second decode and a graph replay, the timed names, device_bytes.  The
cases that need torch (bound output into a poisoned tensor, draft=True through resize and normalise) run in child processes:
tests/libjpeg_scaled_torch_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libjpeg_scaled_model as SM
from test_gpu_poisoned_memory import _fmt, _same
from test_gpu_scaled import box
from test_libjpeg_scaled_cpu import FLAG, MODEL_ONLY, jpeg, manifest, recording

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(manifest()["cases"])
REDUCED = (2, 4, 8)
BIG = "ls_136x72_420_q90"


def scanned(name, s=1, extra=0, flag=True):
    import pjd_amd
    c = manifest()["cases"][name]
    sc = pjd_amd.Scanned(jpeg(name), options=pjd_amd.SCAN_PROGRESSIVE if c["progressive"] else 0)
    assert sc.valid, (name, sc.log)
    sc.desc.flags = int(sc.desc.flags) | ((pjd_amd.F_LIBJPEG | FLAG[s]) if flag else 0) | extra
    return sc


def desc_qts(desc):
    """The quantisers of a descriptor's components in natural order under the T.81 zigzag (entry 58 from qt_slot48)."""
    out = []
    for c in range(desc.num_components):
        t = desc.comp_qt[c]
        q = np.array(desc.qt[t][:], np.int64)
        q[58] = desc.qt_slot48[t]
        out.append(q)
    return out


def model(coef, d, s, gray=False):
    return SM.decode(coef, desc_qts(d), d.width, d.height, d.num_components, d.h_samp, d.v_samp, s, gray)


def expected(name, s, gray, batch, k, desc):
    """Pillow's recording, or for a model-only scale the model over the coefficients picture k of the batch decoded."""
    want = recording(name, s, "l8" if gray else "rgb")
    if want is None:
        assert (name, s) in MODEL_ONLY
        want = model(batch.coefficients(k), desc, s, gray)
    return want


def same(got, want, fmt, label):
    if fmt == "gray":
        got = np.asarray(got)
        assert got.shape == want.shape, (label, got.shape, want.shape)
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, (label, "first differing byte", int(bad[0]), "of", want.size, "differing", int(bad.size))
    else:
        _same(got, want, fmt, label)


def fmt_of(fmt):
    import pjd_amd
    return pjd_amd.OUT_GRAY8 if fmt == "gray" else _fmt(fmt)


@pytest.fixture
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", ["rgb8", "planar", "bmp", "gray"])
@pytest.mark.parametrize("path", ["parallel", "sequential"])
def test_every_fixture_at_every_reduced_scale(ctx, path, fmt):
    """16 fixtures x 3 scales in one batch.  parallel: the lane streams (the progressive file: PJD_F_PROGRESSIVE, the dense front end);
    sequential: PJD_F_FORCE_SEQUENTIAL, the exact kernel and the dense front end for every picture."""
    import pjd_amd
    items = [(n, s) for n in NAMES for s in REDUCED]
    sc = [scanned(n, s, pjd_amd.F_FORCE_SEQUENTIAL if path == "sequential" else 0) for n, s in items]
    with ctx.batch([x.desc for x in sc], fmt_of(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
        assert list(st) == [0] * len(items)
        n_model = 0
        for k, ((n, s), x) in enumerate(zip(items, sc)):
            c = manifest()["cases"][n]
            ow, oh = -(-c["width"] // s), -(-c["height"] // s)
            assert b.output_size(k) == {"rgb8": 3 * ow * oh, "planar": 3 * ow * oh, "gray": ow * oh, "bmp": 26 + oh * (3 * ow + ow % 4)}[fmt]
            want = expected(n, s, fmt == "gray", b, k, x.desc)
            n_model += (n, s) in MODEL_ONLY
            same(outs[k], want, fmt, (n, s, path))
    assert n_model == len(MODEL_ONLY) == 8
    assert info["n_fallback"] == 0, info["flag_waves"]
    assert info["n_sequential"] == (len(items) if path == "sequential" else 3 * sum(manifest()["cases"][n]["progressive"] for n in NAMES))
    # 259 x 19 4:2:2 and 136 x 72 4:2:0 span several back-end ranges (PJD_IDCT_MAX_DU = 96 units each)
    wide = scanned("ls_259x19_422_q50")
    assert pjd_amd.plan_info([wide.desc])["n_data_units"] > 2 * 96


def test_model_equals_the_decoder_on_the_restart_and_the_progressive_file(ctx):
    """The two fixtures the oracle port does not read (tests/test_libjpeg_scaled_cpu.py): the model over the decoder's coefficients is
    Pillow's recording at every scale, RGB and L."""
    names = [n for n in NAMES if manifest()["cases"][n]["progressive"] or manifest()["cases"][n]["restart_marker_blocks"]]
    assert len(names) == 2
    sc = [scanned(n) for n in names]
    with ctx.batch([x.desc for x in sc]) as b:
        b.upload(); b.decode(); b.sync()
        assert list(b.statuses()) == [0, 0]
        for k, (n, x) in enumerate(zip(names, sc)):
            coef = b.coefficients(k)
            for s in (1, 2, 4, 8):
                assert np.array_equal(model(coef, x.desc, s), recording(n, s, "rgb")), (n, s)
                assert np.array_equal(model(coef, x.desc, s, True), recording(n, s, "l8")), (n, s)


def _mixed(port):
    """Flagged pictures at all four scales, unflagged full-size and box-scaled ones, interleaved -> (Scanned, expected H x W x 3)."""
    import pjd_amd
    from conftest import golden_bytes
    items, want = [], []
    flagged = [(BIG, 1), ("ls_259x19_422_q50", 2), ("ls_136x72_420_q100_rst4", 4), (BIG, 8), ("ls_40x24_422_q90", 1), ("ls_33x31_420_q90_prog", 2),
               ("ls_61x45_grey_q50", 4), ("ls_17x17_420_q100", 8), ("ls_8x8_444_q90", 2), ("ls_33x31_420_q90", 4)]
    plain = [("env_64x48_420_q100", 1), ("rst4_128x96_444", 4), ("env_17x9_444_q85", 2), ("env_61x45_422_q30", 8), ("env_61x45_422_q30", 1)]
    for k, (n, s) in enumerate(flagged):
        items.append(scanned(n, s)); want.append(recording(n, s, "rgb"))
        if k < len(plain):
            p, ps = plain[k]
            d = golden_bytes(p)
            x = pjd_amd.Scanned(d)
            x.desc.flags = int(x.desc.flags) | {1: 0, 2: pjd_amd.F_SCALE_1_2, 4: pjd_amd.F_SCALE_1_4, 8: pjd_amd.F_SCALE_1_8}[ps]
            items.append(x); want.append(box(port.decode(d)["rgb"], ps))
    return items, want


@pytest.mark.parametrize("fmt", ["rgb8", "planar"])
def test_mixed_batch_decoded_twice_and_replayed(ctx, port, fmt):
    """Each picture equals its own expectation; a second decode and two replays of a captured graph give identical bytes; the timed
    decode names the launches it always named."""
    items, want = _mixed(port)
    with ctx.batch([x.desc for x in items], _fmt(fmt)) as b:
        b.upload(); b.decode(); b.sync()
        first, st = b.download()
        assert list(st) == [0] * len(items)
        for k, (g, w) in enumerate(zip(first, want)):
            _same(g, w, fmt, ("mixed", k))
        timed, _ = b.decode_timed()
        b.sync()
        again, _ = b.download()
        assert all(np.array_equal(a, c) for a, c in zip(again, first))
        assert "idct_std" in timed and "colour_std" in timed and "idct_colour" in timed, timed
        b.capture()
        for _ in range(2):
            b.decode(); b.sync()
            outs, st2 = b.download()
            assert list(st2) == [0] * len(items)
            assert all(np.array_equal(a, c) for a, c in zip(outs, first))


def test_grey_mixed_batch_and_its_timed_name(ctx):
    import pjd_amd
    items = [(BIG, 1), ("ls_259x19_422_q50", 2), ("ls_136x72_420_q100_rst4", 4), (BIG, 8), ("ls_61x45_grey_q50", 2), ("ls_33x31_420_q90_prog", 4)]
    sc = [scanned(n, s) for n, s in items]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_GRAY8) as b:
        b.upload(); b.decode(); b.sync()
        first, st = b.download()
        assert list(st) == [0] * len(items)
        for (n, s), g in zip(items, first):
            same(g, recording(n, s, "l8"), "gray", (n, s))
        timed, _ = b.decode_timed()
        b.sync()
        again, _ = b.download()
        assert all(np.array_equal(a, c) for a, c in zip(again, first))
        assert "idct_gray_std" in timed and "colour_std" not in timed, timed
        b.capture()
        b.decode(); b.sync()
        outs, _ = b.download()
        assert all(np.array_equal(a, c) for a, c in zip(outs, first))


def test_device_bytes_shrink_with_the_scale(ctx):
    """The component planes of a flagged batch are sized at the reduced geometry: a 1/4 batch occupies less than the same batch at 1/1
    by at least the difference of the pictures and most of the planes'."""
    import pjd_amd
    names = [BIG, "ls_136x72_420_q100_rst4", "ls_259x19_422_q50", "ls_61x45_grey_q50"] * 8
    sizes = {}
    for s in (1, 4):
        sc = [scanned(n, s) for n in names]
        with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            b.upload(); b.decode(); b.sync()
            assert list(b.statuses()) == [0] * len(names)
            sizes[s] = b.info()["device_bytes"]
    full_planes = 16 * (136 * 72 * 3 // 2)                 # the 4:2:0 pictures' planes alone, at full size
    assert sizes[4] < sizes[1] - full_planes // 2, sizes


def _truncated():
    """ls_33x31_420_q90 (3 x 2 MCUs) with its entropy-coded data cut to a third: the error lies in the first MCU row."""
    data = jpeg("ls_33x31_420_q90")
    body = data.rfind(b"\xff\xda") + 14
    n = len(data) - 2 - body
    return data[:body + n // 3] + b"\xff\xd9"


@pytest.mark.parametrize("fmt", ["rgb8", "gray"])
def test_truncated_stream(ctx, fmt):
    """The status is the one at full size; the partial picture is the model over the coefficients the decoder kept -- zero behind the
    error, so 128 there at every scale."""
    import pjd_amd
    data = _truncated()
    for extra in (0, pjd_amd.F_FORCE_SEQUENTIAL):
        sc = []
        for s in (1, 2, 4, 8):
            x = pjd_amd.Scanned(data)
            x.desc.flags = int(x.desc.flags) | pjd_amd.F_LIBJPEG | FLAG[s] | extra
            sc.append(x)
        with ctx.batch([x.desc for x in sc], fmt_of(fmt)) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            coefs = [b.coefficients(k) for k in range(4)]
        assert st[0] != 0 and list(st) == [st[0]] * 4
        assert all(np.array_equal(coefs[0], c) for c in coefs[1:])
        for k, s in enumerate((1, 2, 4, 8)):
            want = model(coefs[0], sc[k].desc, s, fmt == "gray")
            same(outs[k], want, fmt, ("truncated", s, extra))
            # the second MCU row (picture rows 16 / s on) was never decoded; at full size fancy upsampling leans one chroma row up into it
            tail = np.asarray(outs[k])[-(-18 // s):]
            assert tail.size and (tail == 128).all() and not (np.asarray(outs[k])[:8 // s] == 128).all(), (s, extra)


def _torch_case(case, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(HERE, "libjpeg_scaled_torch_cases.py"), case], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and f"CASE OK {case}" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])


@pytest.mark.parametrize("fmt", ["rgb8", "planar", "gray"])
def test_bound_output_into_a_poisoned_tensor(fmt):
    _torch_case("bound_poisoned_" + fmt)


def test_draft_through_resize_and_normalise():
    _torch_case("draft_resize")
