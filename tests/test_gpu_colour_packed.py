"""The colour stage's packed fast path and the division-free unit tables of the lane back end on the GPU (run with -m gpu on an
MI355X): pjd_colour_store and pjd_idct_range, pim-jpeg-decoder_amd/csrc/pjd_k_backend.hip.

The pictures come from tests/colour_packed_cases.py: hand-built streams whose chroma samples lie on both sides of each end of the
range [-16384, 16383] that decides between the packed rows and the 32-bit rows, and at the int16 extremes, beside luma at -32768 and
32767; in-range and out-of-range chroma blocks alternate along an MCU row, so that one wave runs both kinds of row.
(tests/test_colour_packed_cpu.py checks with the oracle port's IDCT that the samples are there.  The blocks hold AC coefficients
too: a DC-only block cannot reach +-16384, see colour_packed_cases.py.)  Status, coefficients and pixels must equal the streams'
intent through the oracle port's back end, and the port's own decode, in all three output formats:

* every sampling mode at 13 x 9 and 35 x 19: the right edge inside a group of four pixels, the bottom edge inside an MCU, the last
  chroma row shared by one picture row;
* 80 x 112 in 4:2:0 (5 x 7 MCUs: back-end ranges straddle MCU rows, a range has a second group of 64 units) and 72 x 40 in 4:4:4
  (45 MCUs of three units: more MCUs than a wave has lanes), in both plan modes;
* restart intervals of 1, 2 and 5 MCUs under PJD_F_STANDARD_RESTART on the 80 x 112 picture: the tabulated segment heads;
* grey pictures and a two-component frame (the missing chroma reads as 0)."""
import functools

import numpy as np
import pytest

import colour_packed_cases as M
from test_gpu_symbol_streams import _decode_and_check, _scan, intent_rgb

pytestmark = pytest.mark.gpu

FORMATS = ["rgb8", "bmp", "planar"]


@functools.lru_cache(maxsize=None)
def _picture(w, h, sub, ri=0, std=False, first=0):
    data, fr, it, _ = M.picture(w, h, sub, ri, std, first)
    return (f"{sub}:{w}x{h}:ri{ri}:first{first}", data, fr, it)


@pytest.fixture(scope="module")
def ctx():
    import pjd_amd
    c = pjd_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(port):
    """label -> the intent's picture through the port's back end, computed once per picture"""
    cache = {}

    def get(item):
        label, data, fr, it = item
        if label not in cache:
            rgb = intent_rgb(port, data, fr, it)
            if not (fr.standard_restart and fr.ri and (fr.hs, fr.vs) != (1, 1)):      # (there the port follows the reference's restart rule)
                assert np.array_equal(rgb, port.decode(data)["rgb"]), label
            rgb.setflags(write=False)
            cache[label] = rgb
        return cache[label]
    return get


def _check_format(ctx, port, want, items, fmt):
    import pjd_amd
    if fmt == "rgb8":
        _decode_and_check(ctx, port, items, _scan(items))                 # status, coefficients, pixels, routing
        return
    out_fmt = pjd_amd.OUT_BMP if fmt == "bmp" else pjd_amd.OUT_RGB8_PLANAR
    scanned = _scan(items)
    with ctx.batch([s.desc for s in scanned], out_fmt) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0, info
    for item, o, status in zip(items, outs, st):
        label, data, fr, it = item
        assert status == it.status, (label, fmt)
        rgb = want(item)
        if fmt == "bmp":
            assert np.array_equal(np.asarray(o).reshape(-1), np.frombuffer(pjd_amd.rgb_to_bmp(rgb), np.uint8)), (label, fmt)
        else:
            assert o.shape == (3, fr.height, fr.width) and np.array_equal(o, rgb.transpose(2, 0, 1)), (label, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sub", ["444", "422", "440", "420"])
def test_small_pictures_every_sampling_and_format(ctx, port, want, sub, fmt):
    """13 x 9 and 35 x 19, started at several places of the block cycle so that the few MCUs of a small picture see every block."""
    items = [_picture(w, h, sub, first=first) for w, h in [(13, 9), (35, 19)] for first in (0, 2, 4, 6, 8)]
    _check_format(ctx, port, want, items, fmt)


@pytest.mark.parametrize("mode", ["latency", "throughput"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ranges_across_mcu_rows_and_more_mcus_than_lanes(port, want, fmt, mode):
    import pjd_amd
    items = [_picture(80, 112, "420"), _picture(72, 40, "444"), _picture(80, 112, "420", first=5), _picture(72, 40, "444", first=3)]
    c = pjd_amd.Context(0)
    try:
        c.set_plan_mode(pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
        _check_format(c, port, want, items, fmt)
    finally:
        c.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_restart_segments_start_inside_ranges(ctx, port, want, fmt):
    """PJD_F_STANDARD_RESTART with 1, 2 and 5 MCUs per segment: every range of 16 MCUs holds several segment heads, at every offset."""
    items = [_picture(80, 112, "420", ri=ri, std=True, first=ri) for ri in (1, 2, 5)] + [_picture(72, 40, "444", ri=5, std=True)]
    _check_format(ctx, port, want, items, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_grey_and_two_component_pictures(ctx, port, want, fmt):
    items = [_picture(w, h, sub, ri=ri, std=ri != 0, first=first)
             for sub in ("grey", "2c") for w, h, ri, first in [(13, 9, 0, 1), (35, 19, 0, 0), (80, 112, 5, 2)]]
    _check_format(ctx, port, want, items, fmt)
