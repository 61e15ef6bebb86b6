"""Reduced-size output (PJD_F_SCALE_*, include/pjd.h) on the host side: output dimensions and sizes, the planner's byte counts
and the exported ABI.  No GPU needed; the pictures themselves are checked in test_gpu_scaled.py."""
import ctypes as C

import pytest

from conftest import golden_bytes

DIMS = [(1, 1), (8, 8), (17, 9), (61, 45), (72, 40), (1200, 64), (40, 900)]
SCALES = [(0, 1), (16, 2), (32, 4), (48, 8)]          # (descriptor flags, s)


def _pjd():
    import pjd_amd
    return pjd_amd


def _want_dims(w, h, s):
    return -(-w // s), -(-h // s)                     # libjpeg's jdiv_round_up


def _want_size(w, h, s, fmt):
    sw, sh = _want_dims(w, h, s)
    return 26 + sh * (3 * sw + sw % 4) if fmt == 1 else 3 * sw * sh


def test_flag_values_and_version():
    pjd = _pjd()
    assert (pjd.F_SCALE_1_2, pjd.F_SCALE_1_4, pjd.F_SCALE_1_8, pjd.F_SCALE_MASK) == (16, 32, 48, 48)
    for flags, s in SCALES:
        assert 1 << ((flags >> 4) & 3) == s
    assert pjd.ABI_VERSION == 6 and pjd.dev_lib().pjd_version() == 6


def test_new_symbols_are_exported():
    pjd = _pjd()
    for name in ("pjd_scaled_dims", "pjd_image_output_size"):
        assert hasattr(pjd.dev_lib(), name)
    pipe = C.CDLL(pjd.LIBPIPE)
    assert hasattr(pipe, "pjd_pipe_run_memory")
    # pjd_pipe_opts gained image_flags at its end
    assert pjd.PipeOpts.image_flags.offset == pjd.PipeOpts.scan_options.offset + 4


@pytest.mark.parametrize("w,h", DIMS)
def test_scaled_dims_and_sizes(w, h):
    pjd = _pjd()
    L = pjd.dev_lib()
    for flags, s in SCALES:
        extra = pjd.F_STANDARD_RESTART | pjd.F_FORCE_SEQUENTIAL       # other flags do not change the output size
        for f in (flags, flags | extra):
            assert pjd.scaled_dims(w, h, f) == _want_dims(w, h, s), (w, h, f)
            d = pjd.ImageDesc()
            d.width, d.height, d.flags = w, h, f
            for fmt in (pjd.OUT_RGB8, pjd.OUT_BMP):
                assert pjd.image_output_size(d, fmt) == _want_size(w, h, s, fmt), (w, h, f, fmt)
                if s == 1:
                    assert pjd.image_output_size(d, fmt) == int(L.pjd_output_size(w, h, fmt))
    assert int(L.pjd_image_output_size(None, pjd.OUT_RGB8)) == 0


@pytest.mark.parametrize("fmt", [0, 1])
def test_plan_info_of_a_mixed_scale_list(fmt):
    pjd = _pjd()
    names = ["ilsvrc_val_00000001", "env_61x45_422_q30", "big_640x480_420_q85", "rst4_128x96_444", "gray_61x45"]
    scanned = [pjd.Scanned(golden_bytes(n)) for n in names]
    descs = []
    for k, s in enumerate(scanned):
        assert s.valid
        descs.append(s.desc)
    full = pjd.plan_info(descs, fmt)
    want = 0
    for k, d in enumerate(descs):
        flags, s = SCALES[k % 4]
        d.flags = int(d.flags) | flags
        want += _want_size(int(d.width), int(d.height), s, fmt)
    mixed = pjd.plan_info(descs, fmt)
    assert mixed["out_bytes"] == want
    assert mixed["pixels"] == full["pixels"] == sum(int(d.width) * int(d.height) for d in descs)
    assert mixed["n_data_units"] == full["n_data_units"] and mixed["n_sequential"] == full["n_sequential"]
    assert mixed["out_bytes"] < full["out_bytes"]
