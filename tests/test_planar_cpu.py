"""Planar output (PJD_OUT_RGB8_PLANAR, include/pjd.h) and pjd_batch_bind_output on the host side: constants, sizes, the planner's
figures, the exported ABI and the pure helper of pjd_amd.tensors.  No GPU needed; the pictures are checked in test_gpu_planar.py."""
import sys

import pytest

from conftest import golden_bytes
from test_scaled_cpu import DIMS, SCALES


def _pjd():
    import pjd_amd
    return pjd_amd


def test_constants_version_and_exports():
    pjd = _pjd()
    assert (pjd.OUT_RGB8, pjd.OUT_BMP, pjd.OUT_RGB8_PLANAR) == (0, 1, 2)
    assert pjd.ABI_VERSION == 6 and pjd.dev_lib().pjd_version() == 6           # no struct changed
    assert hasattr(pjd.dev_lib(), "pjd_batch_bind_output")
    assert callable(pjd.Batch.bind_output)


@pytest.mark.parametrize("w,h", DIMS)
def test_planar_sizes(w, h):
    pjd = _pjd()
    L = pjd.dev_lib()
    for flags, s in SCALES:
        want = 3 * -(-w // s) * -(-h // s)
        d = pjd.ImageDesc()
        d.width, d.height, d.flags = w, h, flags
        assert pjd.image_output_size(d, pjd.OUT_RGB8_PLANAR) == want, (w, h, s)
        assert pjd.image_output_size(d, pjd.OUT_RGB8_PLANAR) == pjd.image_output_size(d, pjd.OUT_RGB8)
        sw, sh = pjd.scaled_dims(w, h, flags)
        assert int(L.pjd_output_size(sw, sh, pjd.OUT_RGB8_PLANAR)) == want, (w, h, s)


def _mixed_descs(pjd):
    names = ["ilsvrc_val_00000001", "env_61x45_422_q30", "big_640x480_420_q85", "rst4_128x96_444", "gray_61x45"]
    scanned = [pjd.Scanned(golden_bytes(n)) for n in names]
    want = 0
    for k, s in enumerate(scanned):
        assert s.valid
        flags, sc = SCALES[k % 4]
        s.desc.flags = int(s.desc.flags) | flags
        want += 3 * -(-int(s.desc.width) // sc) * -(-int(s.desc.height) // sc)
    return scanned, want


def test_plan_info_of_a_mixed_scale_planar_list():
    """The two formats differ in layout only: every figure of the plan equals the PJD_OUT_RGB8 plan of the same list."""
    pjd = _pjd()
    scanned, want = _mixed_descs(pjd)
    descs = [s.desc for s in scanned]
    planar = pjd.plan_info(descs, pjd.OUT_RGB8_PLANAR)
    assert planar["out_bytes"] == want
    assert planar == pjd.plan_info(descs, pjd.OUT_RGB8)


@pytest.mark.parametrize("fmt", [3, -1])
def test_unknown_format_is_still_an_argument_error(fmt):
    pjd = _pjd()
    scanned, _ = _mixed_descs(pjd)
    with pytest.raises(pjd.PjdError, match=r"\(-3\)"):
        pjd.plan_info([s.desc for s in scanned], fmt)


def test_uniform_output_shape_is_pure():
    pjd = _pjd()
    had_torch = "torch" in sys.modules
    from pjd_amd import tensors
    assert had_torch or "torch" not in sys.modules                              # importing the module does not import torch

    def desc(w, h, flags=0):
        d = pjd.ImageDesc()
        d.width, d.height, d.flags = w, h, flags
        return d

    assert tensors.uniform_output_shape([desc(500, 375)] * 4) == (4, 3, 375, 500)
    # scale flags count: 500x375 at 1/2 is 250x188, and so is 499x376 at 1/2; other flags do not
    assert tensors.uniform_output_shape([desc(500, 375, pjd.F_SCALE_1_2), desc(499, 376, pjd.F_SCALE_1_2 | pjd.F_FORCE_SEQUENTIAL)]) == (2, 3, 188, 250)
    assert tensors.uniform_output_shape([desc(64, 48, pjd.F_SCALE_1_8), desc(8, 6)]) == (2, 3, 6, 8)
    for w, h in DIMS:
        for flags, s in SCALES:
            assert tensors.uniform_output_shape([desc(w, h, flags)]) == (1, 3, -(-h // s), -(-w // s))
    with pytest.raises(ValueError):
        tensors.uniform_output_shape([desc(500, 375), desc(500, 375, pjd.F_SCALE_1_2)])
    with pytest.raises(ValueError):
        tensors.uniform_output_shape([desc(500, 375), desc(375, 500)])
    with pytest.raises(ValueError):
        tensors.uniform_output_shape([])
    assert had_torch or "torch" not in sys.modules
