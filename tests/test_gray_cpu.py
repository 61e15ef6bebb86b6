"""PJD_OUT_GRAY8 on the host (no GPU): the format's constants and sizes, what the planner accepts and refuses, and the two builders of
expected planes that tests/test_gpu_gray.py holds the device against (tests/gray_expected.py) -- the oracle with neutral chroma, whose
three channels must be equal, and Pillow's draft("L") recordings, which must be the luma plane of the libjpeg model."""
import io
import json
import os

import numpy as np
import pytest

import gray_expected as G
from gray_expected import golden_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest.json")))
VALID = sorted(k for k, v in MANIFEST.items() if v["rc"] == 0)
E_ARG = -3


def _scanned(name, flags=0):
    import pjd_amd
    s = pjd_amd.Scanned(golden_bytes(name))
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def test_constants_and_exports():
    import pjd_amd
    from pjd_amd import tensors
    # 3 is skipped: tests/test_planar_cpu.py pins it as the unknown value callers were promised PJD_E_ARG for
    assert (pjd_amd.OUT_RGB8, pjd_amd.OUT_BMP, pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_GRAY8) == (0, 1, 2, 4)
    assert pjd_amd.ABI_VERSION == 6 == pjd_amd.dev_lib().pjd_version()
    assert hasattr(pjd_amd.dev_lib(), "pjd_output_channels") and callable(pjd_amd.output_channels)
    import inspect
    for fn in (tensors.decode_to_tensors, tensors.decode_to_batch_tensor):
        assert inspect.signature(fn).parameters["gray"].default is False
    header = open(os.path.join(os.path.dirname(HERE), "include", "pjd.h")).read()
    assert "#define PJD_OUT_GRAY8  4" in header and "int  pjd_output_channels(int out_format);" in header and "#define PJD_VERSION 6" in header


def test_output_channels():
    import pjd_amd
    assert [pjd_amd.output_channels(f) for f in (pjd_amd.OUT_RGB8, pjd_amd.OUT_BMP, pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_GRAY8)] == [3, 3, 3, 1]
    assert [pjd_amd.output_channels(f) for f in (3, 5, 7, -1, 255, 2 ** 31 - 1)] == [0] * 6


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (17, 9), (61, 45), (65535, 65535)])
def test_output_size_is_one_plane(w, h):
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert L.pjd_output_size(w, h, pjd_amd.OUT_GRAY8) == w * h
    assert L.pjd_output_size(w, h, pjd_amd.OUT_RGB8_PLANAR) == 3 * w * h


def test_image_output_size_and_plan_info_at_every_scale():
    import pjd_amd
    names = ["env_61x45_420_q100_opt", "gray_33x70", "h1v2_48x64", "env_17x9_444_q85"]
    for flags, s in [(0, 1), (16, 2), (32, 4), (48, 8)]:
        sc = [_scanned(n, flags) for n in names]
        want = [-(-int(x.desc.width) // s) * -(-int(x.desc.height) // s) for x in sc]
        assert [pjd_amd.image_output_size(x.desc, pjd_amd.OUT_GRAY8) for x in sc] == want
        g = pjd_amd.plan_info([x.desc for x in sc], pjd_amd.OUT_GRAY8)
        p = pjd_amd.plan_info([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR)
        assert g["out_bytes"] == sum(want) and p["out_bytes"] == 3 * sum(want)
        # everything but the byte counts is the planar batch's: lanes, units, the entropy decoder's plan
        for k in g:
            if k not in ("out_bytes", "device_bytes"):
                assert g[k] == p[k], (k, s)


def test_plan_check_accepts_and_refuses_as_specified():
    import pjd_amd
    ok = [_scanned(n) for n in ("env_61x45_420_q100_opt", "gray_33x70", "h1v2_48x64")]
    assert pjd_amd.plan_check([x.desc for x in ok], pjd_amd.OUT_GRAY8) == (0, "")
    for fmt in (3, 5, -1):
        rc, why = pjd_amd.plan_check([x.desc for x in ok], fmt)
        assert rc == E_ARG and "unknown output format" in why
    # a shard is accepted, as in an RGB8 batch
    sh = _scanned("rst4_128x96_444")
    assert sh.desc.n_segments >= 2
    sh.desc.shard_first_seg, sh.desc.shard_n_segs = 0, 1
    assert pjd_amd.plan_check([sh.desc], pjd_amd.OUT_GRAY8)[0] == 0
    # PJD_F_LIBJPEG: accepted; with an output scale, 4:4:0 sampling or a shard refused exactly as in the other formats
    data = G.lj_bytes("lj_136x72_420_q90")
    lj = pjd_amd.Scanned(data)
    lj.desc.flags = int(lj.desc.flags) | pjd_amd.F_LIBJPEG
    assert pjd_amd.plan_check([ok[0].desc, lj.desc], pjd_amd.OUT_GRAY8) == (0, "")
    for flag in (pjd_amd.F_SCALE_1_2, pjd_amd.F_SCALE_1_4, pjd_amd.F_SCALE_1_8):
        bad = pjd_amd.Scanned(data)
        bad.desc.flags = int(bad.desc.flags) | pjd_amd.F_LIBJPEG | flag
        for fmt in (pjd_amd.OUT_GRAY8, pjd_amd.OUT_RGB8_PLANAR):
            rc, why = pjd_amd.plan_check([ok[0].desc, bad.desc], fmt)
            assert rc == E_ARG and "image 1" in why and "PJD_F_SCALE" in why, why
    h1v2 = _scanned("h1v2_48x64", pjd_amd.F_LIBJPEG)
    rc, why = pjd_amd.plan_check([h1v2.desc], pjd_amd.OUT_GRAY8)
    assert rc == E_ARG and "4:4:0" in why


def test_grey_libjpeg_batch_plans_no_plane_buffer():
    """pjd_plan_info leaves device_bytes alone; the GPU suite compares it.  Here: the plan of a flagged picture is the planar one's."""
    import pjd_amd
    data = G.lj_bytes("lj_136x72_420_q90")
    s = pjd_amd.Scanned(data)
    s.desc.flags = int(s.desc.flags) | pjd_amd.F_LIBJPEG
    g, p = pjd_amd.plan_info([s.desc], pjd_amd.OUT_GRAY8), pjd_amd.plan_info([s.desc], pjd_amd.OUT_RGB8_PLANAR)
    assert g["out_bytes"] == 136 * 72 and p["out_bytes"] == 3 * 136 * 72 and g["n_data_units"] == p["n_data_units"] == 270


def test_pipe_refuses_nothing_new():
    """An unknown format is refused before anything is scanned; the grey format, like the three old ones, is not (no input: no device)."""
    import pjd_amd
    for fmt in (pjd_amd.OUT_RGB8, pjd_amd.OUT_BMP, pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_GRAY8):
        st = pjd_amd.pipe_run(jpegs=[], out_format=fmt)
        assert st["n_inputs"] == 0 and st["n_batch_failures"] == 0
    with pytest.raises(pjd_amd.PjdError) as e:
        pjd_amd.pipe_run(jpegs=[], out_format=3)
    assert "(-3)" in str(e.value)


def test_split_decode_refuses_the_format_without_a_device():
    import pjd_amd
    s = _scanned("rst4_128x96_444")
    with pytest.raises(pjd_amd.PjdError) as e:
        pjd_amd.split_decode(s.desc, [0, 0], pjd_amd.OUT_GRAY8)
    assert "(-3)" in str(e.value)


# ---- the expected-value builders -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VALID)
def test_neutral_chroma_picture_has_three_equal_channels(port, name):
    """P0 of the definition: R == G == B, and the status is the decode's own.  Where the file has one component P0 is the oracle's
    picture; where it has three, the plane differs from every channel of the colour picture somewhere (else the fixture shows nothing)."""
    data = golden_bytes(name)
    st, rgb = G.neutral_chroma_picture(port, data)
    full = port.decode(data)
    assert st == full["huff_rc"]
    assert np.array_equal(rgb[:, :, 0], rgb[:, :, 1]) and np.array_equal(rgb[:, :, 0], rgb[:, :, 2]), name
    if full["info"]["ncomp"] == 1:
        assert np.array_equal(rgb, full["rgb"]), name


def test_neutral_chroma_plane_is_not_a_channel_of_the_colour_picture(port):
    data = golden_bytes("env_61x45_420_q100_opt")
    plane, full = G.ref_plane(port, data)[1], port.decode(data)["rgb"]
    assert all(not np.array_equal(plane, full[:, :, c]) for c in range(3))


def test_undecoded_part_is_128(port):
    name = next(n for n in VALID if MANIFEST[n]["huff_ok"] == 0)
    st, plane = G.ref_plane(port, golden_bytes(name))
    assert st != 0 and (plane[-1] == 128).all(), name


def test_fixture_set_matches_the_libjpeg_fixtures():
    cases = G.lj_cases()
    assert sorted(G.gray_manifest()["cases"]) == sorted(cases) and len(cases) == 17
    for n, c in cases.items():
        assert G.l8(n).shape == (c["height"], c["width"])
    assert max(c["max_diff_to_convert_L"] for c in G.gray_manifest()["cases"].values()) >= 20      # not a weighted sum of R, G, B


@pytest.mark.parametrize("name", G.lj_baseline_cases())
def test_recorded_plane_is_the_models_luma_plane(port, name):
    data, rgb, c = G.lj_bytes(name), G.lj_rgb(name), G.lj_cases()[name]
    want = G.model_y_plane(port, data)
    assert np.array_equal(G.l8(name), want), name
    if c["sampling"] == "grey":
        assert np.array_equal(G.l8(name), rgb[:, :, 0])


@pytest.mark.parametrize("name", sorted(G.lj_cases()))
def test_recorded_plane_is_this_pillows_draft_L(name):
    Image = pytest.importorskip("PIL.Image")
    data = G.lj_bytes(name)
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L" and np.array_equal(np.asarray(im), G.l8(name))


def test_box_model_on_one_plane():
    p = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7) * 7
    assert np.array_equal(G.box1(p, 1), p)
    b = G.box1(p, 4)
    assert b.shape == (2, 2) and b[0, 0] == (int(p[:4, :4].sum()) + 8) // 16 and b[1, 1] == (int(p[4:, 4:].sum()) + 1) // 3


# ---- pjd_amd.tensors: the checks that need no device -------------------------------------------------------------------------------
def test_tensor_helpers_check_gray_before_anything_is_created():
    from pjd_amd import tensors
    s = _scanned("gray_33x70")
    with pytest.raises(ValueError, match="planar=True"):
        tensors.decode_to_tensors(None, [s.desc], planar=False, gray=True)
    t = _scanned("env_17x9_444_q85")
    with pytest.raises(ValueError, match="uniform_output_shape"):
        tensors.decode_to_batch_tensor(None, [s.desc, t.desc], gray=True)


def test_gray_keyword_of_the_resizing_helpers_takes_scalars():
    """mean and std: one number or length 1 (or 3); fill and pad_value: one number; all checked before anything is created."""
    import inspect
    from pjd_amd import tensors
    for fn in (tensors.decode_resized_batch_tensor, tensors.decode_normalized_batch_tensor):
        assert inspect.signature(fn).parameters["gray"].default is False
    assert tensors._gray3(0.5, "mean") == [0.5] * 3 and tensors._gray3([0.25], "std") == [0.25] * 3 and tensors._gray3((1, 2, 3), "x") == [1, 2, 3]
    with pytest.raises(ValueError, match="mean"):
        tensors._gray3([1, 2], "mean")
    assert tensors._fill(114, gray=True) == (114, 114, 114) and tensors._fill([7], gray=True) == (7, 7, 7)
    with pytest.raises(ValueError):
        tensors._fill(300, gray=True)
    with pytest.raises((ValueError, TypeError)):
        tensors._fill(114)                                         # three bytes without gray=True, as before
    s = _scanned("gray_33x70")
    # every refusal below comes before a context or torch is touched: ctx is None
    with pytest.raises(ValueError, match="channels_last"):
        tensors.decode_normalized_batch_tensor(None, [s.desc], (8, 8), 0.5, 0.25, channels_last=True, gray=True)
    with pytest.raises(ValueError, match="std"):
        tensors.decode_normalized_batch_tensor(None, [s.desc], (8, 8), 0.5, [0.25, 0.25], gray=True)
    with pytest.raises(ValueError, match="non-zero"):
        tensors.decode_normalized_batch_tensor(None, [s.desc], (8, 8), 0.5, 0.0, gray=True)
    with pytest.raises(ValueError, match="three means"):
        tensors.decode_normalized_batch_tensor(None, [s.desc], (8, 8), 0.5, 0.25)          # scalars only with gray=True
    with pytest.raises(ValueError, match="pad_value needs letterbox"):
        tensors.decode_normalized_batch_tensor(None, [s.desc], (8, 8), 0.5, 0.25, pad_value=0, gray=True)
    with pytest.raises(ValueError, match="prescale=False"):
        tensors.decode_resized_batch_tensor(None, [s.desc], (8, 8), libjpeg=True, gray=True)
    with pytest.raises(ValueError, match="interpolation"):
        tensors.decode_resized_batch_tensor(None, [s.desc], (8, 8), interpolation="nearest", gray=True)
    with pytest.raises(ValueError, match="fill"):
        tensors.decode_resized_batch_tensor(None, [s.desc], (8, 8), letterbox="center", fill=(1, 2), gray=True)


def test_resolver_plans_one_plane():
    """pjd_batch_set_resize needs a device; the sizes it will report are the format's: tw * th bytes a picture (the GPU suite checks
    pjd_batch_output_size itself).  Here: the host-only size entry points at resized dimensions."""
    import pjd_amd
    L = pjd_amd.dev_lib()
    for tw, th in [(1, 1), (23, 17), (41, 30), (224, 224)]:
        assert L.pjd_output_size(tw, th, pjd_amd.OUT_GRAY8) == tw * th
