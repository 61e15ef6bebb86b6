"""PJD_F_LIBJPEG_SCALE_* on the host (no GPU): the numpy model of the arithmetic in include/pjd.h (tests/libjpeg_scaled_model.py) equals
Pillow's recorded draft decode of the fixtures under tests/golden/libjpeg_scaled/ byte for byte at 1/1, 1/2, 1/4 and 1/8, as RGB and as
"L"; the host entry point pjd_libjpeg_idct_scaled -- the inline the kernels run -- equals the model; sizes, refusals, the tensors
keyword and the CLI.  Zero tolerance everywhere: the arithmetic is integer.

The model is fed the oracle port's coefficients, and the port reads neither progressive frames nor T.81 restart intervals: the restart
and the progressive fixture are held to their recordings on the GPU (tests/test_gpu_libjpeg_scaled.py), where the decoder's own
coefficients are at hand."""
import ctypes as C
import functools
import io
import json
import os
import subprocess

import numpy as np
import pytest

import libjpeg_scaled_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "libjpeg_scaled")
SCALES = (1, 2, 4, 8)
FLAG = {1: 0, 2: 128, 4: 256, 8: 384}
E_ARG = -3                                  # PJD_E_ARG of include/pjd.h
# the scales Pillow cannot be made to take (an axis shorter than s): fixed by the sizes of the fixture set, held to the model alone
MODEL_ONLY = {("ls_3x5_420_q90", 4), ("ls_3x5_420_q90", 8), ("ls_3x5_422_q100", 4), ("ls_3x5_422_q100", 8), ("ls_4x9_420_q50", 8),
              ("ls_4x9_422_q90", 8), ("ls_5x4_420_q90", 8), ("ls_5x4_422_q90", 8)}


@functools.lru_cache(maxsize=1)
def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)


def jpeg(name):
    with open(os.path.join(GOLD, name + ".jpg"), "rb") as f:
        return f.read()


def out_size(c, s):
    return -(-c["width"] // s), -(-c["height"] // s)


@functools.lru_cache(maxsize=None)
def recording(name, s, mode):
    """Pillow's recorded decode at 1/s: mode "rgb" -> [oh, ow, 3], "l8" -> [oh, ow]; None for a model-only scale."""
    c = manifest()["cases"][name]
    if s in c["model_only"]:
        return None
    ow, oh = out_size(c, s)
    with open(os.path.join(GOLD, f"{name}.s{s}.{mode}"), "rb") as f:
        a = np.frombuffer(f.read(), np.uint8).reshape((oh, ow, 3) if mode == "rgb" else (oh, ow))
    return a


def port_cases():
    return sorted(n for n, c in manifest()["cases"].items() if not c["progressive"] and not c["restart_marker_blocks"])


@functools.lru_cache(maxsize=None)
def _port_decode(name):
    import oracle_lib
    port = oracle_lib.Port()
    port.standard_zigzag(True)
    try:
        d = port.decode(jpeg(name))
    finally:
        port.standard_zigzag(False)
    assert d["huff_rc"] == 0
    info = d["info"]
    qts = [info["qt"][info["comp_qt"][k]] for k in range(info["ncomp"])]
    return d["coef"], qts, info


def model_from_port(name, s, gray):
    coef, qts, info = _port_decode(name)
    return SM.decode(coef, qts, info["width"], info["height"], info["ncomp"], info["hsamp"], info["vsamp"], s, gray)


def test_fixture_set_is_the_one_the_mode_is_specified_on():
    cases = manifest()["cases"]
    have = {(c["width"], c["height"], c["sampling"]) for c in cases.values()}
    for want in [(8, 8, "4:4:4"), (16, 16, "4:2:0"), (17, 17, "4:2:0"), (33, 31, "4:2:0"), (40, 24, "4:2:2"), (259, 19, "4:2:2"), (61, 45, "grey"),
                 (3, 5, "4:2:0"), (3, 5, "4:2:2"), (4, 9, "4:2:0"), (4, 9, "4:2:2"), (5, 4, "4:2:0"), (5, 4, "4:2:2"), (136, 72, "4:2:0")]:
        assert want in have, want
    assert {c["quality"] for c in cases.values()} >= {50, 90, 100}
    assert any(c["progressive"] for c in cases.values())
    assert any(c["restart_marker_blocks"] == 4 and (c["width"], c["height"]) == (136, 72) for c in cases.values())
    assert manifest()["pillow"]
    # "model only" is exactly the scales an axis is too short for, and the list may not grow
    assert {(n, s) for n, c in cases.items() for s in c["model_only"]} == MODEL_ONLY
    assert all((min(c["width"], c["height"]) < s) == (s in c["model_only"]) for c in cases.values() for s in SCALES)
    # 259 x 19: a chroma row of odd length > 2 at every fancy scale
    for s in (2, 4):
        dw = -(-259 * (8 // s) // 16)
        assert dw % 2 == 1 and dw > 2


@pytest.mark.parametrize("mode", ["rgb", "l8"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", port_cases())
def test_model_equals_recorded_pillow_draft(name, s, mode):
    want = recording(name, s, mode)
    got = model_from_port(name, s, mode == "l8")
    c = manifest()["cases"][name]
    ow, oh = out_size(c, s)
    assert got.shape == ((oh, ow, 3) if mode == "rgb" else (oh, ow))
    if want is None:
        assert (name, s) in MODEL_ONLY
        return
    assert np.array_equal(got, want), f"{name} 1/{s} {mode}: {int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("name", sorted(manifest()["cases"]))
def test_recorded_draft_is_this_pillows(name):
    """Where Pillow is installed its draft decode of the fixture is the recorded one, at every scale it takes."""
    Image = pytest.importorskip("PIL.Image")
    c = manifest()["cases"][name]
    for s in SCALES:
        if s in c["model_only"]:
            continue
        for mode, pm in (("rgb", "RGB"), ("l8", "L")):
            im = Image.open(io.BytesIO(jpeg(name)))
            im.draft(pm, (max(1, c["width"] // s), max(1, c["height"] // s)))
            assert im.size == out_size(c, s)
            assert np.array_equal(np.asarray(im.convert(pm)), recording(name, s, mode)), (name, s, mode)


def test_symbol_and_flags_exist():
    import pjd_amd
    assert (pjd_amd.F_LIBJPEG_SCALE_1_2, pjd_amd.F_LIBJPEG_SCALE_1_4, pjd_amd.F_LIBJPEG_SCALE_1_8, pjd_amd.F_LIBJPEG_SCALE_MASK) == (128, 256, 384, 384)
    assert hasattr(pjd_amd.dev_lib(), "pjd_libjpeg_idct_scaled")
    others = (pjd_amd.F_LIBJPEG | pjd_amd.F_SCALE_MASK | pjd_amd.F_PROGRESSIVE | pjd_amd.F_STANDARD_ZIGZAG | pjd_amd.F_STANDARD_RESTART |
              pjd_amd.F_FORCE_SEQUENTIAL)
    assert pjd_amd.F_LIBJPEG_SCALE_MASK & others == 0
    assert pjd_amd.dev_lib().pjd_version() == 6


def _random_units(rng, count):
    """Seeded units: sparse and dense inside libjpeg's envelope, then int16 extremes and 16-bit quantisers (beyond it: pinned to the text)."""
    out = []
    for k in range(count):
        kind = k % 4
        if kind == 3:
            q = rng.integers(1, 65536, 64)
            c = rng.integers(-32768, 32768, 64)
            c[rng.choice(64, 6, replace=False)] = rng.choice([-32768, 32767, -1, 0, 1], 6)
            q[rng.choice(64, 4, replace=False)] = rng.choice([1, 255, 32768, 65535], 4)
        else:
            q = rng.integers(1, 256, 64) if kind else rng.integers(1, 4096, 64)
            lim = 32767 // q
            c = rng.integers(-lim, lim + 1)
            if kind == 2:
                keep = np.zeros(64, bool)
                keep[rng.choice(64, int(rng.integers(0, 6)), replace=False)] = True
                keep[0] = True
                c = np.where(keep, c, 0)
        out.append((c.astype(np.int16), q.astype(np.uint16)))
    return out


@pytest.mark.parametrize("n", [8, 4, 2, 1])
def test_host_idct_scaled_equals_model_on_random_units(n):
    import pjd_amd
    units = _random_units(np.random.default_rng(20261020 + n), 1200)
    for c, q in units:
        want = SM.idct_units(c[None, :], q, n)[0].reshape(n * n)
        got = pjd_amd.libjpeg_idct_scaled(c, q, n)
        assert got.shape == (n * n,) and np.array_equal(got, want), (n, c.tolist(), q.tolist())
    c, q = units[0]
    assert np.array_equal(pjd_amd.libjpeg_idct_scaled(c, q, 8), pjd_amd.libjpeg_idct(c, q))


def test_host_idct_scaled_never_reads_what_the_text_skips():
    """Column and row 4 at 4x4; columns and rows 2, 4, 6 at 2x2; everything but d[0] at 1x1."""
    import pjd_amd
    rng = np.random.default_rng(7)
    q = rng.integers(1, 64, 64).astype(np.uint16)
    c = rng.integers(-200, 200, 64).astype(np.int16)
    for n, skipped in ((4, [4]), (2, [2, 4, 6]), (1, [1, 2, 3, 4, 5, 6, 7])):
        c2 = c.reshape(8, 8).copy()
        for k in skipped:
            c2[k, :] = 12345 if n > 1 else c2[k, :] + 999
            c2[:, k] = -12345 if n > 1 else c2[:, k] - 999
        if n == 1:
            c2[0, 0] = c[0]
        assert np.array_equal(pjd_amd.libjpeg_idct_scaled(c, q, n), pjd_amd.libjpeg_idct_scaled(c2.reshape(64), q, n)), n


def test_host_idct_scaled_refuses_other_sizes():
    import pjd_amd
    L = pjd_amd.dev_lib()
    c, q, out = (C.c_int16 * 64)(), (C.c_uint16 * 64)(), (C.c_uint8 * 64)()
    for n in (0, 3, 5, 6, 7, 16, 0xffffffff):
        assert L.pjd_libjpeg_idct_scaled(c, q, n, out) == E_ARG, n
    assert L.pjd_libjpeg_idct_scaled(None, q, 4, out) == E_ARG and L.pjd_libjpeg_idct_scaled(c, q, 4, None) == E_ARG
    for n in (8, 4, 2, 1):
        assert L.pjd_libjpeg_idct_scaled(c, q, n, out) == 0 and out[0] == 128


def _desc(name, flags):
    import pjd_amd
    c = manifest()["cases"][name]
    s = pjd_amd.Scanned(jpeg(name), options=pjd_amd.SCAN_PROGRESSIVE if c["progressive"] else 0)
    assert s.valid, s.log
    s.desc.flags = int(s.desc.flags) | flags
    return s


def test_sizes_are_the_reduced_ones():
    import pjd_amd
    for name, c in manifest()["cases"].items():
        for s in SCALES:
            ow, oh = out_size(c, s)
            assert pjd_amd.scaled_dims(c["width"], c["height"], pjd_amd.F_LIBJPEG | FLAG[s]) == (ow, oh)
            sc = _desc(name, pjd_amd.F_LIBJPEG | FLAG[s])
            assert pjd_amd.image_output_size(sc.desc, pjd_amd.OUT_RGB8) == 3 * ow * oh
            assert pjd_amd.image_output_size(sc.desc, pjd_amd.OUT_RGB8_PLANAR) == 3 * ow * oh
            assert pjd_amd.image_output_size(sc.desc, pjd_amd.OUT_GRAY8) == ow * oh
            assert pjd_amd.image_output_size(sc.desc, pjd_amd.OUT_BMP) == 26 + oh * (3 * ow + ow % 4)
            from pjd_amd import tensors as T
            assert T.output_hw(sc.desc) == (oh, ow)
    for w, h in ((65535, 65535), (1, 1), (9, 8)):
        assert pjd_amd.scaled_dims(w, h, pjd_amd.F_LIBJPEG | 384) == (-(-w // 8), -(-h // 8))


def _check(descs, fmt=None):
    """pjd_plan_check -> (rc, reason)."""
    import pjd_amd
    return pjd_amd.plan_check(descs, pjd_amd.OUT_RGB8 if fmt is None else fmt)


def test_plan_check_refusals_new_and_old():
    import pjd_amd
    ok = _desc("ls_16x16_420_q50", pjd_amd.F_LIBJPEG | 256)
    for fmt in (pjd_amd.OUT_RGB8, pjd_amd.OUT_BMP, pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_GRAY8):
        assert _check([ok.desc], fmt)[0] == 0
    for bits in (128, 256, 384):
        s = _desc("ls_16x16_420_q50", bits)                                    # a new bit without PJD_F_LIBJPEG
        rc, why = _check([ok.desc, s.desc])
        assert rc == E_ARG and "image 1" in why and "PJD_F_LIBJPEG" in why, why
        s = _desc("ls_16x16_420_q50", pjd_amd.F_LIBJPEG | bits | pjd_amd.F_SCALE_1_2)      # ... and together with PJD_F_SCALE_*
        rc, why = _check([ok.desc, ok.desc, s.desc])
        assert rc == E_ARG and "image 2" in why and "PJD_F_SCALE" in why and "PJD_F_LIBJPEG_SCALE" in why, why
        s = _desc("ls_16x16_420_q50", bits | pjd_amd.F_SCALE_1_4)
        assert _check([s.desc])[0] == E_ARG
    s = _desc("ls_16x16_420_q50", pjd_amd.F_LIBJPEG | pjd_amd.F_SCALE_1_2)     # the old refusal, as it was
    rc, why = _check([s.desc])
    assert rc == E_ARG and "image 0" in why and "PJD_F_SCALE" in why and "PJD_F_LIBJPEG_SCALE" not in why, why
    # mixed batches are fine: every scale, flagged full size, unflagged, box-scaled
    mixed = [_desc("ls_33x31_420_q90", f) for f in (pjd_amd.F_LIBJPEG, pjd_amd.F_LIBJPEG | 128, pjd_amd.F_LIBJPEG | 256, pjd_amd.F_LIBJPEG | 384, 0,
                                                    pjd_amd.F_SCALE_1_4)]
    assert _check([m.desc for m in mixed])[0] == 0


def test_device_bytes_of_the_plan_shrink_with_the_scale():
    import pjd_amd
    full = _desc("ls_136x72_420_q90", pjd_amd.F_LIBJPEG)
    quarter = _desc("ls_136x72_420_q90", pjd_amd.F_LIBJPEG | 256)
    a, b = pjd_amd.plan_info([full.desc]), pjd_amd.plan_info([quarter.desc])
    assert b["out_bytes"] == 3 * 34 * 18 and a["out_bytes"] == 3 * 136 * 72
    assert a["n_data_units"] == b["n_data_units"]


def test_pick_libjpeg_scale_flags():
    from pjd_amd import tensors as T
    assert T.pick_libjpeg_scale_flags(1024, 768, 224, 224) == 128          # 1/2: 512 x 384; 1/4 would be 256 x 192 < 224
    assert T.pick_libjpeg_scale_flags(1024, 1024, 224, 224) == 256
    assert T.pick_libjpeg_scale_flags(2000, 1800, 224, 224) == 384
    assert T.pick_libjpeg_scale_flags(1793, 1785, 224, 224) == 384         # ceil: 225 x 224
    assert T.pick_libjpeg_scale_flags(1792, 1784, 224, 224) == 256         # 224 x 223 at 1/8
    assert T.pick_libjpeg_scale_flags(100, 100, 224, 224) == 0
    assert T.pick_libjpeg_scale_flags(447, 448, 224, 224) == 128 and T.pick_libjpeg_scale_flags(446, 448, 224, 224) == 0
    for w, h, tw, th in ((640, 480, 64, 64), (33, 31, 5, 4), (136, 72, 17, 9)):
        assert T.pick_libjpeg_scale_flags(w, h, tw, th) >> 7 == T.pick_scale_flags(w, h, tw, th) >> 4


def test_tensors_keyword_errors():
    """draft needs libjpeg=True; prescale=True with libjpeg=True keeps raising; all before anything is created (ctx is never touched)."""
    from pjd_amd import tensors as T
    sc = _desc("ls_136x72_420_q90", 0)                 # (a Scanned owns what its descriptor points to: it has to stay alive)
    d = [sc.desc]
    with pytest.raises(ValueError, match="draft needs libjpeg=True"):
        T.decode_resized_batch_tensor(None, d, (16, 16), prescale=False, draft=True)
    with pytest.raises(ValueError, match="draft needs libjpeg=True"):
        T.decode_normalized_batch_tensor(None, d, (16, 16), [0.5] * 3, [0.5] * 3, prescale=True, draft=True)
    with pytest.raises(ValueError, match="draft needs libjpeg=True"):
        T.decode_to_tensors(None, d, draft=2)
    with pytest.raises(ValueError, match="denominator"):
        T.decode_to_tensors(None, d, libjpeg=True, draft=3)
    with pytest.raises(ValueError, match="denominator"):
        T.decode_to_tensors(None, d, libjpeg=True, draft=True)
    with pytest.raises(ValueError, match="prescale=False"):
        T.decode_resized_batch_tensor(None, d, (16, 16), prescale=True, libjpeg=True, draft=True)
    with pytest.raises(ValueError, match="prescale=False"):
        T.decode_resized_batch_tensor(None, d, (16, 16), libjpeg=True)
    # the copies a drafted call decodes: flagged, at the picked scale; the caller's descriptor untouched
    run = T.drafted_descs(T.libjpeg_descs(d), (16, 30))
    import pjd_amd
    assert int(run[0].flags) & (pjd_amd.F_LIBJPEG | pjd_amd.F_LIBJPEG_SCALE_MASK) == pjd_amd.F_LIBJPEG | 256 and T.output_hw(run[0]) == (18, 34)
    assert int(d[0].flags) & (pjd_amd.F_LIBJPEG | pjd_amd.F_LIBJPEG_SCALE_MASK) == 0


def _cli(*args):
    exe = os.path.join(ROOT, "bin", "decoder")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # a refusal comes before any device is opened
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=60)


def test_cli_refusals():
    f = os.path.join(GOLD, "ls_16x16_420_q50.jpg")
    r = _cli("--draft", "1/2", f)
    assert r.returncode == 1 and "--draft needs --libjpeg" in r.stdout, r.stdout
    r = _cli("--libjpeg", "--scale", "1/2", f)
    assert r.returncode == 1 and "--libjpeg takes no --scale" in r.stdout, r.stdout
    r = _cli("--libjpeg", "--draft", "1/2", "--scale", "1/4", f)
    assert r.returncode == 1 and "--libjpeg takes no --scale" in r.stdout, r.stdout
    for bad in ("1/3", "2", ""):
        r = _cli("--libjpeg", "--draft", bad, f)
        assert r.returncode == 1 and "Invalid arguments" in r.stdout, (bad, r.stdout)
