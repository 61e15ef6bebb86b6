"""PJD_F_LIBJPEG on the host (no GPU): the numpy model of the arithmetic in include/pjd.h (tests/libjpeg_model.py) equals Pillow's decode
of every baseline fixture under tests/golden/libjpeg/ byte for byte, and the three host entry points -- the inlines the kernels run --
equal the model.  Zero tolerance everywhere: the arithmetic is integer."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

import libjpeg_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "libjpeg")


def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)


def fixture(name):
    c = manifest()["cases"][name]
    with open(os.path.join(GOLD, name + ".jpg"), "rb") as f:
        data = f.read()
    with open(os.path.join(GOLD, name + ".rgb"), "rb") as f:
        rgb = np.frombuffer(f.read(), np.uint8).reshape(c["height"], c["width"], 3)
    return data, rgb, c


def baseline_cases():
    return sorted(n for n, c in manifest()["cases"].items() if not c["progressive"] and not c["restart_marker_blocks"])


def model_from_port(port, data):
    """The model fed the oracle port's coefficients under the T.81 zigzag and its quantisers."""
    port.standard_zigzag(True)
    try:
        d = port.decode(data)
    finally:
        port.standard_zigzag(False)
    info = d["info"]
    assert d["huff_rc"] == 0
    qts = [info["qt"][info["comp_qt"][k]] for k in range(info["ncomp"])]
    return M.decode(d["coef"], qts, info["width"], info["height"], info["ncomp"], info["hsamp"], info["vsamp"])


def test_fixture_set_is_the_one_the_mode_is_specified_on():
    cases = manifest()["cases"]
    have = {(c["width"], c["height"], c["sampling"]) for c in cases.values()}
    for want in [(8, 8, "4:4:4"), (16, 16, "4:2:0"), (17, 17, "4:2:0"), (33, 31, "4:2:0"), (40, 24, "4:2:2"), (61, 45, "grey"),
                 (3, 5, "4:2:0"), (3, 5, "4:2:2"), (4, 9, "4:2:0"), (4, 9, "4:2:2"), (5, 4, "4:2:0"), (5, 4, "4:2:2"), (136, 72, "4:2:0")]:
        assert want in have, want
    assert {c["quality"] for c in cases.values()} >= {50, 90, 100}
    assert any(c["progressive"] for c in cases.values()) and any(c["restart_marker_blocks"] == 4 for c in cases.values())
    assert all(c["width"] <= 136 and c["height"] <= 72 for c in cases.values())
    assert manifest()["pillow"]


@pytest.mark.parametrize("name", baseline_cases())
def test_model_equals_recorded_pillow_decode(port, name):
    data, rgb, _ = fixture(name)
    got = model_from_port(port, data)
    assert got.shape == rgb.shape and np.array_equal(got, rgb), f"{name}: {int((got != rgb).sum())} bytes differ"


@pytest.mark.parametrize("name", baseline_cases())
def test_recorded_decode_is_this_pillows(name):
    """Where Pillow is installed its decode of the fixture is the recorded one (a libjpeg whose defaults differ would show here)."""
    Image = pytest.importorskip("PIL.Image")
    data, rgb, _ = fixture(name)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), rgb)


def test_symbols_and_flag_exist():
    import pjd_amd
    assert pjd_amd.F_LIBJPEG == 64
    L = pjd_amd.dev_lib()
    for sym in ("pjd_libjpeg_idct", "pjd_libjpeg_ycc_to_rgb", "pjd_libjpeg_upsample_row"):
        assert hasattr(L, sym), sym
    assert pjd_amd.F_LIBJPEG & (pjd_amd.F_SCALE_MASK | pjd_amd.F_PROGRESSIVE | pjd_amd.F_STANDARD_ZIGZAG | pjd_amd.F_STANDARD_RESTART |
                                pjd_amd.F_FORCE_SEQUENTIAL) == 0


def test_host_idct_equals_model_on_random_units():
    """2000 seeded units, sparse and dense, every dequantised value within int16 (libjpeg's own envelope)."""
    import pjd_amd
    rng = np.random.default_rng(20261018)
    coefs, qs = [], []
    for k in range(2000):
        q = rng.integers(1, 256, 64) if k % 3 else rng.integers(1, 4096, 64)
        lim = 32767 // q
        c = rng.integers(-lim, lim + 1)
        if k % 2:                                                   # sparse: a DC and a few low-frequency terms
            keep = np.zeros(64, bool)
            keep[rng.choice(64, int(rng.integers(0, 6)), replace=False)] = True
            keep[0] = True
            c = np.where(keep, c, 0)
        assert np.abs(c * q).max() <= 32767
        coefs.append(c.astype(np.int16)); qs.append(q.astype(np.uint16))
    for c, q in zip(coefs, qs):
        want = M.idct_units(c[None, :], q)[0].reshape(64)
        assert np.array_equal(pjd_amd.libjpeg_idct(c, q), want)


def test_host_idct_flat_unit_is_dc_shortcut():
    """A unit with only a DC term: every sample is clamp(((dc * q) << 2 rounded through pass 2) + 128): libjpeg's zero-AC shortcut."""
    import pjd_amd
    for dc, q in [(0, 16), (5, 16), (-7, 3), (100, 8), (-128, 8), (127, 9)]:
        c = np.zeros(64, np.int16); c[0] = dc
        out = pjd_amd.libjpeg_idct(c, np.full(64, q, np.uint16))
        want = min(max((((dc * q) << 2) * 8192 + (1 << 17)) >> 18, -128), 127) + 128
        assert (out == want).all(), (dc, q)


def test_host_colour_equals_model_on_a_grid():
    import pjd_amd
    vals = sorted(set(range(0, 256, 32)) | {0, 127, 128, 255})
    y, cb, cr = np.meshgrid(vals, vals, vals, indexing="ij")
    want = M.ycc_to_rgb(y.ravel(), cb.ravel(), cr.ravel())
    for k, (a, b, c) in enumerate(zip(y.ravel(), cb.ravel(), cr.ravel())):
        assert pjd_amd.libjpeg_ycc_to_rgb(a, b, c) == tuple(int(v) for v in want[k]), (a, b, c)
    assert pjd_amd.libjpeg_ycc_to_rgb(77, 128, 128) == (77, 77, 77)


@pytest.mark.parametrize("n", range(1, 10))
def test_host_upsample_row_equals_model(n):
    import pjd_amd
    rng = np.random.default_rng(n)
    for _ in range(20):
        cur, nb = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
        assert np.array_equal(pjd_amd.libjpeg_upsample_row(cur), M.upsample_row(cur))
        for v in (0, 1):
            assert np.array_equal(pjd_amd.libjpeg_upsample_row(cur, nb, v), M.upsample_row(cur, nb))
    lo, hi = np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    assert (pjd_amd.libjpeg_upsample_row(hi, hi) == 255).all() and (pjd_amd.libjpeg_upsample_row(lo, lo) == 0).all()


def test_host_functions_refuse_null_and_empty():
    import pjd_amd
    L = pjd_amd.dev_lib()
    c, q, o = (C.c_int16 * 64)(), (C.c_uint16 * 64)(), (C.c_uint8 * 64)()
    assert L.pjd_libjpeg_idct(None, q, o) == -3 and L.pjd_libjpeg_idct(c, None, o) == -3 and L.pjd_libjpeg_idct(c, q, None) == -3
    assert L.pjd_libjpeg_ycc_to_rgb(1, 2, 3, None) == -3
    row, out = (C.c_uint8 * 4)(), (C.c_uint8 * 8)()
    assert L.pjd_libjpeg_upsample_row(None, None, 0, 4, out) == -3 and L.pjd_libjpeg_upsample_row(row, None, 0, 4, None) == -3
    assert L.pjd_libjpeg_upsample_row(row, None, 0, 0, out) == -3
    assert L.pjd_libjpeg_upsample_row(row, None, 0, 4, out) == 0


def test_planner_accepts_and_refuses_without_a_device():
    """pjd_plan_info runs the planner the batch runs: the flag is accepted on the envelope's samplings and refused with an output
    scale; a batch with a flagged picture counts its plane buffer nowhere else than in device memory (coef_bytes stays)."""
    import pjd_amd
    data, _, _ = fixture("lj_17x17_420_q90")
    s = pjd_amd.Scanned(data)
    plain = pjd_amd.plan_info([s.desc])
    from pjd_amd import tensors
    d = tensors.libjpeg_descs([s.desc])[0]
    assert d.flags == s.desc.flags | pjd_amd.F_LIBJPEG and s.desc.flags & pjd_amd.F_LIBJPEG == 0       # a copy
    flagged = pjd_amd.plan_info([d])
    assert flagged["n_data_units"] == plain["n_data_units"] and flagged["out_bytes"] == plain["out_bytes"]
    d.flags |= pjd_amd.F_SCALE_1_2
    with pytest.raises(Exception):
        pjd_amd.plan_info([d])


def test_tensors_argument_checks_need_no_device():
    import pjd_amd
    from pjd_amd import tensors
    data, _, _ = fixture("lj_17x17_420_q90")
    s = pjd_amd.Scanned(data)
    with pytest.raises(ValueError, match="prescale"):
        tensors.decode_resized_batch_tensor(None, [s.desc], (8, 8), libjpeg=True)                     # prescale defaults to True
    with pytest.raises(ValueError, match="prescale"):
        tensors.decode_normalized_batch_tensor(None, [s.desc], (8, 8), (0.5,) * 3, (0.5,) * 3, libjpeg=True)
    scaled = tensors.prescaled_descs([s.desc], (2, 2))
    assert scaled[0].flags & pjd_amd.F_SCALE_MASK
    for call in (lambda: tensors.decode_to_tensors(None, scaled, libjpeg=True),
                 lambda: tensors.decode_to_batch_tensor(None, scaled, libjpeg=True),
                 lambda: tensors.decode_resized_batch_tensor(None, scaled, (8, 8), prescale=False, libjpeg=True)):
        with pytest.raises(ValueError, match="output scale"):
            call()


def test_cli_refuses_the_flag_with_a_scale_and_with_split():
    """bin/decoder --libjpeg: refused, with a message and before any device is opened, with --scale other than 1/1 and with --split."""
    import subprocess
    exe = os.path.join(os.path.dirname(HERE), "bin", "decoder")
    for extra, word in ((["--scale", "1/2"], "--scale"), (["--scale", "1/8"], "--scale"), (["--split"], "--split")):
        r = subprocess.run([exe, "--libjpeg"] + extra + ["x.jpg"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--libjpeg" in r.stdout and word in r.stdout, (extra, r.stdout)
