"""Orientation on decode, the parts that need no device: the scanner's EXIF orientation tag (pjd_scanned_orientation, the rule of
include/pjd_host.h) on the hand-built fixtures of tests/golden/exif/, Pillow as a second opinion where it is installed, the reader
under AddressSanitizer + UBSan in a stand-alone program, the numpy model (tests/orientation_model.py) against numpy's and Pillow's
own rotations, and the pure helpers of pjd_amd.tensors by brute force."""
import ctypes as C
import glob
import importlib.util
import io
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import orientation_model as om
from conftest import golden_bytes, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
EXIF = os.path.join(HERE, "golden", "exif")
MANIFEST = json.load(open(os.path.join(EXIF, "manifest.json")))
FIXTURES = sorted(MANIFEST["fixtures"])
WELL_FORMED = [n for n in FIXTURES if MANIFEST["fixtures"][n]["well_formed"]]


def _bytes(name):
    with open(os.path.join(EXIF, name + ".jpg"), "rb") as f:
        return f.read()


def _pillow():
    return pytest.importorskip("PIL.Image", reason="Pillow is not installed: the numpy model is the norm")


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_covers_the_rule():
    fx = MANIFEST["fixtures"]
    for bo in ("ii", "mm"):
        assert [fx[f"exif_{bo}_{v}"]["orientation"] for v in range(1, 9)] == list(range(1, 9))
    assert fx["exif_behind_jfif_6"]["orientation"] == 6 and fx["exif_behind_xmp_8"]["orientation"] == 8
    bad = [n for n in FIXTURES if n.startswith("bad_")]
    assert len(bad) >= 12 and all(fx[n]["orientation"] == 1 and not fx[n]["well_formed"] for n in bad)
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(EXIF, "*.jpg"))) == FIXTURES


def test_the_committed_fixtures_are_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("make_exif_fixtures", os.path.join(EXIF, "make_exif_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    base = golden_bytes(MANIFEST["base"])
    made = {name: (seg, want, wf) for name, seg, want, wf in gen.fixtures()}
    assert sorted(made) == FIXTURES
    for name, (seg, want, wf) in made.items():
        assert (want, wf) == (MANIFEST["fixtures"][name]["orientation"], MANIFEST["fixtures"][name]["well_formed"])
        if seg is not None:
            assert _bytes(name) == base[:2] + seg + base[2:], name


@pytest.mark.parametrize("name", FIXTURES)
def test_scanner_reads_the_orientation(name):
    import pjd_amd
    s = pjd_amd.Scanned(_bytes(name))
    assert s.orientation == MANIFEST["fixtures"][name]["orientation"]
    assert s.valid == MANIFEST["fixtures"][name]["valid_jpeg"]


def test_files_without_a_segment_have_orientation_1(manifest):
    import pjd_amd
    for n in sorted(manifest)[::5] + ["neg_empty", "neg_not_jpeg"]:
        assert pjd_amd.Scanned(golden_bytes(n)).orientation == 1, n


def _desc_fields(s):
    d = s.desc
    out = {}
    for name, typ in d._fields_:
        v = getattr(d, name)
        if name in ("ecs", "seg_offsets") or isinstance(v, (C._Pointer, C.c_void_p)) or "POINTER" in repr(typ):
            continue
        out[name] = bytes(memoryview(v).cast("B")) if isinstance(v, (C.Array, C.Structure)) else v
    return out


@pytest.mark.parametrize("name", [n for n in FIXTURES if MANIFEST["fixtures"][n]["valid_jpeg"]])
def test_descriptor_and_log_are_those_of_the_file_without_the_segment(name):
    import pjd_amd
    a, b = pjd_amd.Scanned(golden_bytes(MANIFEST["base"]), name="f.jpg"), pjd_amd.Scanned(_bytes(name), name="f.jpg")
    assert (a.rc, a.valid, a.log) == (b.rc, b.valid, b.log) and a.valid
    fa, fb = _desc_fields(a), _desc_fields(b)
    assert fa == fb and {"width", "height", "flags", "ecs_len", "n_segments"} <= set(fa)
    assert np.array_equal(a.ecs(), b.ecs()) and np.array_equal(a.seg_offsets(), b.seg_offsets())
    assert np.array_equal(a.metadata(), b.metadata())


@pytest.mark.parametrize("name", WELL_FORMED)
def test_pillow_reads_the_same_tag(name):
    Image = _pillow()
    with Image.open(io.BytesIO(_bytes(name))) as im:
        assert im.getexif().get(0x0112) == MANIFEST["fixtures"][name]["orientation"]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_orient_is_numpys_rotations_and_mirrors():
    Q = np.random.default_rng(7).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    assert np.array_equal(om.orient(Q, 1), Q)
    assert np.array_equal(om.orient(Q, 2), Q[:, ::-1]) and np.array_equal(om.orient(Q, 4), Q[::-1])
    assert np.array_equal(om.orient(Q, 3), np.rot90(Q, 2))
    assert np.array_equal(om.orient(Q, 5), Q.transpose(1, 0, 2)) and np.array_equal(om.orient(Q, 7), np.rot90(Q, 2).transpose(1, 0, 2))
    assert np.array_equal(om.orient(Q, 6), np.rot90(Q, -1)) and np.array_equal(om.orient(Q, 8), np.rot90(Q, 1))
    assert len({om.orient(Q, o).tobytes() + bytes(om.orient(Q, o).shape) for o in range(1, 9)}) == 8


def test_exif_transpose_of_the_oracles_picture_equals_orient(port):
    Image = _pillow()
    from PIL import ImageOps
    rgb = port.decode(golden_bytes(MANIFEST["base"]))["rgb"]
    assert rgb.shape == (45, 61, 3)
    for o in range(1, 9):
        im = Image.fromarray(rgb)
        ex = im.getexif()
        ex[0x0112] = o
        im.info["exif"] = ex.tobytes()
        buf = io.BytesIO()
        im.save(buf, format="PNG", exif=ex.tobytes())
        with Image.open(io.BytesIO(buf.getvalue())) as tagged:
            assert tagged.getexif().get(0x0112) == o
            up = np.asarray(ImageOps.exif_transpose(tagged))
        assert np.array_equal(up, om.orient(rgb, o)), o


def test_wrong_models_differ_from_the_model_on_an_asymmetric_picture():
    rgb = np.random.default_rng(3).integers(0, 256, (45, 61, 3), dtype=np.uint8)
    met = set()
    for o in range(1, 9):
        for win in (None, dict(x=3, y=5, w=40, h=30, flags=1), dict(vw=40, vh=40, ox=2, oy=1), dict(vh=40, oy=3)):
            want = om.oriented(rgb, win, 30, 20, o)
            met |= om.assert_not_a_wrong_model(rgb, win, 30, 20, o, "bilinear", want, (o, win))
    assert met == {"ignored", "no_mirrors", "exchanged_6_8", "mirrors_first", "unswapped_target"}


# ---- the reader under the sanitizers -----------------------------------------------------------------------------------------------------
def test_exif_reader_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "exif_host_fuzz"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "exif_host_fuzz.cpp"), os.path.join(ROOT, "pim-jpeg-decoder_amd", "host", "pjd_scan.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("this toolchain has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    files = [os.path.join(EXIF, n + ".jpg") for n in FIXTURES]
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    hist = [int(x) for x in r.stdout.split("orientations 1..8:")[1].split("\n")[0].split()]
    assert len(hist) == 8 and all(h > 0 for h in hist), "the mutations reach every value"


# ---- the pure helpers ---------------------------------------------------------------------------------------------------------------------
def test_orient_hw_and_orient_then_hflip():
    from pjd_amd import tensors
    Q = np.arange(5 * 7).reshape(5, 7)
    for o in range(1, 9):
        assert tensors.orient_hw(o, 5, 7) == om.orient(Q, o).shape
        assert tensors.orient_hw(o, *tensors.orient_hw(o, 5, 7)) == (5, 7)
        assert np.array_equal(om.orient(Q, tensors.orient_then_hflip(o)), om.orient(Q, o)[:, ::-1]), o
    assert [tensors.orient_then_hflip(o) for o in range(1, 9)] == [2, 1, 4, 3, 6, 5, 8, 7]
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            tensors.orient_hw(bad, 5, 7)
        with pytest.raises(ValueError):
            tensors.orient_then_hflip(bad)


def test_crop_to_stored_by_brute_force():
    """Every pixel of a small stored picture carries its index: crop-then-orient equals orient-then-mapped-crop, for every orientation and
    every crop of the upright picture."""
    from pjd_amd import tensors
    H, W = 4, 6
    S = np.arange(H * W).reshape(H, W)
    n = 0
    for o in range(1, 9):
        U = om.orient(S, o)
        UH, UW = U.shape
        for x, y in itertools.product(range(UW), range(UH)):
            for w, h in itertools.product(range(1, UW - x + 1), range(1, UH - y + 1)):
                xs, ys, ws, hs = tensors.crop_to_stored(o, (x, y, w, h), W, H)
                assert 0 <= xs and xs + ws <= W and 0 <= ys and ys + hs <= H
                assert np.array_equal(om.orient(S[ys:ys + hs, xs:xs + ws], o), U[y:y + h, x:x + w]), (o, x, y, w, h)
                n += 1
        for bad in ((UW, 0, 1, 1), (0, 0, UW + 1, 1), (0, 0, 1, UH + 1), (-1, 0, 1, 1), (0, 0, 0, 1)):
            with pytest.raises(ValueError):
                tensors.crop_to_stored(o, bad, W, H)
    assert n == 8 * (W * (W + 1) // 2) * (H * (H + 1) // 2)


def _desc(w, h):
    import pjd_amd
    d = pjd_amd.ImageDesc()
    d.width, d.height = w, h
    return d


def test_the_plan_of_the_tensor_helpers_is_orient_then_crop_then_flip():
    """tensors._plan with orientations, emulated with the model where the resample is the identity (the target is the crop's own size, so
    every tap weight is 0 or 1): the windows and orientations it hands to the batch deliver exactly flip(orient(P, o)[crop])."""
    from pjd_amd import tensors
    rng = np.random.default_rng(11)
    P = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)           # the stored picture
    for o in range(1, 9):
        U = om.orient(P, o)
        UH, UW = U.shape[:2]
        for flip in (False, True):
            x, y, w, h = 2, 1, UW - 4, UH - 3
            run, wins, oris = tensors._plan_outputs([_desc(13, 9)], (h, w), False, [(x, y, w, h)], [flip], [o])[:3]
            assert len(run) == 1 and not (wins[0] or {}).get("flags"), "the flip is folded into the orientation"
            got = om.oriented(P, wins[0], w, h, oris[0])
            want = U[y:y + h, x:x + w]
            assert np.array_equal(got, want[:, ::-1] if flip else want), (o, flip)
        # Resize(short side) + CenterCrop: the resize is the identity, the crop is torchvision's
        short = min(UH, UW)
        th, tw = UH - 3, UW - 2
        run, wins, oris = tensors._plan_outputs([_desc(13, 9)], (th, tw), False, None, None, [o], short)[:3]
        cc = tensors.center_crop_window((UH, UW), short, (th, tw))
        assert (cc["vw"], cc["vh"]) == (UW, UH)
        got = om.oriented(P, wins[0], tw, th, oris[0])
        assert np.array_equal(got, U[cc["oy"]:cc["oy"] + th, cc["ox"]:cc["ox"] + tw]), o
    # no orientations: the plan is what it was
    run, wins, oris = tensors._plan_outputs([_desc(13, 9)], (4, 4), False, [(1, 1, 5, 5)], [True], None)[:3]
    assert oris is None and wins == [dict(x=1, y=1, w=5, h=5, flags=1)]
    with pytest.raises(ValueError):
        tensors._plan_outputs([_desc(13, 9)], (4, 4), False, None, None, [9])
    with pytest.raises(ValueError):
        tensors._plan_outputs([_desc(13, 9)], (4, 4), False, None, None, [1, 1])
    with pytest.raises(ValueError):
        tensors._plan_outputs([_desc(13, 9)], (4, 4), False, [(0, 0, 13, 9)], None, [6])      # 13 x 9 is not inside the upright 9 x 13


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_exports_exist_and_the_version_stays_6():
    import pjd_amd
    L, Hl = pjd_amd.dev_lib(), pjd_amd.host_lib()
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert L.pjd_batch_set_orientation and Hl.pjd_scanned_orientation
    assert L.pjd_batch_set_orientation(None, None) == -3                                # PJD_E_ARG: no batch
    assert C.sizeof(pjd_amd.ResizeWindow) == 40
    assert hasattr(pjd_amd.Batch, "set_orientation")
