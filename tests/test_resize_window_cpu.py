"""Source windows of the resize on decode on the host (no GPU): pjd_resize_window_check -- the one implementation of the rules of
include/pjd.h -- rule by rule; tests/resize_window_model.py (crop -> model -> crop -> flip over the two numpy models that exist)
against torch's interpolate on the cropped tensor; the pure helpers of pjd_amd.tensors against values computed by hand."""
import ctypes as C

import numpy as np
import pytest

import resize_window_model as wm

E_ARG = -3
BL, AA = 0, 1


def _check(sw, sh, tw, th, win, filt=BL):
    import pjd_amd
    L = pjd_amd.dev_lib()
    rec = pjd_amd.ResizeWindow(**win) if win is not None else None
    return L.pjd_resize_window_check(sw, sh, tw, th, C.byref(rec) if rec is not None else None, filt)


def test_exports_exist_and_the_abi_version_is_unchanged():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert hasattr(L, "pjd_batch_set_resize_window") and hasattr(L, "pjd_resize_window_check")
    assert L.pjd_version() == 6 == pjd_amd.ABI_VERSION
    assert pjd_amd.RW_HFLIP == 1 == wm.HFLIP
    assert C.sizeof(pjd_amd.ResizeWindow) == 40 and [k for k, _ in pjd_amd.ResizeWindow._fields_][:9] == list(wm.FIELDS)
    assert callable(pjd_amd.Batch.set_resize_window) and callable(pjd_amd.resize_window_check)


# (what, sw, sh, tw, th, window, filter): accepted
ACCEPTED = [
    ("the zero record is the identity", 61, 45, 7, 5, {}, BL),
    ("the zero record, antialiased", 61, 45, 7, 5, {}, AA),
    ("a window that fills the picture", 61, 45, 7, 5, dict(x=0, y=0, w=61, h=45), BL),
    ("a window in the last column and row", 61, 45, 7, 5, dict(x=60, y=44, w=1, h=1), BL),
    ("flags alone", 61, 45, 7, 5, dict(flags=1), BL),
    ("a virtual target with the delivered part at its far corner", 61, 45, 7, 5, dict(vw=20, vh=10, ox=13, oy=5), BL),
    ("vw alone: vh defaults to th", 61, 45, 7, 5, dict(vw=65535, ox=65528), BL),
    ("vh alone: vw defaults to tw", 61, 45, 7, 5, dict(vh=6, oy=1), BL),
    ("a picture past 16x its target whose window is inside", 200, 120, 4, 4, dict(x=100, y=40, w=64, h=64), AA),
    ("a window at exactly 16x", 65, 65, 4, 4, dict(x=1, y=1, w=64, h=64), AA),
    ("past 16x is no error for the bilinear filter", 200, 120, 4, 4, {}, BL),
    ("the 16x limit is against the virtual target", 200, 120, 4, 4, dict(vw=13, vh=8, ox=9, oy=4), AA),
]

# (what, sw, sh, tw, th, window, filter): PJD_E_ARG
REFUSED = [
    ("w == 0 but h != 0", 61, 45, 7, 5, dict(h=10), BL),
    ("h == 0 but w != 0", 61, 45, 7, 5, dict(w=10), BL),
    ("a zero window with x", 61, 45, 7, 5, dict(x=1), BL),
    ("a zero window with y", 61, 45, 7, 5, dict(y=1), BL),
    ("x + w > sw", 61, 45, 7, 5, dict(x=41, y=0, w=21, h=15), BL),
    ("y + h > sh", 61, 45, 7, 5, dict(x=0, y=31, w=21, h=15), BL),
    ("x + w wraps 32 bits", 61, 45, 7, 5, dict(x=2 ** 32 - 1, y=0, w=2, h=15), BL),
    ("vw above 65535", 61, 45, 7, 5, dict(vw=65536), BL),
    ("vh above 65535", 61, 45, 7, 5, dict(vh=65536), BL),
    ("ox + tw > vw", 61, 45, 7, 5, dict(vw=20, ox=14), BL),
    ("oy + th > vh", 61, 45, 7, 5, dict(vh=10, oy=6), BL),
    ("ox with the default vw", 61, 45, 7, 5, dict(ox=1), BL),
    ("oy with the default vh", 61, 45, 7, 5, dict(oy=1), BL),
    ("vw below tw", 61, 45, 7, 5, dict(vw=6), BL),
    ("an unknown flag bit", 61, 45, 7, 5, dict(flags=2), BL),
    ("the top flag bit", 61, 45, 7, 5, dict(flags=0x80000001), BL),
    ("reserved_ set", 61, 45, 7, 5, dict(reserved_=1), BL),
    ("antialias: w > 16 * vw", 200, 120, 4, 4, dict(x=100, y=40, w=65, h=64), AA),
    ("antialias: h > 16 * vh", 200, 120, 4, 4, dict(x=100, y=40, w=64, h=65), AA),
    ("antialias: the whole picture past 16x", 200, 120, 4, 4, {}, AA),
    ("an unknown filter", 61, 45, 7, 5, {}, 2),
    ("sw == 0", 0, 45, 7, 5, {}, BL),
    ("tw above 65535", 61, 45, 65536, 5, {}, BL),
    ("a null record", 61, 45, 7, 5, None, BL),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c[0])
def test_window_check_accepts(case):
    _, sw, sh, tw, th, win, filt = case
    import pjd_amd
    assert _check(sw, sh, tw, th, win, filt) == 0
    assert pjd_amd.resize_window_check(sw, sh, tw, th, win or None, filt) is True
    wm.resolve(win, sw, sh, tw, th)                        # the model's own assertions agree


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c[0])
def test_window_check_refuses(case):
    _, sw, sh, tw, th, win, filt = case
    assert _check(sw, sh, tw, th, win, filt) == E_ARG


def test_python_wrapper_takes_tuples_dicts_and_records():
    import pjd_amd
    assert pjd_amd.resize_window_check(61, 45, 7, 5, (40, 30, 21, 15))
    assert not pjd_amd.resize_window_check(61, 45, 7, 5, (41, 30, 21, 15))
    assert pjd_amd.resize_window_check(61, 45, 7, 5, (0, 0, 61, 45, 20, 10, 13, 5, pjd_amd.RW_HFLIP))
    assert pjd_amd.resize_window_check(61, 45, 7, 5, pjd_amd.ResizeWindow(vw=20, ox=13))
    assert not pjd_amd.resize_window_check(200, 120, 4, 4, None, pjd_amd.RESIZE_ANTIALIAS)
    w = pjd_amd.resize_window({"x": 1, "y": 2, "w": 3, "h": 4, "flags": 1})
    assert (w.x, w.y, w.w, w.h, w.vw, w.vh, w.ox, w.oy, w.flags, w.reserved_) == (1, 2, 3, 4, 0, 0, 0, 0, 1, 0)
    for bad in ({"z": 1}, (1, 2, 3), (0, 0, 1, 1, 0, 0, 0, 0, 0, 1), (-1, 0, 1, 1)):
        with pytest.raises(ValueError):
            pjd_amd.resize_window(bad)


# ---- the model against torch on the cropped tensor --------------------------------------------------------------------------------------
def _picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 100 * np.sin(xx / 7.0 + seed), 127 + 90 * np.cos(yy / 11.0), (xx + yy) * 255 / (w + h)], -1) + rng.normal(0, 25, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _torch_resize(torch, crop, vw, vh, antialias):
    x = torch.from_numpy(crop.astype(np.float64)).permute(2, 0, 1)[None]
    return torch.nn.functional.interpolate(x, size=(vh, vw), mode="bilinear", align_corners=False, antialias=antialias)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "antialias"])
@pytest.mark.parametrize("seed", [1, 2])
def test_model_is_within_one_level_of_torch_on_the_cropped_tensor(seed, antialias):
    """A crop resized, resize(256)[centre 224] and a flipped crop with an offset, on two seeded pictures: the window model against
    interpolate over the cropped float64 tensor, rounded to nearest -- at most 1 level apart (the bound of include/pjd.h)."""
    torch = pytest.importorskip("torch")
    from pjd_amd import tensors
    w, h = (500, 375) if seed == 1 else (400, 480)
    P = _picture(w, h, seed)
    cc = tensors.center_crop_window((h, w), 256, (224, 224))
    cases = [(dict(x=37, y=21, w=301, h=255), 224, 224),
             (cc, 224, 224),
             (dict(x=100, y=50, w=160, h=120, vw=96, vh=80, ox=9, oy=6, flags=wm.HFLIP), 64, 64)]
    for win, tw, th in cases:
        r = wm.resolve(win, w, h, tw, th)
        got = wm.window(P, win, tw, th, antialias).astype(np.int64)
        ref = _torch_resize(torch, P[r["y"]:r["y"] + r["h"], r["x"]:r["x"] + r["w"]], r["vw"], r["vh"], antialias)
        ref = ref[r["oy"]:r["oy"] + th, r["ox"]:r["ox"] + tw]
        ref = ref[:, ::-1] if r["flags"] & wm.HFLIP else ref
        err = np.abs(got - np.rint(ref)).max()
        print(f"seed {seed} {'aa' if antialias else 'bilinear'} {win}: |model - round(torch)| max {err}")
        assert got.shape == (th, tw, 3) and err <= 1, (win, err)
        for name, wrong in wm.wrong_models(P, win, tw, th, antialias).items():
            assert wrong.shape == got.shape and not np.array_equal(wrong, got), (win, name)


def test_zero_record_is_the_unwindowed_model():
    import resize_aa_model as aa
    import resize_model
    P = _picture(61, 45, 3)
    assert np.array_equal(wm.window(P, None, 50, 33), resize_model.resize(P, 50, 33))
    assert np.array_equal(wm.window(P, {}, 7, 5, True), aa.resize(P, 7, 5))
    assert wm.wrong_models(P, None, 7, 5) == {}


# ---- the pure helpers of pjd_amd.tensors --------------------------------------------------------------------------------------------------
def test_center_crop_window_by_hand():
    from pjd_amd import tensors
    ccw = tensors.center_crop_window
    # 500 x 375 (w x h): short side 375 -> 256, long 500 -> int(256 * 500 / 375) = 341; (341 - 224) / 2 = 58.5 -> 58 (half to even)
    assert ccw((375, 500), 256, (224, 224)) == {"vw": 341, "vh": 256, "ox": 58, "oy": 16}
    # portrait 333 x 480: vw = 256, vh = int(256 * 480 / 333) = 369; (369 - 224) / 2 = 72.5 -> 72
    assert ccw((480, 333), 256, (224, 224)) == {"vw": 256, "vh": 369, "ox": 16, "oy": 72}
    # round half to even: v - t = 1 -> 0.5 -> 0;  v - t = 3 -> 1.5 -> 2
    assert ccw((100, 100), 65, (64, 64)) == {"vw": 65, "vh": 65, "ox": 0, "oy": 0}
    assert ccw((100, 100), 67, (64, 64)) == {"vw": 67, "vh": 67, "ox": 2, "oy": 2}
    assert ccw((100, 100), 66, (64, 63)) == {"vw": 66, "vh": 66, "ox": 2, "oy": 1}      # size is (H, W): rows 2 -> 1; columns 3 -> 1.5 -> 2
    # a square: w <= h takes the first branch, both sides resize_short
    assert ccw((64, 64), 73, (64, 64)) == {"vw": 73, "vh": 73, "ox": 4, "oy": 4}        # 9 / 2 = 4.5 -> 4
    for hw, rs, size in (((375, 500), 200, (224, 224)), ((375, 500), 256, (224, 342)), ((480, 333), 256, (370, 224))):
        with pytest.raises(ValueError):
            ccw(hw, rs, size)


def test_window_at_scale_by_hand():
    from pjd_amd import tensors
    was = tensors.window_at_scale
    assert was((37, 21, 301, 255), 0, 500, 375) == (37, 21, 301, 255)                  # s = 1: the crop itself
    # s = 2, picture 250 x 188: x 37 >> 1 = 18, ceil(338 / 2) = 169; y 21 >> 1 = 10, ceil(276 / 2) = 138
    assert was((37, 21, 301, 255), 1, 250, 188) == (18, 10, 151, 128)
    # s = 8, picture 63 x 47: x 4, ceil(338 / 8) = 43; y 2, ceil(276 / 8) = 35
    assert was((37, 21, 301, 255), 3, 63, 47) == (4, 2, 39, 33)
    # the hull is clipped to the scaled picture: 500 x 375 at s = 4 is 125 x 94; the crop's far edge 500 -> 125, 375 -> ceil(93.75) = 94
    assert was((493, 370, 7, 5), 2, 125, 94) == (123, 92, 2, 2)
    assert was((499, 374, 1, 1), 3, 63, 47) == (62, 46, 1, 1)
    with pytest.raises(ValueError):
        was((0, 0, 0, 5), 1, 10, 10)


def test_windowed_plan_uses_the_crop_for_the_prescale(monkeypatch):
    """_windowed: pick_scale_flags takes the CROP's size against the virtual target; the windows are window_at_scale's; the callers'
    descriptors are untouched; the keyword defaults are None."""
    import inspect
    import pjd_amd
    from pjd_amd import tensors
    for fn in (tensors.decode_resized_batch_tensor, tensors.decode_normalized_batch_tensor):
        p = inspect.signature(fn).parameters
        assert p["crops"].default is None and p["flips"].default is None and p["resize_short"].default is None
    descs = [pjd_amd.ImageDesc() for _ in range(3)]
    for d in descs:
        d.width, d.height = 2000, 1500
    calls = []
    real = tensors.pick_scale_flags
    monkeypatch.setattr(tensors, "pick_scale_flags", lambda w, h, tw, th: calls.append((w, h, tw, th)) or real(w, h, tw, th))
    run, wins = tensors._plan_outputs(descs, (224, 224), True, [(100, 200, 1000, 900), None, (0, 0, 300, 300)], [False, True, True], None)[:2]
    assert calls == [(1000, 900, 224, 224), (2000, 1500, 224, 224), (300, 300, 224, 224)]
    assert [int(d.flags) >> 4 for d in run] == [2, 2, 0] and all(int(d.flags) == 0 for d in descs)
    assert wins[0] == {"x": 25, "y": 50, "w": 250, "h": 225}
    assert wins[1] == {"flags": pjd_amd.RW_HFLIP}
    assert wins[2] == {"x": 0, "y": 0, "w": 300, "h": 300, "flags": pjd_amd.RW_HFLIP}
    # resize_short: the virtual target comes from the full-size picture, the pre-scale is picked against it
    calls.clear()
    run, wins = tensors._plan_outputs(descs[:1], (224, 224), True, None, None, None, 256)[:2]
    assert calls == [(2000, 1500, 341, 256)] and int(run[0].flags) >> 4 == 2
    assert wins == [{"vw": 341, "vh": 256, "ox": 58, "oy": 16}]
    # nothing asked: no windows, the plain pre-scale
    run, wins = tensors._plan_outputs(descs, (224, 224), False, None, None, None)[:2]
    assert wins is None and run is descs
    with pytest.raises(ValueError):
        tensors._plan_outputs(descs, (224, 224), False, [(0, 0, 10, 10)] * 3, None, None, 256)
    with pytest.raises(ValueError):
        tensors._plan_outputs(descs, (224, 224), False, [(1995, 0, 10, 10)] * 3, None, None)
    with pytest.raises(ValueError):
        tensors._plan_outputs(descs, (224, 224), False, None, [True], None)
