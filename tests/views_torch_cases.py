"""The cases of test_gpu_views.py that need torch, each run in a process of its own:

    python views_torch_cases.py <case>

As tests/gray_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so use ONE
HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expectations are the numpy
models of the resize tests over the oracle's pictures (tests/views_cases.py), never something this library delivered."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import os                                                         # noqa: E402
import sys                                                        # noqa: E402

import numpy as np                                                # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))

import gray_expected as G                                         # noqa: E402
import normalize_model as nm                                      # noqa: E402
import oracle_lib                                                 # noqa: E402
import pjd_amd                                                    # noqa: E402
import resize_pad_model as pm                                     # noqa: E402
import views_cases as V                                           # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from test_gpu_scaled import box                                   # noqa: E402

PORT = oracle_lib.Port()
SIZE = (31, 40)                                                   # (H, W): 40 columns, ten lane groups; 31 rows, a ragged fourth row tile
# per view, in the coordinates of the picture as stored: the crop (x, y, w, h) or None, and the flip
CROPS = [(5, 7, 33, 41), (3, 5, 40, 30), None, (1, 2, 30, 60), None, (0, 0, 45, 61), (8, 4, 80, 50), (20, 10, 41, 35)]
FLIPS = [0, 1, 0, 1, 1, 0, 0, 1]


def _descs():
    sc = [pjd_amd.Scanned(V.golden_bytes(n)) for n in V.NAMES]
    assert all(s.valid for s in sc)
    return sc, [s.desc for s in sc]


def _window(v):
    win = {} if CROPS[v] is None else dict(zip("xywh", CROPS[v]))
    if FLIPS[v]:
        win["flags"] = 1
    return win or None


def _u8(v, filt, gray):
    st, rgb, plane = V.oracle(PORT)[V.NAMES[V.VIEWS[v]]]
    src = np.repeat(plane[:, :, None], 3, axis=2) if gray else rgb
    return pm.padded(src, _window(v), SIZE[1], SIZE[0], (0, 0, 0, 0), (0, 0, 0), 1, filt)


def _statuses(st):
    assert st == [V.oracle(PORT)[n][0] for n in V.NAMES] and st[4] != 0, st


def case_resized_views():
    sc, descs = _descs()
    c = pjd_amd.Context(0)
    for gray in (False, True):
        for kw, filt in ((dict(), "bilinear"), (dict(antialias=True), "antialias"), (dict(interpolation="bicubic"), "bicubic")):
            t, st = tensors.decode_resized_batch_tensor(c, descs, SIZE, prescale=False, crops=CROPS, flips=FLIPS, views=V.VIEWS, gray=gray, **kw)
            assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (8, 1 if gray else 3, SIZE[0], SIZE[1]) and t.is_contiguous()
            _statuses(st)
            host = t.cpu().numpy()
            for v in range(8):
                want = _u8(v, filt, gray)
                want = want[..., :1] if gray else want
                assert np.array_equal(host[v], want.transpose(2, 0, 1)), (v, filt, gray)
    # crops, flips and orientations must have one entry per VIEW, and a view must name a picture
    for bad in (dict(crops=CROPS[:5]), dict(flips=FLIPS[:5]), dict(orientations=[1] * 5)):
        try:
            tensors.decode_resized_batch_tensor(c, descs, SIZE, prescale=False, views=V.VIEWS, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    for views in ([0, 5], [-1], []):
        try:
            tensors.decode_resized_batch_tensor(c, descs, SIZE, views=views)
        except ValueError:
            continue
        raise AssertionError(views)
    # without views= nothing changes: [N, 3, H, W], one entry per picture
    t, st = tensors.decode_resized_batch_tensor(c, descs, SIZE, prescale=False)
    assert tuple(t.shape) == (5, 3, SIZE[0], SIZE[1]) and len(st) == 5
    c.close()


def case_normalized_views():
    sc, descs = _descs()
    c = pjd_amd.Context(0)
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    # channels_last, binary16, bicubic, crops and flips
    t, st = tensors.decode_normalized_batch_tensor(c, descs, SIZE, nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.float16, channels_last=True, prescale=False,
                                                   crops=CROPS, flips=FLIPS, interpolation="bicubic", views=V.VIEWS)
    assert tuple(t.shape) == (8, 3, SIZE[0], SIZE[1]) and t.dtype == torch.float16 and t.is_contiguous(memory_format=torch.channels_last)
    _statuses(st)
    host = t.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    for v in range(8):
        want = nm.normalize(_u8(v, "bicubic", False), nm.DT_F16, scale, bias)
        assert np.array_equal(nm.bits(host[v]), nm.bits(want)), v
    # grey, binary32, letterboxed with a pad value, orientations per view: [V, 1, H, W]
    oris = [1, 6, 3, 8, 2, 5, 4, 7]
    t, st = tensors.decode_normalized_batch_tensor(c, descs, SIZE, 0.449, 0.226, dtype=torch.float32, prescale=False, orientations=oris, letterbox="center",
                                                   fill=77, pad_value=-1.5, antialias=True, views=V.VIEWS, gray=True)
    assert tuple(t.shape) == (8, 1, SIZE[0], SIZE[1]) and t.dtype == torch.float32 and t.is_contiguous()
    _statuses(st)
    host = t.cpu().numpy()
    gs, gb = tensors.normalize_constants([0.449] * 3, [0.226] * 3)
    for v in range(8):
        plane = V.oracle(PORT)[V.NAMES[V.VIEWS[v]]][2]
        uh, uw = tensors.orient_hw(oris[v], *plane.shape)
        ch, cw, left, top, right, bottom = tensors.letterbox_plan((uh, uw), SIZE, "center")
        pad = (left, top, right, bottom)
        C = pm.padded(np.repeat(plane[:, :, None], 3, axis=2), None, SIZE[1], SIZE[0], pad, (77, 77, 77), oris[v], "antialias")
        want = pm.normalized(C, SIZE[1], SIZE[0], pad, nm.DT_F32, gs, gb, (-1.5, -1.5, -1.5))[..., 0]
        assert np.array_equal(nm.bits(host[v, 0]), nm.bits(want)), v
    c.close()


def case_two_crops_prescaled():
    """prescale=True with views: a picture is decoded at the LEAST reduced of the scales its views would pick, and every view's crop is
    taken at that scale."""
    sc, descs = _descs()
    c = pjd_amd.Context(0)
    size = (12, 10)
    views = [1, 4, 1, 1, 4]
    crops = [None, None, (0, 0, 40, 48), (16, 8, 20, 24), (32, 0, 64, 64)]
    # picture 1 (80 x 96): whole -> 1/8, 40 x 48 -> 1/4, 20 x 24 -> 1/2: decoded at 1/2.  picture 4 (96 x 64): whole -> 1/4 (24 x 16; 1/8 is
    # 12 x 8, too low), 64 x 64 -> 1/4: decoded at 1/4.  The pictures without a view are decoded at 1/8: nothing reads them.
    run, windows, oris, pads = tensors.plan_views(descs, views, size, True, crops, None, None, None, None)
    assert [int(d.flags) & pjd_amd.F_SCALE_MASK for d in run] == [pjd_amd.F_SCALE_1_8, pjd_amd.F_SCALE_1_2, pjd_amd.F_SCALE_1_8, pjd_amd.F_SCALE_1_8, pjd_amd.F_SCALE_1_4]
    assert windows == [None, None, dict(x=0, y=0, w=20, h=24), dict(x=8, y=4, w=10, h=12), dict(x=8, y=0, w=16, h=16)] and oris is None and pads is None
    t, st = tensors.decode_resized_batch_tensor(c, descs, size, prescale=True, crops=crops, views=views)
    assert tuple(t.shape) == (5, 3, 12, 10)
    _statuses(st)
    host = t.cpu().numpy()
    for v, p in enumerate(views):
        src = box(V.oracle(PORT)[V.NAMES[p]][1], 2 if p == 1 else 4)
        want = pm.padded(src, windows[v], size[1], size[0], (0, 0, 0, 0), (0, 0, 0), 1, "bilinear")
        assert np.array_equal(host[v], want.transpose(2, 0, 1)), v
    c.close()


if __name__ == "__main__":
    case = sys.argv[1]
    {"resized_views": case_resized_views, "normalized_views": case_normalized_views, "two_crops_prescaled": case_two_crops_prescaled}[case]()
    print("CASE OK", case)
