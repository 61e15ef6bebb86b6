"""The cases of test_gpu_orientation.py that need torch, each run in a process of its own:

    python orientation_torch_cases.py <case>

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected pictures
are tests/orientation_model.py over the oracle's picture; the second case holds the result against torch computing "orient, crop,
interpolate" on the float tensor."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import normalize_model as nm                                      # noqa: E402
import oracle_lib                                                 # noqa: E402
import orientation_model as om                                    # noqa: E402
import pjd_amd                                                    # noqa: E402
import synth                                                      # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from test_gpu_resize import _scanned                              # noqa: E402

N = 8
SIZES = [(61, 45), (45, 61), (80, 52), (33, 70), (96, 40), (40, 96), (64, 64), (57, 83)]      # stored (w, h)
ORIS = [1, 2, 3, 4, 5, 6, 7, 8]


def _batch():
    """Eight small pictures without symmetry, one per orientation: descriptors and the oracle's pictures."""
    port = oracle_lib.Port()
    jpegs = [synth.make(w, h, 40 + i, 90, synth.SUB_444) for i, (w, h) in enumerate(SIZES)]
    scanned = [_scanned(j, 0) for j in jpegs]
    return scanned, [x.desc for x in scanned], [port.decode(j)["rgb"] for j in jpegs]


def case_orientations_against_the_model():
    scanned, descs, rgb = _batch()
    c = pjd_amd.Context(0)
    # decode_to_tensors: every picture upright at its own size, the exact permutation
    for planar in (True, False):
        outs, st = tensors.decode_to_tensors(c, descs, planar=planar, orientations=ORIS)
        assert st == [0] * N
        for i, (t, o) in enumerate(zip(outs, ORIS)):
            want = om.orient(rgb[i], o)
            assert t.is_cuda and t.dtype == torch.uint8
            got = t.cpu().numpy()
            assert np.array_equal(got, want.transpose(2, 0, 1) if planar else want), (i, o, planar)
    plain, _ = tensors.decode_to_tensors(c, descs, orientations=None)
    assert all(np.array_equal(t.cpu().numpy(), p.transpose(2, 0, 1)) for t, p in zip(plain, rgb))
    # decode_resized_batch_tensor: crops of the UPRIGHT picture, flips folded into the orientation
    crops, flips = [], []
    for i, ((w, h), o) in enumerate(zip(SIZES, ORIS)):
        uh, uw = tensors.orient_hw(o, h, w)
        crops.append(None if i == 2 else (3 + i, 2, uw - 9 - i, uh - 7))
        flips.append(i % 3 == 1)
    for kw, filt in ((dict(), "bilinear"), (dict(antialias=True), "antialias"), (dict(interpolation="bicubic"), "bicubic")):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (24, 40), prescale=False, crops=crops, flips=flips, orientations=ORIS, **kw)
        assert st == [0] * N and tuple(t.shape) == (N, 3, 24, 40) and t.is_contiguous()
        host = t.cpu().numpy()
        for i, ((w, h), o) in enumerate(zip(SIZES, ORIS)):
            win = None if crops[i] is None else dict(zip("xywh", tensors.crop_to_stored(o, crops[i], w, h)))
            want = om.oriented(rgb[i], win, 40, 24, o, filt)
            want = want[:, ::-1] if flips[i] else want
            assert np.array_equal(host[i], want.transpose(2, 0, 1)), (i, o, filt)
    # decode_normalized_batch_tensor: Resize(short) + CenterCrop of the upright picture, channels_last bf16
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (20, 28), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.bfloat16, channels_last=True,
                                                   prescale=False, resize_short=30, orientations=ORIS)
    assert st == [0] * N and tuple(t.shape) == (N, 3, 20, 28) and t.is_contiguous(memory_format=torch.channels_last)
    bits = t.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy()
    for i, ((w, h), o) in enumerate(zip(SIZES, ORIS)):
        uh, uw = tensors.orient_hw(o, h, w)
        cc = tensors.center_crop_window((uh, uw), 30, (20, 28))
        tr = o >= 5
        svw, svh = (cc["vh"], cc["vw"]) if tr else (cc["vw"], cc["vh"])
        ox, oy, _, _ = tensors.crop_to_stored(o, (cc["ox"], cc["oy"], 28, 20), svw, svh)
        u8 = om.oriented(rgb[i], dict(vw=svw, vh=svh, ox=ox, oy=oy), 28, 20, o)
        want = nm.bits(nm.normalize(u8, nm.DT_BF16, scale, bias))
        assert np.array_equal(bits[i].view(want.dtype), want), (i, o)
    c.close()


def _torch_resize(x_hw3, th, tw, mode):
    x = torch.from_numpy(np.ascontiguousarray(x_hw3).astype(np.float64)).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=(th, tw), mode=mode, align_corners=False, antialias=(mode == "bicubic"))
    return y[0].clamp(0, 255).numpy()


def case_within_one_level_of_orient_crop_interpolate():
    """torch on the float tensor: orient the picture, crop it, interpolate -- the order a loader without this feature works in.  The
    library resamples in the stored picture's coordinates and permutes, which differs only in tie-breaking: within one level.  The
    pictures and the target are those of the existing torch cases (tests/resize_bicubic_torch_cases.py)."""
    port = oracle_lib.Port()
    jpegs = synth.cfg3_imagenet_like(N, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [_scanned(j, 0) for j in jpegs]
    descs = [x.desc for x in scanned]
    rgb = [port.decode(j)["rgb"] for j in jpegs]
    c = pjd_amd.Context(0)
    crops = []
    for d, o in zip(descs, ORIS):
        uh, uw = tensors.orient_hw(o, int(d.height), int(d.width))
        crops.append((uw // 9, uh // 7, uw - uw // 4, uh - uh // 5))
    for kw, mode in ((dict(), "bilinear"), (dict(interpolation="bicubic"), "bicubic")):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (96, 160), prescale=False, crops=crops, orientations=ORIS, **kw)
        assert st == [0] * N
        host = t.cpu().numpy().astype(np.int64)
        for i, o in enumerate(ORIS):
            x, y, w, h = crops[i]
            up = om.orient(rgb[i], o)[y:y + h, x:x + w]
            ref = _torch_resize(up, 96, 160, mode).transpose(0, 1, 2)
            worst = np.abs(host[i] - np.rint(ref)).max()
            print(mode, "picture", i, "orientation", o, "worst difference to torch, rounded:", int(worst), flush=True)
            assert worst <= 1, (i, o, mode, float(np.abs(host[i] - ref).max()))
    c.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
