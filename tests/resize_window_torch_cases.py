"""The cases of test_gpu_resize_window.py that need torch, each run in a process of its own:

    python resize_window_torch_cases.py <case>

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected pictures
are tests/resize_window_model.py over the box filter of the oracle's picture."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import ctypes as C                                                # noqa: E402
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
import pjd_amd                                                    # noqa: E402
import resize_window_model as wm                                  # noqa: E402
from resize_probe import random_resized_crop                      # noqa: E402  (tools/: torchvision's RandomResizedCrop.get_params)
import synth                                                      # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from test_gpu_resize import _scanned                              # noqa: E402
from test_gpu_scaled import box                                   # noqa: E402

N = 32


def _batch():
    """32 ImageNet-like pictures of different sizes, their descriptors and the oracle's pictures."""
    port = oracle_lib.Port()
    jpegs = synth.cfg3_imagenet_like(N, seed=5, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [_scanned(j, 0) for j in jpegs]
    descs = [x.desc for x in scanned]
    assert len({(int(d.width), int(d.height)) for d in descs}) > 1, "the batch is ragged"
    rgb = [port.decode(j)["rgb"] for j in jpegs]
    return scanned, descs, rgb


def case_crops_and_flips():
    scanned, descs, rgb = _batch()
    rng = np.random.default_rng(11)
    crops = [random_resized_crop(rng, int(d.width), int(d.height)) for d in descs]
    crops[3] = None                                               # the whole picture
    flips = [bool(rng.integers(0, 2)) for _ in descs]
    assert any(flips) and not all(flips)
    c = pjd_amd.Context(0)
    before = [bytes(C.string_at(C.byref(d), C.sizeof(pjd_amd.ImageDesc))) for d in descs]
    wins = [dict(({} if cr is None else dict(zip("xywh", cr))), **({"flags": wm.HFLIP} if f else {})) for cr, f in zip(crops, flips)]
    for antialias in (False, True):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (64, 64), prescale=False, antialias=antialias, crops=crops, flips=flips)
        assert [bytes(C.string_at(C.byref(d), C.sizeof(pjd_amd.ImageDesc))) for d in descs] == before
        assert st == [0] * N
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (N, 3, 64, 64) and t.is_contiguous()
        host = t.cpu().numpy()
        for i in range(N):
            assert np.array_equal(host[i], wm.window(rgb[i], wins[i], 64, 64, antialias).transpose(2, 0, 1)), (i, antialias, wins[i])
    # the window did something: picture 0 differs from the un-windowed call
    plain, _ = tensors.decode_resized_batch_tensor(c, descs[:1], (64, 64), prescale=False)
    assert not np.array_equal(plain.cpu().numpy()[0], wm.window(rgb[0], wins[0], 64, 64).transpose(2, 0, 1))
    # with the pre-scale: chosen from the crop's size, and the crop becomes window_at_scale's hull over the box picture
    t, st = tensors.decode_resized_batch_tensor(c, descs, (64, 64), crops=crops, flips=flips)
    assert st == [0] * N
    host = t.cpu().numpy()
    logs = []
    for i, d in enumerate(descs):
        cw, ch = (crops[i][2], crops[i][3]) if crops[i] is not None else (int(d.width), int(d.height))
        log = tensors.pick_scale_flags(cw, ch, 64, 64) >> 4
        src = box(rgb[i], 1 << log)
        win = {"flags": wm.HFLIP} if flips[i] else {}
        if crops[i] is not None:
            win.update(zip("xywh", tensors.window_at_scale(crops[i], log, src.shape[1], src.shape[0])))
        assert np.array_equal(host[i], wm.window(src, win, 64, 64).transpose(2, 0, 1)), (i, log, win)
        logs.append(log)
    assert len(set(logs)) > 1, "more than one pre-scale is met"
    c.close()


def case_resize_short_normalized():
    scanned, descs, rgb = _batch()
    c = pjd_amd.Context(0)
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    flips = [i % 3 == 0 for i in range(N)]
    for prescale, antialias in ((True, False), (False, True)):
        t, st = tensors.decode_normalized_batch_tensor(c, descs, (64, 64), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.bfloat16, channels_last=True,
                                                       prescale=prescale, antialias=antialias, resize_short=73, flips=flips)
        assert st == [0] * N
        assert t.dtype == torch.bfloat16 and t.is_cuda and tuple(t.shape) == (N, 3, 64, 64)
        assert t.is_contiguous(memory_format=torch.channels_last) and t.stride() == (3 * 64 * 64, 1, 3 * 64, 3)
        bits = t.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy()
        for i, d in enumerate(descs):
            win = tensors.center_crop_window((int(d.height), int(d.width)), 73, (64, 64))
            assert min(win["vw"], win["vh"]) == 73 and (win["ox"], win["oy"]) != (0, 0)
            log = tensors.pick_scale_flags(d.width, d.height, win["vw"], win["vh"]) >> 4 if prescale else 0
            if flips[i]:
                win["flags"] = wm.HFLIP
            u8 = wm.window(box(rgb[i], 1 << log), win, 64, 64, antialias)
            want = nm.bits(nm.normalize(u8, nm.DT_BF16, scale, bias))
            assert np.array_equal(bits[i].view(want.dtype), want), (i, prescale, antialias, win)
    # a resized picture smaller than the crop is refused before anything is created
    try:
        tensors.decode_resized_batch_tensor(c, descs, (64, 64), resize_short=63)
        raise AssertionError("resize_short=63 with a 64 x 64 crop must raise")
    except ValueError:
        pass
    c.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
