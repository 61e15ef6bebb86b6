"""The cases of test_gpu_resize_bicubic.py that need torch, each run in a process of its own:

    python resize_bicubic_torch_cases.py <case>

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected pictures
are tests/resize_bicubic_model.py over the box filter of the oracle's picture; torch's own bicubic filter (antialias=True, on the
float64 picture, on the CPU) is held against them to within 1 level."""
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
import resize_bicubic_model as bc                                 # noqa: E402
import synth                                                      # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from test_gpu_resize import _scanned                              # noqa: E402
from test_gpu_scaled import box                                   # noqa: E402

N = 16


def _batch():
    """16 ImageNet-like pictures of different sizes, their descriptors and the oracle's pictures."""
    port = oracle_lib.Port()
    jpegs = synth.cfg3_imagenet_like(N, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [_scanned(j, 0) for j in jpegs]
    descs = [x.desc for x in scanned]
    assert len({(int(d.width), int(d.height)) for d in descs}) > 1, "the batch is ragged"
    rgb = [port.decode(j)["rgb"] for j in jpegs]
    return scanned, descs, rgb


def _torch_bicubic(rgb, th, tw):
    """torch's bicubic filter with antialias=True over the float64 picture, clamped once: th x tw x 3 float64."""
    x = torch.from_numpy(rgb.astype(np.float64)).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=(th, tw), mode="bicubic", align_corners=False, antialias=True)
    return y[0].permute(1, 2, 0).clamp(0, 255).numpy()


def case_resized_batch_tensor():
    scanned, descs, rgb = _batch()
    c = pjd_amd.Context(0)
    before = [bytes(C.string_at(C.byref(d), C.sizeof(pjd_amd.ImageDesc))) for d in descs]
    t, st = tensors.decode_resized_batch_tensor(c, descs, (224, 224), interpolation="bicubic")
    assert [bytes(C.string_at(C.byref(d), C.sizeof(pjd_amd.ImageDesc))) for d in descs] == before
    assert st == [0] * N
    assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (N, 3, 224, 224) and t.is_contiguous()
    host = t.cpu().numpy()
    flags = [tensors.pick_scale_flags(d.width, d.height, 224, 224) for d in descs]
    assert len(set(flags)) > 1
    for i in range(N):
        want = bc.resize(box(rgb[i], 1 << (flags[i] >> 4)), 224, 224).transpose(2, 0, 1)
        assert np.array_equal(host[i], want), i
    # without the pre-scale: the bicubic resize of the full-size picture, a non-square target; antialias is not consulted
    for aa in (False, True):
        t2, st2 = tensors.decode_resized_batch_tensor(c, descs, (96, 160), prescale=False, antialias=aa, interpolation="bicubic")
        assert st2 == [0] * N and tuple(t2.shape) == (N, 3, 96, 160)
        host2 = t2.cpu().numpy()
        for i in range(N):
            assert np.array_equal(host2[i], bc.resize(rgb[i], 160, 96).transpose(2, 0, 1)), (i, aa)
    for i in range(N):
        ref = _torch_bicubic(rgb[i], 96, 160).transpose(2, 0, 1)
        assert np.abs(host2[i].astype(np.int64) - np.rint(ref)).max() <= 1, i
    # the default is the bilinear filter, the antialiased one is the triangle: both differ
    t3, _ = tensors.decode_resized_batch_tensor(c, descs[:4], (96, 160), prescale=False)
    t4, _ = tensors.decode_resized_batch_tensor(c, descs[:4], (96, 160), prescale=False, antialias=True)
    assert not np.array_equal(t3.cpu().numpy(), host2[:4]) and not np.array_equal(t4.cpu().numpy(), host2[:4])
    c.close()


def case_normalized_channels_last():
    scanned, descs, rgb = _batch()
    c = pjd_amd.Context(0)
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    flags = [tensors.pick_scale_flags(d.width, d.height, 224, 224) for d in descs]
    u8 = [bc.resize(box(rgb[i], 1 << (flags[i] >> 4)), 224, 224) for i in range(N)]
    for dtype, dt in ((torch.float16, nm.DT_F16), (torch.bfloat16, nm.DT_BF16), (torch.float32, nm.DT_F32)):
        t, st = tensors.decode_normalized_batch_tensor(c, descs, (224, 224), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=dtype, channels_last=True,
                                                       interpolation="bicubic")
        assert st == [0] * N
        assert t.dtype == dtype and t.is_cuda and tuple(t.shape) == (N, 3, 224, 224)
        assert t.is_contiguous(memory_format=torch.channels_last) and t.stride() == (3 * 224 * 224, 1, 3 * 224, 3)
        bits = t.permute(0, 2, 3, 1).contiguous().view(torch.int16 if dt != nm.DT_F32 else torch.int32).cpu().numpy()
        for i in range(N):
            want = nm.bits(nm.normalize(u8[i], dt, scale, bias))
            assert np.array_equal(bits[i].view(want.dtype), want), (i, dt)
    # one launch, full-size pictures, NCHW float32: torch's bicubic filter on the float picture reproduces it to within 1 level
    # before the normalisation
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (224, 224), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.float32, prescale=False,
                                                   interpolation="bicubic")
    assert st == [0] * N and t.is_contiguous()
    host = t.cpu().numpy().astype(np.float64)
    for i in range(N):
        level = (host[i] - bias.astype(np.float64)[:, None, None]) / scale.astype(np.float64)[:, None, None]
        ref = _torch_bicubic(rgb[i], 224, 224).transpose(2, 0, 1)
        assert np.abs(level - np.rint(level)).max() < 1e-3 and np.abs(level - ref).max() <= 1.0 + 1e-3, i
    c.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
