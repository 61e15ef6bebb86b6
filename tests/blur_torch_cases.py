"""The case of test_gpu_blur.py that needs torch, run in a process of its own:

    python blur_torch_cases.py blurs

As tests/colour_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  The expectation of
every call with blurs= is tests/blur_model.py (with tests/normalize_model.py on top) of what the SAME call delivers without it; and,
where torch's reflect padding applies (r < min(H, W)), torch.nn.functional.conv2d over the padded float64 tensor, to within 1 level."""
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

import blur_model as M                                            # noqa: E402
import normalize_model as nm                                      # noqa: E402
import pjd_amd                                                    # noqa: E402
from pjd_amd import tensors                                       # noqa: E402

NAMES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61"]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy() if t.dtype != torch.uint8 else t.cpu().numpy()


def torch_blur(u8, ksize, sigma):
    """torchvision's gaussian_blur, written out in float64 on the CPU: reflect pad, then one depthwise conv2d per axis"""
    x = torch.from_numpy(u8.astype(np.float64))[None]             # [1, C, H, W]
    r = ksize // 2
    k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=torch.float64) / sigma) ** 2)
    k = k / k.sum()
    ch = x.shape[1]
    x = torch.nn.functional.pad(x, (r, r, r, r), mode="reflect")
    x = torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1).expand(ch, 1, 1, -1), groups=ch)
    x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1).expand(ch, 1, -1, 1), groups=ch)
    return x[0].numpy()


def case_blurs():
    datas = [open(os.path.join(HERE, "golden", n + ".jpg"), "rb").read() for n in NAMES]
    scanned = [pjd_amd.Scanned(d) for d in datas]                # kept: a descriptor points into its Scanned
    descs = [s.desc for s in scanned]
    c = pjd_amd.Context(0)
    views = [2, 0, 0, 1, 2, 1, 0]
    blurs = [(23, 2.0), None, (3, 0.8), (63, 10.0), (5, 100.0), (3, 0.1), (23, 0.5)]
    crops = [(3, 2, 40, 50), None, (10, 5, 30, 30), (0, 0, 80, 96), None, (7, 9, 50, 60), (1, 1, 59, 43)]
    flips = [k % 2 == 1 for k in range(7)]
    size = (33, 37)
    kw = dict(prescale=False, views=views, crops=crops, flips=flips)

    # decode_resized_batch_tensor: the model of the unblurred call; torch's own filter; the Batch-level result
    plain, st0 = tensors.decode_resized_batch_tensor(c, descs, size, **kw)
    got, st = tensors.decode_resized_batch_tensor(c, descs, size, blurs=blurs, **kw)
    assert st == st0 and got.dtype == torch.uint8 and tuple(got.shape) == (7, 3, 33, 37) and got.is_contiguous()
    P = plain.cpu().numpy()
    worst = 0.0
    for v in range(7):
        a = got[v].cpu().numpy()
        assert np.array_equal(a, M.blur(P[v], blurs[v])), v
        if blurs[v] is not None and blurs[v][0] // 2 < min(size):
            d = float(np.abs(a.astype(np.float64) - torch_blur(P[v], *blurs[v])).max())
            worst = max(worst, d)
            assert d <= 1.0, (v, blurs[v], d)
    print("worst difference from conv2d on the reflect-padded float64 tensor:", worst)
    assert torch.equal(got[1], plain[1]) and torch.equal(got[5], plain[5]) and not torch.equal(got[0], plain[0])
    run, windows, oris, pads = tensors.plan_views(descs, views, size, False, crops, flips)
    with c.batch(run, pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_views(views)
        b.set_resize([size] * 7)
        if oris is not None:
            b.set_orientation(oris)
        b.set_resize_window(windows)
        b.set_blur(blurs)
        b.upload(); b.decode()
        outs, _ = b.download()
    for v in range(7):
        assert np.array_equal(got[v].cpu().numpy(), outs[v]), v

    # decode_normalized_batch_tensor: planar fp16, channels_last bf16, planar fp32
    for dtype, dt, cl in ((torch.float16, nm.DT_F16, False), (torch.bfloat16, nm.DT_BF16, True), (torch.float32, nm.DT_F32, False)):
        t, st = tensors.decode_normalized_batch_tensor(c, descs, size, nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=dtype, channels_last=cl, blurs=blurs, **kw)
        assert st == st0 and t.dtype == dtype and tuple(t.shape) == (7, 3, 33, 37)
        assert t.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
        for v in range(7):
            u8 = M.blur(P[v], blurs[v])
            want = np.stack([nm.table(dt, scale[ch], bias[ch])[u8[ch]] for ch in range(3)])
            assert np.array_equal(bits(t[v]).view(np.uint16 if dt != nm.DT_F32 else np.uint32), nm.bits(want)), (dtype, v)
    # a grey batch: one plane
    gp, _ = tensors.decode_resized_batch_tensor(c, descs, size, gray=True, **kw)
    gb, _ = tensors.decode_resized_batch_tensor(c, descs, size, gray=True, blurs=blurs, **kw)
    for v in range(7):
        assert np.array_equal(gb[v].cpu().numpy(), M.blur(gp[v].cpu().numpy(), blurs[v])), v

    # the keywords that are refused, before anything is created
    for bad in (dict(blurs=[None] * 2), dict(views=views, blurs=[None] * 3), dict(letterbox="center", blurs=[None] * 3)):
        try:
            tensors.decode_resized_batch_tensor(c, descs, size, **bad)
        except ValueError:
            pass
        else:
            raise AssertionError(f"{bad} was accepted")
    try:
        tensors.decode_normalized_batch_tensor(c, descs, size, nm.IMAGENET_MEAN, nm.IMAGENET_STD, letterbox="topleft", blurs=[(3, 1.0)] * 3)
    except ValueError:
        pass
    else:
        raise AssertionError("letterbox= with blurs= was accepted")
    c.close()


if __name__ == "__main__":
    case = sys.argv[1]
    {"blurs": case_blurs}[case]()
    print("CASE OK", case)
