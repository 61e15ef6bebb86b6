"""The case of test_gpu_resize_pad.py that needs torch, run in a process of its own:

    python resize_pad_torch_cases.py letterbox

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected canvases
are tests/resize_pad_model.py over the oracle's picture; the second half holds the result against torch computing "interpolate, then
pad" on the float tensor."""
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
import resize_pad_model as pm                                     # noqa: E402
import pjd_amd                                                    # noqa: E402
import synth                                                      # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from test_gpu_resize import _scanned                              # noqa: E402

N = 8
SIZES = [(61, 45), (45, 61), (80, 52), (33, 70), (96, 40), (40, 96), (64, 64), (57, 83)]      # stored (w, h)
ORIS = [1, 2, 3, 4, 5, 6, 7, 8]
FILL = (114, 114, 113)


def _torch_resize(x_hw3, th, tw, mode):
    x = torch.from_numpy(np.ascontiguousarray(x_hw3).astype(np.float64)).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(x, size=(th, tw), mode=mode, align_corners=False, antialias=(mode == "bicubic"))
    return y.clamp(0, 255)


def case_letterbox():
    port = oracle_lib.Port()
    jpegs = [synth.make(w, h, 40 + i, 90, synth.SUB_444) for i, (w, h) in enumerate(SIZES)]
    scanned = [_scanned(j, 0) for j in jpegs]
    descs = [x.desc for x in scanned]
    rgb = [port.decode(j)["rgb"] for j in jpegs]
    c = pjd_amd.Context(0)
    H, W = 40, 56
    flips = [i % 3 == 1 for i in range(N)]

    def plan(i, mode):
        uh, uw = tensors.orient_hw(ORIS[i], SIZES[i][1], SIZES[i][0])
        ch, cw, l, t, r, b = tensors.letterbox_plan((uh, uw), (H, W), mode)
        return (l, t, r, b)

    # letterbox="center", uint8: orientations and flips act on the content, the rectangle stays where the plan put it
    for kw, filt in ((dict(), "bilinear"), (dict(antialias=True), "antialias"), (dict(interpolation="bicubic"), "bicubic")):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (H, W), prescale=False, flips=flips, orientations=ORIS, letterbox="center", fill=FILL, **kw)
        assert st == [0] * N and tuple(t.shape) == (N, 3, H, W) and t.is_contiguous() and t.dtype == torch.uint8
        host = t.cpu().numpy()
        for i in range(N):
            pad = plan(i, "center")
            o = tensors.orient_then_hflip(ORIS[i]) if flips[i] else ORIS[i]
            want = pm.padded(rgb[i], None, W, H, pad, FILL, o, filt)
            assert any(pad) or SIZES[i] == (64, 64)
            assert np.array_equal(host[i], want.transpose(2, 0, 1)), (i, ORIS[i], filt)
    # letterbox="topleft", pad_value=0, bf16, channels_last: zeros after normalisation
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (H, W), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.bfloat16, channels_last=True,
                                                   prescale=False, orientations=ORIS, letterbox="topleft", fill=FILL, pad_value=0)
    assert st == [0] * N and tuple(t.shape) == (N, 3, H, W) and t.is_contiguous(memory_format=torch.channels_last)
    bits = t.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy()
    for i in range(N):
        pad = plan(i, "topleft")
        assert pad[0] == pad[1] == 0
        u8 = pm.padded(rgb[i], None, W, H, pad, FILL, ORIS[i])
        want = nm.bits(pm.normalized(u8, W, H, pad, nm.DT_BF16, scale, bias, (0.0, 0.0, 0.0)))
        assert np.array_equal(bits[i].view(want.dtype), want), (i, ORIS[i])
        assert (bits[i][pm.border_mask(W, H, pad)] == 0).all()
    # within one level of torch: interpolate the picture to the content size, then pad.  The pictures and the canvas are those of the
    # existing torch cases (tests/orientation_torch_cases.py)
    jpegs = synth.cfg3_imagenet_like(N, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [_scanned(j, 0) for j in jpegs]
    descs = [x.desc for x in scanned]
    rgb = [port.decode(j)["rgb"] for j in jpegs]
    H, W = 96, 160
    for kw, mode in ((dict(), "bilinear"), (dict(interpolation="bicubic"), "bicubic")):
        for lb in ("center", "topleft"):
            t, st = tensors.decode_resized_batch_tensor(c, descs, (H, W), prescale=False, letterbox=lb, fill=FILL, **kw)
            assert st == [0] * N
            host = t.cpu().numpy().astype(np.int64)
            for i, d in enumerate(descs):
                w, h = int(d.width), int(d.height)
                ch, cw, l, tp, r, b = tensors.letterbox_plan((h, w), (H, W), lb)
                ref = _torch_resize(rgb[i], ch, cw, mode)
                planes = [torch.nn.functional.pad(ref[:, k:k + 1], (l, r, tp, b), value=float(FILL[k])) for k in range(3)]
                ref = torch.cat(planes, dim=1)[0].numpy()
                worst = np.abs(host[i] - np.rint(ref)).max()
                print(mode, lb, "picture", i, "worst difference to torch, rounded:", int(worst), flush=True)
                assert worst <= 1, (i, mode, lb, float(np.abs(host[i] - ref).max()))
                m = pm.border_mask(W, H, (l, tp, r, b))
                assert (host[i].transpose(1, 2, 0)[m] == np.asarray(FILL)).all()
    # ... and the normalised tensor: letterbox="topleft", pad_value=0, bf16, channels_last against torch's interpolate, normalise, pad with
    # zeros.  A sample is fma(v, scale, bias) of a level v within one of torch's, rounded once to bfloat16 (8 significant bits): within
    # scale[c] + 2^-8 * |value| of the reference (and 1e-6 for the binary32 arithmetic on either side); the border is exactly zero.
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (H, W), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.bfloat16, channels_last=True,
                                                   prescale=False, letterbox="topleft", fill=FILL, pad_value=0)
    assert st == [0] * N and t.is_contiguous(memory_format=torch.channels_last)
    got = t.float().cpu().numpy().astype(np.float64)
    for i, d in enumerate(descs):
        w, h = int(d.width), int(d.height)
        ch, cw, l, tp, r, b = tensors.letterbox_plan((h, w), (H, W), "topleft")
        ref = np.rint(_torch_resize(rgb[i], ch, cw, "bilinear")[0].numpy())
        ref = ref * scale.astype(np.float64)[:, None, None] + bias.astype(np.float64)[:, None, None]
        ref = torch.nn.functional.pad(torch.from_numpy(ref), (l, r, tp, b), value=0.0).numpy()
        tol = scale.astype(np.float64)[:, None, None] + np.abs(got[i]) / 256.0 + 1e-6
        excess = (np.abs(got[i] - ref) - tol).max()
        print("bf16 topleft picture", i, "largest excess over the tolerance:", float(excess), flush=True)
        assert excess <= 0, (i, float(excess))
        assert (got[i].transpose(1, 2, 0)[pm.border_mask(W, H, (l, tp, r, b))] == 0).all()
    c.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
