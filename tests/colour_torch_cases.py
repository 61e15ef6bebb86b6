"""The case of test_gpu_colour.py that needs torch, run in a process of its own:

    python colour_torch_cases.py colours

As tests/warp_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  The expectation of
every call with colours= is tests/colour_model.py (with tests/normalize_model.py on top) of what the SAME call delivers without it."""
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

import colour_model as M                                          # noqa: E402
import normalize_model as nm                                      # noqa: E402
import pjd_amd                                                    # noqa: E402
from pjd_amd import tensors                                       # noqa: E402

NAMES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61"]
FILL = (114, 7, 201)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy() if t.dtype != torch.uint8 else t.cpu().numpy()


def case_colours():
    datas = [open(os.path.join(HERE, "golden", n + ".jpg"), "rb").read() for n in NAMES]
    scanned = [pjd_amd.Scanned(d) for d in datas]                # kept: a descriptor points into its Scanned
    descs = [s.desc for s in scanned]
    c = pjd_amd.Context(0)
    rng = np.random.default_rng(11)
    jit = [tensors.colour_matrix(brightness=rng.uniform(0.6, 1.4), contrast=rng.uniform(0.6, 1.4), saturation=rng.uniform(0.6, 1.4), hue=rng.uniform(-0.1, 0.1),
                                 grayscale=k == 2, channel_order="bgr" if k == 3 else "rgb") for k in range(7)]
    views = [2, 0, 0, 1, 2, 1, 0]
    colours = [jit[0], None, jit[2], jit[3], M.IDENTITY, jit[5], jit[6]]
    crops = [(3, 2, 40, 50), None, (10, 5, 30, 30), (0, 0, 80, 96), None, (7, 9, 50, 60), (1, 1, 59, 43)]
    flips = [k % 2 == 1 for k in range(7)]
    size = (33, 37)
    kw = dict(prescale=False, views=views, crops=crops, flips=flips)

    # decode_resized_batch_tensor: the model of the uncoloured call; the Batch-level result
    plain, st0 = tensors.decode_resized_batch_tensor(c, descs, size, **kw)
    got, st = tensors.decode_resized_batch_tensor(c, descs, size, colours=colours, **kw)
    assert st == st0 and got.dtype == torch.uint8 and tuple(got.shape) == (7, 3, 33, 37) and got.is_contiguous()
    P = plain.cpu().numpy()
    for v in range(7):
        assert np.array_equal(got[v].cpu().numpy(), M.apply(M.IDENTITY if colours[v] is None else colours[v], P[v])), v
    assert torch.equal(got[1], plain[1]) and torch.equal(got[4], plain[4])
    run, windows, oris, pads = tensors.plan_views(descs, views, size, False, crops, flips)
    with c.batch(run, pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_views(views)
        b.set_resize([size] * 7)
        if oris is not None:
            b.set_orientation(oris)
        b.set_resize_window(windows)
        b.set_colour(colours)
        b.upload(); b.decode()
        outs, _ = b.download()
    for v in range(7):
        assert np.array_equal(got[v].cpu().numpy(), outs[v]), v

    # decode_normalized_batch_tensor: planar fp16, channels_last bf16, a letterbox whose border is not mapped
    for dtype, dt, cl in ((torch.float16, nm.DT_F16, False), (torch.bfloat16, nm.DT_BF16, True), (torch.float32, nm.DT_F32, False)):
        t, st = tensors.decode_normalized_batch_tensor(c, descs, size, nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=dtype, channels_last=cl, colours=colours, **kw)
        assert st == st0 and t.dtype == dtype and tuple(t.shape) == (7, 3, 33, 37)
        scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
        for v in range(7):
            u8 = M.apply(M.IDENTITY if colours[v] is None else colours[v], P[v])
            want = np.stack([nm.table(dt, scale[ch], bias[ch])[u8[ch]] for ch in range(3)])
            assert np.array_equal(bits(t[v]).view(np.uint16 if dt != nm.DT_F32 else np.uint32), nm.bits(want)), (dtype, v)
    lb_plain, _ = tensors.decode_resized_batch_tensor(c, descs, (40, 40), prescale=False, letterbox="center", fill=FILL)
    lb, _ = tensors.decode_resized_batch_tensor(c, descs, (40, 40), prescale=False, letterbox="center", fill=FILL, colours=[jit[3], jit[2], jit[0]])
    for i, m in enumerate((jit[3], jit[2], jit[0])):
        a, p = lb[i].cpu().numpy(), lb_plain[i].cpu().numpy()
        mapped = M.apply(m, p)
        ch, cw, left, top, _, _ = tensors.letterbox_plan(tensors.output_hw(descs[i]), (40, 40))
        inside = np.zeros((40, 40), bool)
        inside[top:top + ch, left:left + cw] = True
        assert np.array_equal(a[:, inside], mapped[:, inside]), i
        assert (a[:, ~inside] == np.asarray(FILL, np.uint8)[:, None]).all() and (~inside).any(), i

    # the keywords that are refused, before anything is created
    for bad in (dict(gray=True, colours=[None] * 3), dict(colours=[None] * 2), dict(views=views, colours=[None] * 3)):
        try:
            tensors.decode_resized_batch_tensor(c, descs, size, **bad)
        except ValueError:
            pass
        else:
            raise AssertionError(f"{bad} was accepted")
    try:
        tensors.decode_normalized_batch_tensor(c, descs, size, 0.5, 0.25, gray=True, colours=[None] * 3)
    except ValueError:
        pass
    else:
        raise AssertionError("gray=True with colours= was accepted")
    c.close()


if __name__ == "__main__":
    case = sys.argv[1]
    {"colours": case_colours}[case]()
    print("CASE OK", case)
