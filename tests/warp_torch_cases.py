"""The case of test_gpu_warp.py that needs torch, run in a process of its own:

    python warp_torch_cases.py affines

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  The source P of
every expectation is what decode_to_tensors delivers un-resampled; the expectations are tests/warp_model.py of it."""
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

import normalize_model as nm                                      # noqa: E402
import warp_model as M                                            # noqa: E402
import pjd_amd                                                    # noqa: E402
from pjd_amd import tensors                                       # noqa: E402

NAMES = ["env_61x45_420_q100_opt", "noise_80x96_422_q50_opt", "h1v2_45x61", "gray_33x70"]
FILL = (114, 7, 201)


def case_affines():
    datas = [open(os.path.join(HERE, "golden", n + ".jpg"), "rb").read() for n in NAMES]
    scanned = [pjd_amd.Scanned(d) for d in datas]
    descs = [s.desc for s in scanned]
    n = len(descs)
    c = pjd_amd.Context(0)
    plain, st0 = tensors.decode_to_tensors(c, descs)
    P = [t.cpu().numpy() for t in plain]                         # [3, h, w]
    plain_g, _ = tensors.decode_to_tensors(c, descs, gray=True)
    PG = [t.cpu().numpy() for t in plain_g]                      # [1, h, w]
    hw = [p.shape[1:] for p in P]

    # angle=90 onto the transposed size is numpy.rot90(P, 1); angle=0, scale=1 onto the picture's own size is P.  One size a batch, so a
    # picture a call
    for i in range(n):
        h, w = hw[i]
        t, st = tensors.decode_resized_batch_tensor(c, [descs[i]], (w, h), prescale=False, affines=[tensors.affine_inverse_matrix((h, w), (w, h), angle=90)], fill=FILL)
        assert st == [st0[i]] and tuple(t.shape) == (1, 3, w, h) and t.dtype == torch.uint8 and t.is_contiguous()
        assert np.array_equal(t[0].cpu().numpy(), np.rot90(P[i], 1, (1, 2))), NAMES[i]
        t, st = tensors.decode_resized_batch_tensor(c, [descs[i]], (h, w), prescale=False, affines=[tensors.affine_inverse_matrix((h, w), (h, w), angle=0, scale=1)], fill=FILL)
        assert np.array_equal(t[0].cpu().numpy(), P[i]), NAMES[i]
        # an orientation of 6 with the identity map of the UPRIGHT picture is orientations= alone
        uh, uw = tensors.orient_hw(6, h, w)
        a, _ = tensors.decode_resized_batch_tensor(c, [descs[i]], (uh, uw), prescale=False, orientations=[6], affines=[(1, 0, 0, 0, 1, 0)], fill=FILL)
        b, _ = tensors.decode_resized_batch_tensor(c, [descs[i]], (uh, uw), prescale=False, orientations=[6])
        assert torch.equal(a, b) and tuple(a.shape) == (1, 3, uh, uw), NAMES[i]
        assert np.array_equal(a[0].cpu().numpy(), np.rot90(P[i], -1, (1, 2))), "orientation 6 turns the stored picture clockwise"

    # one batch, one matrix a picture: RandomAffine-like maps against the model; then the same with views, channels_last and gray
    H, W = 48, 72
    rng = np.random.default_rng(12)
    mats = [tensors.affine_inverse_matrix(hw[i], (H, W), angle=float(rng.uniform(-180, 180)), translate=(float(rng.uniform(-9, 9)), float(rng.uniform(-9, 9))),
                                          scale=float(rng.uniform(0.5, 1.6)), shear=(float(rng.uniform(-20, 20)), float(rng.uniform(-10, 10)))) for i in range(n)]
    t, st = tensors.decode_resized_batch_tensor(c, descs, (H, W), prescale=False, affines=mats, fill=FILL)
    assert st == st0 and tuple(t.shape) == (n, 3, H, W)
    host = t.cpu().numpy()
    for i in range(n):
        assert np.array_equal(host[i], M.warp(P[i], mats[i], W, H, FILL)), NAMES[i]
    views = [1, 1, 0, 3, 1]
    vm = [mats[1], tensors.affine_inverse_matrix(hw[1], (H, W), angle=45), mats[0], mats[3], tensors.affine_inverse_matrix(hw[1], (H, W), translate=(30, -20))]
    t, st = tensors.decode_resized_batch_tensor(c, descs, (H, W), prescale=False, affines=vm, fill=FILL, views=views)
    assert st == st0 and tuple(t.shape) == (5, 3, H, W)
    host = t.cpu().numpy()
    for v, p in enumerate(views):
        assert np.array_equal(host[v], M.warp(P[p], vm[v], W, H, FILL)), v
    # gray=True: one plane, the fill one byte
    t, st = tensors.decode_resized_batch_tensor(c, descs, (H, W), prescale=False, affines=mats, fill=77, gray=True)
    assert tuple(t.shape) == (n, 1, H, W)
    host = t.cpu().numpy()
    for i in range(n):
        assert np.array_equal(host[i], M.warp(PG[i], mats[i], W, H, (77, 77, 77))), NAMES[i]
    # normalised, channels_last, bf16: the table of tests/normalize_model.py over the model's bytes
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (H, W), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.bfloat16, channels_last=True, prescale=False,
                                                   affines=mats, fill=FILL)
    assert st == st0 and tuple(t.shape) == (n, 3, H, W) and t.is_contiguous(memory_format=torch.channels_last)
    bits = t.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    for i in range(n):
        u8 = M.warp(P[i], mats[i], W, H, FILL)
        want = np.stack([nm.table(nm.DT_BF16, scale[ch], bias[ch])[u8[ch]] for ch in range(3)], axis=-1)
        assert np.array_equal(bits[i], nm.bits(want)), NAMES[i]
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (H, W), 0.5, 0.25, dtype=torch.float32, prescale=False, affines=mats, fill=9, gray=True)
    sg, bg = tensors.normalize_constants([0.5] * 3, [0.25] * 3)
    host = t.cpu().numpy()
    for i in range(n):
        want = nm.table(nm.DT_F32, sg[0], bg[0])[M.warp(PG[i], mats[i], W, H, (9, 9, 9))]
        assert np.array_equal(nm.bits(host[i]), nm.bits(want)), NAMES[i]

    # prescale=True: a map that shrinks 4.5x on both axes is decoded at 1/4 and its matrix divided by 4 (the model over the library's own
    # 1/4 picture); one that shrinks an axis by less than 2 leaves its picture at full size
    shrink = [tensors.affine_inverse_matrix(hw[i], (12, 16), scale=1 / 4.5) for i in range(n)]
    run, pm = tensors.plan_affines(descs, shrink, True)
    assert all(int(d.flags) & pjd_amd.F_SCALE_MASK == pjd_amd.F_SCALE_1_4 for d in run) and all(abs(m[0] - 4.5 / 4) < 1e-12 for m in pm)
    quarter, _ = tensors.decode_to_tensors(c, run)
    t, st = tensors.decode_resized_batch_tensor(c, descs, (12, 16), affines=shrink, fill=FILL)
    for i in range(n):
        assert np.array_equal(t[i].cpu().numpy(), M.warp(quarter[i].cpu().numpy(), pm[i], 16, 12, FILL)), NAMES[i]
    aniso = [(4.0, 0, 0, 0, 1.5, 0)] * n
    run, pm = tensors.plan_affines(descs, aniso, True)
    assert all(int(d.flags) & pjd_amd.F_SCALE_MASK == 0 for d in run) and pm[0] == aniso[0]
    run, pm = tensors.plan_affines(descs, [aniso[0], shrink[1], shrink[1]], True, views=[1, 1, 1])
    assert int(run[1].flags) & pjd_amd.F_SCALE_MASK == 0, "the least reduced of a picture's views decides"

    # what affines= excludes
    for kw in (dict(crops=[None] * n), dict(flips=[False] * n), dict(resize_short=64), dict(letterbox="center"), dict(antialias=True), dict(interpolation="bicubic")):
        try:
            tensors.decode_resized_batch_tensor(c, descs, (H, W), affines=mats, **kw)
        except ValueError as e:
            assert "affines" in str(e), e
        else:
            raise AssertionError(f"affines= with {kw} was accepted")
    for bad in ([mats[0]] * (n - 1), [mats[0]] * (n - 1) + [(1, 2, 3)], [mats[0]] * (n - 1) + [(float("nan"), 0, 0, 0, 1, 0)]):
        try:
            tensors.decode_resized_batch_tensor(c, descs, (H, W), affines=bad)
        except ValueError:
            pass
        else:
            raise AssertionError("a bad affines= was accepted")
    c.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
