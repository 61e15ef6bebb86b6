"""What the colour map on decode costs: the default bench workload (1024 ragged pictures, box pre-scale), two 224 x 224
RandomResizedCrop views per picture (seeded crops and flips), planar, bound into a torch buffer, as uint8 and as normalised bf16, with
(a) the batch without set_colour in its plain form (the windowed kernels) -- the yardstick, (b) the same batch in the padded form (one
output padded by a single column: the kernels the coloured form is built from), (c) the coloured batch, a distinct non-identity
ColorJitter matrix per view, (d) the coloured batch with every matrix the identity (the skipped branch), and (e) the unfused
alternative: the uint8 tensor of (a) followed by the torch float pass that applies the matrices of (c) -- matrix, round, clamp, and for
bf16 the normalisation and conversion.

    python tools/colour_probe.py [--rounds 15] [--warmup 3] [--size 224] [--images 1024]

Prints one JSON line: per dtype and batch the median, minimum and maximum of the `resize` launch and of the whole decode from
pjd_batch_decode_timed -- HIP events on the library's stream -- and for (e) of the torch pass from torch's events.  The batches are
resident on one context and decoded in alternation, so that clock and cache state are shared out evenly."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stat(v):
    s = sorted(v)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "n": len(s)}


def random_resized_crop(rng, h, w):
    """torchvision's RandomResizedCrop.get_params with scale (0.08, 1) and ratio (3/4, 4/3): (x, y, w, h)"""
    area = h * w
    for _ in range(10):
        target = area * rng.uniform(0.08, 1.0)
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        cw, ch = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            return rng.randint(0, w - cw), rng.randint(0, h - ch), cw, ch
    side = min(h, w)
    return (w - side) // 2, (h - side) // 2, side, side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    # before anything loads libpjd.so: torch and the library then share one HIP runtime (pjd_amd/tensors.py)
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    import random
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = [s.desc for s in scanned]
    T = args.size
    n = len(descs)
    rng = random.Random(2025)
    views = [i for i in range(n) for _ in range(2)]
    V = len(views)
    crops = [random_resized_crop(rng, int(descs[p].height), int(descs[p].width)) for p in views]
    flips = [rng.random() < 0.5 for _ in views]
    run, windows, oris, pads = tensors.plan_views(descs, views, (T, T), True, crops, flips)
    jitter = [tensors.colour_matrix(brightness=rng.uniform(0.6, 1.4), contrast=rng.uniform(0.6, 1.4), saturation=rng.uniform(0.6, 1.4), hue=rng.uniform(-0.1, 0.1),
                                    grayscale=rng.random() < 0.2) for _ in views]
    assert not any(m == pjd_amd.COLOUR_IDENTITY for m in jitter)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    scale, bias = tensors.normalize_constants(mean, std)
    ctx = pjd_amd.Context(0)
    out = {"probe": "colour_matrix", "workload": label, "size": T, "views": V, "rounds": args.rounds, "launch": {}}
    kinds = ["a_plain", "b_padded", "c_coloured", "d_identity"]
    batches, bufs = {}, {}
    for dname, dt, es in (("u8", None, 1), ("bf16", pjd_amd.DT_BF16, 2)):
        for key in kinds:
            b = ctx.batch(run, pjd_amd.OUT_RGB8_PLANAR)
            b.set_views(views)
            b.set_resize([(T, T)] * V)
            if key == "b_padded":
                b.set_resize_pad([(1, 0, 0, 0)] + [None] * (V - 1), (0, 0, 0))
            if oris is not None:
                b.set_orientation(oris)
            b.set_resize_window(windows if key != "b_padded" else [None] + list(windows[1:]))
            if key == "c_coloured":
                b.set_colour(jitter)
            if key == "d_identity":
                b.set_colour([None] * V)
            if dt is not None:
                b.set_normalize(dt, scale, bias)
            plane = 3 * T * T * es
            buf = torch.empty(V * plane, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), V * plane, [i * plane for i in range(V)])
            b.upload()
            batches[(dname, key)] = b
            bufs[(dname, key)] = buf
    # the unfused pass: the same matrices in float32 on the uint8 tensor of (a)
    A = torch.tensor([[m[0:3], m[4:7], m[8:11]] for m in jitter], dtype=torch.float32, device="cuda:0")
    O = torch.tensor([[m[3], m[7], m[11]] for m in jitter], dtype=torch.float32, device="cuda:0").view(V, 3, 1, 1)
    mean_t = torch.tensor(mean, device="cuda:0").view(1, 3, 1, 1)
    std_t = torch.tensor(std, device="cuda:0").view(1, 3, 1, 1)

    def torch_pass(dname):
        x = bufs[("u8", "a_plain")].view(V, 3, T, T).float()
        y = (torch.einsum("vck,vkhw->vchw", A, x) + O).round_().clamp_(0, 255)
        if dname == "u8":
            return y.to(torch.uint8)
        return y.div_(255).sub_(mean_t).div_(std_t).to(torch.bfloat16)

    def timed_pass(dname):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = torch_pass(dname)
        e1.record()
        torch.cuda.synchronize()
        del r
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
        for d in ("u8", "bf16"):
            timed_pass(d)
    samples = {k: {"resize": [], "total": []} for k in batches}
    passes = {"u8": [], "bf16": []}
    for _ in range(args.rounds):
        for k, b in batches.items():
            per, total = b.decode_timed()
            samples[k]["resize"].append(per["resize"] + per.get("pad", 0.0))
            samples[k]["total"].append(total)
        for d in passes:
            passes[d].append(timed_pass(d))
    # the fused result against the unfused one, once: the float pass rounds half to even where the fixed point rounds half up, and its
    # weights are not quantised, so single levels may differ
    fused = bufs[("u8", "c_coloured")].view(V, 3, T, T)
    diff = (fused.to(torch.int16) - torch_pass("u8").to(torch.int16)).abs()
    out["fused_vs_torch"] = {"max_abs_levels": int(diff.max()), "share_differing": round(float((diff != 0).float().mean()), 6)}
    for (dname, key), b in batches.items():
        b.sync()
        r = {"resize": stat(samples[(dname, key)]["resize"]), "decode_total": stat(samples[(dname, key)]["total"]), "device_bytes": b.info()["device_bytes"],
             "n_fallback": b.info()["n_fallback"]}
        out["launch"].setdefault(dname, {})[key] = r
        b.destroy()
    for d in passes:
        a = out["launch"][d]["a_plain"]
        p = stat(passes[d])
        out["launch"][d]["e_unfused"] = {"torch_pass": p, "resize_plus_pass_ms": round(a["resize"]["median_ms"] + p["median_ms"], 4),
                                         "decode_total_plus_pass_ms": round(a["decode_total"]["median_ms"] + p["median_ms"], 4)}
    out["summary"] = {d: {k: (v["resize"]["median_ms"] if "resize" in v else v["resize_plus_pass_ms"]) for k, v in per.items()} for d, per in out["launch"].items()}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
