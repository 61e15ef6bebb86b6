"""What the Gaussian blur on decode costs: the default bench workload (1024 ragged pictures, box pre-scale), two 224 x 224
RandomResizedCrop views per picture (seeded crops and flips), planar, bound into a torch buffer, as uint8 and as normalised bf16, with
(a) the batch without set_blur, (b) the same batch with set_blur -- 23 taps, a seeded sigma in [0.1, 2], on half of the views (p = 0.5,
seeded), None on the others -- and (c) the unfused alternative a caller writes today: the uint8 tensor of (a) followed by the eager torch
pass over the blurred half -- float conversion, reflect pad, two depthwise conv2d with each view's own kernel, round and clamp, and for
bf16 the normalisation and conversion of the whole batch.

    python tools/blur_probe.py [--rounds 15] [--warmup 3] [--size 224] [--images 1024]

Prints one JSON line: per dtype and batch the median, minimum and maximum of the `blur` launch (where there is one) and of the whole
decode from pjd_batch_decode_timed -- HIP events on the library's stream -- and for (c) of the torch pass from torch's events; the
spread of (a) over the alternations; and the bytes the blur launch reads and writes, with the time they take at the HBM rate given on
the command line (--hbm-gbs, measured copy rate).  The batches are resident on one context and decoded in alternation, so that clock and
cache state are shared out evenly."""
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
    ap.add_argument("--ksize", type=int, default=23)
    ap.add_argument("--hbm-gbs", type=float, default=6290.0, help="the HBM rate the floor is derived from, GB/s (default: a measured float4 copy on an MI355X)")
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
    T, K = args.size, args.ksize
    n = len(descs)
    rng = random.Random(2025)
    views = [i for i in range(n) for _ in range(2)]
    V = len(views)
    crops = [random_resized_crop(rng, int(descs[p].height), int(descs[p].width)) for p in views]
    flips = [rng.random() < 0.5 for _ in views]
    run, windows, oris, pads = tensors.plan_views(descs, views, (T, T), True, crops, flips)
    blurs = [(K, rng.uniform(0.1, 2.0)) if rng.random() < 0.5 else None for _ in views]
    which = [v for v, e in enumerate(blurs) if e is not None]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    scale, bias = tensors.normalize_constants(mean, std)
    ctx = pjd_amd.Context(0)
    out = {"probe": "gaussian_blur", "workload": label, "size": T, "views": V, "blurred_views": len(which), "ksize": K, "rounds": args.rounds, "launch": {}}
    kinds = ["a_plain", "b_blurred"]
    batches, bufs = {}, {}
    for dname, dt, es in (("u8", None, 1), ("bf16", pjd_amd.DT_BF16, 2)):
        for key in kinds:
            b = ctx.batch(run, pjd_amd.OUT_RGB8_PLANAR)
            b.set_views(views)
            b.set_resize([(T, T)] * V)
            if oris is not None:
                b.set_orientation(oris)
            b.set_resize_window(windows)
            if key == "b_blurred":
                b.set_blur(blurs)
            if dt is not None:
                b.set_normalize(dt, scale, bias)
            plane = 3 * T * T * es
            buf = torch.empty(V * plane, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), V * plane, [i * plane for i in range(V)])
            b.upload()
            batches[(dname, key)] = b
            bufs[(dname, key)] = buf
    # the unfused pass: torchvision's gaussian_blur on the blurred half, each view with its own kernel (one group per view and channel)
    r = K // 2
    idx = torch.tensor(which, device="cuda:0")
    x1 = torch.arange(-r, r + 1, dtype=torch.float32, device="cuda:0")
    sig = torch.tensor([blurs[v][1] for v in which], dtype=torch.float32, device="cuda:0").view(-1, 1)
    k1 = torch.exp(-0.5 * (x1.view(1, -1) / sig) ** 2)
    k1 = (k1 / k1.sum(dim=1, keepdim=True)).repeat_interleave(3, dim=0)      # [3 * B, K]
    G = k1.shape[0]
    mean_t = torch.tensor(mean, device="cuda:0").view(1, 3, 1, 1)
    std_t = torch.tensor(std, device="cuda:0").view(1, 3, 1, 1)

    def torch_pass(dname):
        u = bufs[("u8", "a_plain")].view(V, 3, T, T)
        x = u[idx].float().view(1, G, T, T)
        x = torch.nn.functional.pad(x, (r, r, r, r), mode="reflect")
        x = torch.nn.functional.conv2d(x, k1.view(G, 1, 1, K), groups=G)
        x = torch.nn.functional.conv2d(x, k1.view(G, 1, K, 1), groups=G)
        y = x.view(-1, 3, T, T).round_().clamp_(0, 255).to(torch.uint8)
        if dname == "u8":
            res = u.clone()
            res[idx] = y
            return res
        res = u.float()
        res[idx] = y.float()
        return res.div_(255).sub_(mean_t).div_(std_t).to(torch.bfloat16)

    def timed_pass(dname):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = torch_pass(dname)
        e1.record()
        torch.cuda.synchronize()
        del res
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
        for d in ("u8", "bf16"):
            timed_pass(d)
    samples = {k: {"blur": [], "resize": [], "total": []} for k in batches}
    passes = {"u8": [], "bf16": []}
    for _ in range(args.rounds):
        for k, b in batches.items():
            per, total = b.decode_timed()
            samples[k]["blur"].append(per.get("blur", 0.0))
            samples[k]["resize"].append(per["resize"])
            samples[k]["total"].append(total)
        for d in passes:
            passes[d].append(timed_pass(d))
    # the fused result against the unfused one, once: the float pass keeps no 8-bit row sample and its weights are not quantised, so
    # single levels may differ
    fused = bufs[("u8", "b_blurred")].view(V, 3, T, T)
    diff = (fused.to(torch.int16) - torch_pass("u8").to(torch.int16)).abs()
    out["fused_vs_torch"] = {"max_abs_levels": int(diff.max()), "share_differing": round(float((diff != 0).float().mean()), 6)}
    for (dname, key), b in batches.items():
        b.sync()
        s = samples[(dname, key)]
        res = {"resize": stat(s["resize"]), "decode_total": stat(s["total"]), "device_bytes": b.info()["device_bytes"], "n_fallback": b.info()["n_fallback"]}
        if key == "b_blurred":
            res["blur"] = stat(s["blur"])
        out["launch"].setdefault(dname, {})[key] = res
        b.destroy()
    for d, es in (("u8", 1), ("bf16", 2)):
        a, bb = out["launch"][d]["a_plain"], out["launch"][d]["b_blurred"]
        p = stat(passes[d])
        out["launch"][d]["c_unfused"] = {"torch_pass": p, "decode_total_plus_pass_ms": round(a["decode_total"]["median_ms"] + p["median_ms"], 4)}
        spread = a["decode_total"]["max_ms"] - a["decode_total"]["min_ms"]
        moved = V * 3 * T * T * (1 + es)                      # the launch reads U once (the halo from cache) and writes every element once
        out["launch"][d]["verdict"] = {
            "a_spread_ms": round(spread, 4),
            "b_minus_a_ms": round(bb["decode_total"]["median_ms"] - a["decode_total"]["median_ms"], 4),
            "c_minus_b_ms": round(a["decode_total"]["median_ms"] + p["median_ms"] - bb["decode_total"]["median_ms"], 4),
            "b_faster_than_c_by_more_than_the_spread": a["decode_total"]["median_ms"] + p["median_ms"] - bb["decode_total"]["median_ms"] > spread,
            "blur_bytes_moved": moved, "blur_floor_ms_at_hbm_rate": round(moved / (args.hbm_gbs * 1e9) * 1e3, 4), "hbm_gbs": args.hbm_gbs}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
