"""What resize on decode costs and what it saves: the default bench workload (1024 ragged pictures) to one uint8[N, 3, H, W] tensor.

    python tools/resize_probe.py [--rounds 60] [--warmup 5] [--size 224] [--e2e-rounds 20] [--antialias] [--window]

Prints one JSON line:
  kernel    per batch kind (prescale = pick_scale_flags, noprescale = full-size decode; planar and rgb8; planar bound to a torch
            buffer) the median, minimum, maximum and 10th / 90th percentile of every kernel's time from pjd_batch_decode_timed, the batches resident on one
            context and decoded in alternation; beside the `resize` kernel the bytes it has to move, computed from the shapes (the
            source footprint read once + the output written once), and what that is in GB/s
  e2e       the same tensor two ways, host clock around a device synchronise, from "upload done" to "tensor complete", alternating:
            `resized`   a bound, resized, captured batch: decode + sync
            `torch`     today's route: a bound planar batch of ragged pictures (what decode_to_tensors makes), decode + sync, then one
                        torch.nn.functional.interpolate per picture into a preallocated [N, 3, H, W] tensor
            each with and without the box pre-scale
  device_bytes of the resized default batch, unbound and bound
--antialias: every batch kind a second time with the antialiased filter (Batch.set_resize_filter, key suffix `_aa`), resident beside
its bilinear twin and decoded in the same alternation, and `aa_over_bilinear`: the ratio of the two `resize` medians per kind.
--window: every batch kind (and its `_aa` twin) a second time with source windows (Batch.set_resize_window, key suffix `_win`): seeded
RandomResizedCrop windows with torchvision's defaults (area 8-100 %, aspect 3/4-4/3), every second picture mirrored; with the pre-scale
the scale is picked from the crop's size, as pjd_amd.tensors does.  Resident beside the un-windowed twin and decoded in the same
alternation.  `window` holds, per kind, the `resize` launch windowed beside un-windowed: both medians, the un-windowed launch's own
spread in this run (min, max, and the 10th and 90th percentile), and their ratio.
--e2e-rounds 0 leaves the end-to-end part out.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "p10_ms": round(pct(v, 0.1), 4), "p90_ms": round(pct(v, 0.9), 4)}


def random_resized_crop(rng, W, H):
    """torchvision's RandomResizedCrop.get_params with its defaults (area 8-100 %, aspect 3/4-4/3, log-uniform; ten tries, then the
    centre crop at the nearest allowed aspect) -> (x, y, w, h); rng: a numpy Generator."""
    for _ in range(10):
        area = W * H * rng.uniform(0.08, 1.0)
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h
    r = W / H
    w, h = (W, int(round(W / (3 / 4)))) if r < 3 / 4 else ((int(round(H * (4 / 3))), H) if r > 4 / 3 else (W, H))
    return (W - w) // 2, (H - h) // 2, w, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e-rounds", type=int, default=20)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--antialias", action="store_true")
    ap.add_argument("--window", action="store_true")
    args = ap.parse_args()
    # before anything loads libpjd.so: torch and the library then share one HIP runtime (pjd_amd/tensors.py)
    import torch
    import torch.nn.functional as F
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = {"noprescale": [s.desc for s in scanned]}
    T = args.size
    descs["prescale"] = tensors.prescaled_descs(descs["noprescale"], (T, T))
    n = len(jpegs)
    plane = 3 * T * T
    ctx = pjd_amd.Context(0)
    out = {"probe": "resize", "workload": label, "size": T, "rounds": max(args.rounds, 60), "kernel": {}, "e2e": {}, "device_bytes": {}}

    # ---- kernel times
    kinds = [("prescale", "planar", False), ("noprescale", "planar", False), ("prescale", "rgb8", False), ("noprescale", "rgb8", False),
             ("prescale", "planar", True)]
    batches, keep = {}, []
    kinds = [k + (False,) for k in kinds] + ([k + (True,) for k in kinds] if args.antialias else [])
    kinds = [k + (False,) for k in kinds] + ([k + (True,) for k in kinds] if args.window else [])
    windows = {}
    if args.window:
        import numpy as np
        rng = np.random.default_rng(7)
        crops = [random_resized_crop(rng, int(d.width), int(d.height)) for d in descs["noprescale"]]
        flips = [i % 2 == 1 for i in range(n)]
        for pre in ("prescale", "noprescale"):
            descs[pre + "_win"], windows[pre] = tensors._plan_outputs(descs["noprescale"], (T, T), pre == "prescale", crops, flips, None)[:2]
    for pre, fmt, bound, antialias, windowed in kinds:
        key = f"{pre}_{fmt}" + ("_bound" if bound else "") + ("_aa" if antialias else "") + ("_win" if windowed else "")
        if windowed:
            pre = pre + "_win"
        b = ctx.batch(descs[pre], pjd_amd.OUT_RGB8_PLANAR if fmt == "planar" else pjd_amd.OUT_RGB8)
        b.set_resize([(T, T)] * n)
        if windowed:
            b.set_resize_window(windows[pre[:-4]])
        if antialias:
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        out["device_bytes"][key] = b.info()["device_bytes"]
        if bound:
            buf = torch.empty(n * plane, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), n * plane, [i * plane for i in range(n)])
            keep.append(buf)
            out["device_bytes"][key] = b.info()["device_bytes"]
        b.upload()
        batches[key] = b
        src = sum(3 * tensors.output_hw(d)[0] * tensors.output_hw(d)[1] for d in descs[pre])
        out["kernel"][key] = {"src_bytes": src, "dst_bytes": n * plane}
    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
    samples = {k: {} for k in batches}
    for _ in range(max(args.rounds, 60)):
        for k, b in batches.items():                                        # alternation: clock and cache state are shared out evenly
            per_kernel, total = b.decode_timed()
            per_kernel["total"] = total
            for name, ms in per_kernel.items():
                samples[k].setdefault(name, []).append(ms)
    for k, b in batches.items():
        b.sync()
        for name, v in samples[k].items():
            out["kernel"][k][name] = stat(v)
        moved = out["kernel"][k]["src_bytes"] + out["kernel"][k]["dst_bytes"]
        out["kernel"][k]["resize_gb_per_s"] = round(moved / (out["kernel"][k]["resize"]["median_ms"] * 1e-3) / 1e9, 1)
        out["kernel"][k]["n_fallback"] = b.info()["n_fallback"]
        b.destroy()
    keep.clear()
    if args.antialias:
        out["aa_over_bilinear"] = {k: round(out["kernel"][k + "_aa"]["resize"]["median_ms"] / out["kernel"][k]["resize"]["median_ms"], 2)
                                   for k in list(out["kernel"]) if not k.endswith("_aa") and k + "_aa" in out["kernel"]}
    if args.window:
        out["window"] = {}
        for k in [k for k in out["kernel"] if not k.endswith("_win")]:
            plain, win = samples[k]["resize"], samples[k + "_win"]["resize"]
            out["window"][k] = {"plain_ms": stat(plain)["median_ms"], "plain_min_ms": round(min(plain), 4), "plain_max_ms": round(max(plain), 4),
                                "plain_p10_ms": round(pct(plain, 0.1), 4), "plain_p90_ms": round(pct(plain, 0.9), 4),
                                "windowed_ms": stat(win)["median_ms"], "windowed_min_ms": round(min(win), 4), "windowed_max_ms": round(max(win), 4),
                                "windowed_over_plain": round(statistics.median(win) / statistics.median(plain), 3)}

    # ---- end to end against today's route
    runs = {}
    for pre in ("prescale", "noprescale") if args.e2e_rounds > 0 else ():
        result = torch.empty(n, 3, T, T, dtype=torch.uint8, device="cuda:0")
        b = ctx.batch(descs[pre], pjd_amd.OUT_RGB8_PLANAR)
        b.set_resize([(T, T)] * n)
        b.bind_output(result.data_ptr(), n * plane, [i * plane for i in range(n)])
        b.upload(); b.capture(); b.sync()

        def run_resized(b=b):
            b.decode(); b.sync()
        runs[f"resized_{pre}"] = (run_resized, b, result)

        rb = ctx.batch(descs[pre], pjd_amd.OUT_RGB8_PLANAR)
        size = rb.packed_size()
        buf = torch.empty(size, dtype=torch.uint8, device="cuda:0")
        rb.bind_output(buf.data_ptr(), size)
        views = []
        for i, d in enumerate(descs[pre]):
            h, w = tensors.output_hw(d)
            off = rb.output_offset(i)
            views.append(buf[off:off + 3 * h * w].view(1, 3, h, w))
        rb.upload(); rb.capture(); rb.sync()
        dst = torch.empty(n, 3, T, T, dtype=torch.uint8, device="cuda:0")

        def run_torch(rb=rb, views=views, dst=dst):
            rb.decode(); rb.sync()
            for i, v in enumerate(views):
                dst[i] = F.interpolate(v.float(), size=(T, T), mode="bilinear", align_corners=False).round_().to(torch.uint8)[0]
            torch.cuda.synchronize()
        runs[f"torch_{pre}"] = (run_torch, rb, (buf, dst))
    times = {k: [] for k in runs}
    for rnd in range(args.e2e_rounds + 2):
        for k, (fn, _, _) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd >= 2:
                times[k].append(dt)
    for k in runs:
        out["e2e"][k] = stat(times[k])
    for pre in ("prescale", "noprescale") if args.e2e_rounds > 0 else ():
        a, bq = runs[f"resized_{pre}"][2], runs[f"torch_{pre}"][2][1]
        out["e2e"][f"max_abs_difference_{pre}"] = int((a.to(torch.int16) - bq.to(torch.int16)).abs().max().item())
        out["e2e"][f"torch_over_resized_{pre}"] = round(out["e2e"][f"torch_{pre}"]["median_ms"] / out["e2e"][f"resized_{pre}"]["median_ms"], 2)
    for _, b, _ in runs.values():
        b.destroy()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
