"""What resize on decode costs and what it saves: the default bench workload (1024 ragged pictures) to one uint8[N, 3, H, W] tensor.

    python tools/resize_probe.py [--rounds 60] [--warmup 5] [--size 224] [--e2e-rounds 20] [--antialias]

Prints one JSON line:
  kernel    per batch kind (prescale = pick_scale_flags, noprescale = full-size decode; planar and rgb8; planar bound to a torch
            buffer) the median, minimum and maximum of every kernel's time from pjd_batch_decode_timed, the batches resident on one
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
--e2e-rounds 0 leaves the end-to-end part out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e-rounds", type=int, default=20)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--antialias", action="store_true")
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
    for pre, fmt, bound, antialias in kinds:
        key = f"{pre}_{fmt}" + ("_bound" if bound else "") + ("_aa" if antialias else "")
        b = ctx.batch(descs[pre], pjd_amd.OUT_RGB8_PLANAR if fmt == "planar" else pjd_amd.OUT_RGB8)
        b.set_resize([(T, T)] * n)
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
                                   for k in list(out["kernel"]) if not k.endswith("_aa")}

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
