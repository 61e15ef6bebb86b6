"""What orientation on decode costs: the default bench workload (1024 ragged pictures, box pre-scale, 224 x 224, normalised) with
(a) no orientation, (b) every picture in orientation 3, (c) every picture in 6, (d) orientations mixed 1..8, and (e) the torch pass the
feature replaces for (c): rot90 + .contiguous() over the finished tensor.

    python tools/orientation_probe.py [--rounds 15] [--warmup 3] [--size 224] [--dtype f16|bf16|f32|u8] [--interleaved]

Prints one JSON line: per batch the median, minimum and maximum of the `resize` launch from pjd_batch_decode_timed (the batches are
resident on one context and decoded in alternation, so that clock and cache state are shared out evenly), the sum of the other
kernels of the decode, and device_bytes; for (e) HIP events on torch's stream around torch.rot90(x, -1, (2, 3)).contiguous().  The
square target keeps sizes and offsets of all four batches the same."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stat(v):
    s = sorted(v)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dtype", default="f16", choices=["u8", "f16", "bf16", "f32"])
    ap.add_argument("--interleaved", action="store_true")
    ap.add_argument("--filter", default="bilinear", choices=["bilinear", "antialias", "bicubic"])
    args = ap.parse_args()
    # before anything loads libpjd.so: torch and the library then share one HIP runtime (pjd_amd/tensors.py)
    import torch
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
    T = args.size
    descs = tensors.prescaled_descs([s.desc for s in scanned], (T, T))
    n = len(descs)
    ctx = pjd_amd.Context(0)
    dt = {"u8": None, "f16": pjd_amd.DT_F16, "bf16": pjd_amd.DT_BF16, "f32": pjd_amd.DT_F32}[args.dtype]
    tdt = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]
    scale, bias = tensors.normalize_constants((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    fmt = pjd_amd.OUT_RGB8 if args.interleaved else pjd_amd.OUT_RGB8_PLANAR
    out = {"probe": "orientation", "workload": label, "size": T, "dtype": args.dtype, "interleaved": args.interleaved, "filter": args.filter,
           "rounds": args.rounds, "resize": {}, "torch": {}}
    kinds = [("a_unoriented", None), ("b_all_3", [3] * n), ("c_all_6", [6] * n), ("d_mixed", [1 + i % 8 for i in range(n)])]
    batches = {}
    for key, oris in kinds:
        b = ctx.batch(descs, fmt)
        b.set_resize([(T, T)] * n)
        if oris is not None:
            b.set_orientation(oris)
        if args.filter != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS if args.filter == "antialias" else pjd_amd.RESIZE_BICUBIC)
        if dt is not None:
            b.set_normalize(dt, scale, bias)
        b.upload()
        batches[key] = b
    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
    samples = {k: {"resize": [], "others": []} for k in batches}
    for _ in range(args.rounds):
        for k, b in batches.items():
            per, total = b.decode_timed()
            samples[k]["resize"].append(per["resize"])
            samples[k]["others"].append(sum(v for name, v in per.items() if name != "resize"))
    for k, b in batches.items():
        b.sync()
        r = stat(samples[k]["resize"])
        r.update({"other_kernels": stat(samples[k]["others"]), "device_bytes": b.info()["device_bytes"], "n_fallback": b.info()["n_fallback"]})
        out["resize"][k] = r
        b.destroy()
    # ---- (e) what the feature replaces for (c): the quarter turn over the finished tensor
    x = torch.empty((n, T, T, 3) if args.interleaved else (n, 3, T, T), dtype=tdt, device="cuda:0")
    if tdt == torch.uint8:
        x.random_(0, 256)
    else:
        x.normal_()
    dims = (1, 2) if args.interleaved else (2, 3)
    times = []
    for rnd in range(args.warmup + args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = torch.rot90(x, -1, dims).contiguous()
        e1.record()
        torch.cuda.synchronize()
        if rnd >= args.warmup:
            times.append(e0.elapsed_time(e1))
        del y
    out["torch"]["rot90_contiguous"] = stat(times)
    a = out["resize"]["a_unoriented"]["median_ms"]
    out["summary"] = {"a_ms": a, "a_plus_e_ms": round(a + out["torch"]["rot90_contiguous"]["median_ms"], 4),
                      **{k + "_ms": v["median_ms"] for k, v in out["resize"].items() if k != "a_unoriented"}}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
