"""What pad on decode costs: the default bench workload (1024 ragged pictures, box pre-scale, normalised) letterboxed into a size x size
canvas.  The content of every picture is tensors.letterbox_plan of it into a canvas eight columns narrower, so that it can be placed
at any left pad up to 8; its top pad centres it.  Batches:
(a) the contents alone: every picture resized to its content size, no pad -- the launch a caller without the feature runs before they
    pad each picture themselves (these kernels are instruction for instruction those of the commit before the feature);
(b) padded, left = 4: with a canvas width that is a multiple of four the content rows start on multiples of four elements;
(c) padded, left = 5: the odd placement, whose content rows take the element stores of store_row;
(d) all-zero records: the batch of (a) with the call, which must launch what (a) launches.

    python tools/resize_pad_probe.py [--rounds 15] [--warmup 3] [--size 224] [--dtype f16|bf16|f32|u8] [--interleaved] [--filter ...]

Prints one JSON line: per batch the median, minimum and maximum of the `resize` and `pad` launches from pjd_batch_decode_timed (the
batches are resident on one context and decoded in alternation, so that clock and cache state are shared out evenly), the sum of the
other kernels, device_bytes, and the border bytes the pad launch writes."""
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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    T = args.size
    n = len(scanned)
    plans = [tensors.letterbox_plan((int(s.desc.height), int(s.desc.width)), (T, T - 8), "center") for s in scanned]
    descs = [tensors.prescaled_descs([s.desc], (p[0], p[1]))[0] for s, p in zip(scanned, plans)]
    ctx = pjd_amd.Context(0)
    dt = {"u8": None, "f16": pjd_amd.DT_F16, "bf16": pjd_amd.DT_BF16, "f32": pjd_amd.DT_F32}[args.dtype]
    es = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4}[args.dtype]
    scale, bias = tensors.normalize_constants((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    fmt = pjd_amd.OUT_RGB8 if args.interleaved else pjd_amd.OUT_RGB8_PLANAR

    def pads(left):
        return [(left, p[3], T - p[1] - left, p[5]) for p in plans]

    content_bytes = sum(3 * p[0] * p[1] * es for p in plans)
    out = {"probe": "resize_pad", "workload": label, "size": T, "dtype": args.dtype, "interleaved": args.interleaved, "filter": args.filter,
           "rounds": args.rounds, "content_bytes": content_bytes, "border_bytes": 3 * T * T * es * n - content_bytes, "batches": {}}
    kinds = [("a_contents_alone", [(p[0], p[1]) for p in plans], None), ("b_left_4", [(T, T)] * n, pads(4)), ("c_left_5", [(T, T)] * n, pads(5)),
             ("d_zero_records", [(p[0], p[1]) for p in plans], [None] * n)]
    batches = {}
    for key, sizes, pd in kinds:
        b = ctx.batch(descs, fmt)
        b.set_resize(sizes)
        if pd is not None:
            b.set_resize_pad(pd, (114, 114, 114))
        if args.filter != "bilinear":
            b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS if args.filter == "antialias" else pjd_amd.RESIZE_BICUBIC)
        if dt is not None:
            b.set_normalize(dt, scale, bias)
        b.upload()
        batches[key] = b
    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
    samples = {k: {"resize": [], "pad": [], "both": [], "others": []} for k in batches}
    for _ in range(args.rounds):
        for k, b in batches.items():
            per, total = b.decode_timed()
            samples[k]["resize"].append(per["resize"])
            samples[k]["pad"].append(per.get("pad", 0.0))
            samples[k]["both"].append(per["resize"] + per.get("pad", 0.0))
            samples[k]["others"].append(sum(v for name, v in per.items() if name not in ("resize", "pad")))
    for k, b in batches.items():
        b.sync()
        info = b.info()
        out["batches"][k] = {"resize": stat(samples[k]["resize"]), "pad": stat(samples[k]["pad"]), "resize_plus_pad": stat(samples[k]["both"]),
                             "other_kernels": stat(samples[k]["others"]), "device_bytes": info["device_bytes"], "out_bytes": info["out_bytes"],
                             "n_fallback": info["n_fallback"]}
        b.destroy()
    a = out["batches"]["a_contents_alone"]["resize"]["median_ms"]
    out["summary"] = {"a_ms": a, **{k + "_extra_ms": round(v["resize_plus_pad"]["median_ms"] - a, 4) for k, v in out["batches"].items() if k != "a_contents_alone"}}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
