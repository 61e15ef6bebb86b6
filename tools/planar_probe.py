"""What the planar store costs: per-kernel times of the default bench workload as PJD_OUT_RGB8, as PJD_OUT_RGB8_PLANAR and as
PJD_OUT_RGB8_PLANAR bound to a torch buffer (pjd_batch_bind_output), the three batches resident on one context and decoded in
alternation with pjd_batch_decode_timed.  Prints one JSON line: per batch kind the median, minimum and maximum of every kernel's
time over the rounds, the planar / RGB8 ratio of the back-end kernel, and device_bytes of the batches.

    python tools/planar_probe.py [--rounds 60] [--warmup 5] [--kinds rgb8,planar,bound] [--package DIR]

--package: the directory that holds the pjd_amd package of the build to measure (default: this tree's); with --kinds rgb8 the probe
runs on a build that predates the planar format, so that two builds can be compared in one session on the same device.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--kinds", default="rgb8,planar,bound")
    ap.add_argument("--package", default=os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    kinds = [k for k in args.kinds.split(",") if k]
    if "bound" in kinds:
        # before anything loads libpjd.so: torch and the library then share one HIP runtime (pjd_amd/tensors.py)
        import torch
        torch.zeros(1, device="cuda:0")
        torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, args.package)
    import pjd_amd
    import bench
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = [s.desc for s in scanned]
    ctx = pjd_amd.Context(0)
    batches, keep, dev_bytes = {}, [], {}
    for kind in kinds:
        fmt = pjd_amd.OUT_RGB8 if kind == "rgb8" else pjd_amd.OUT_RGB8_PLANAR
        b = ctx.batch(descs, fmt)
        if kind == "bound":
            size = b.packed_size()
            buf = torch.empty(size, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), size)
            keep.append(buf)
        b.upload()
        batches[kind] = b
        dev_bytes[kind] = b.info()["device_bytes"]
    for _ in range(args.warmup):
        for kind in kinds:
            batches[kind].decode_timed()
    samples = {kind: {} for kind in kinds}
    for _ in range(max(args.rounds, 50)):
        for kind in kinds:                                                  # alternation: clock and cache state are shared out evenly
            per_kernel, total = batches[kind].decode_timed()
            per_kernel["total"] = total
            for name, ms in per_kernel.items():
                samples[kind].setdefault(name, []).append(ms)
    out = {"probe": "planar", "label": args.label, "workload": label, "rounds": max(args.rounds, 50), "kinds": {}, "device_bytes": dev_bytes}
    for kind in kinds:
        batches[kind].sync()
        info = batches[kind].info()
        out["kinds"][kind] = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                              for name, v in samples[kind].items()}
        out["kinds"][kind]["n_fallback"] = info["n_fallback"]
        out["pixels"] = info["pixels"]
    if "rgb8" in kinds:
        base = out["kinds"]["rgb8"]["idct_colour"]["median_ms"]
        for kind in kinds:
            if kind != "rgb8":
                out[f"idct_colour_{kind}_over_rgb8"] = round(out["kinds"][kind]["idct_colour"]["median_ms"] / base, 4)
    for b in batches.values():
        b.destroy()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
