"""What the libjpeg-exact mode (PJD_F_LIBJPEG) costs: bench.py's default workload (1024 ImageNet-like 4:2:0 pictures) decoded without and
with the flag, the two batches resident on one context and decoded in alternation.

    python tools/libjpeg_probe.py [--rounds 40] [--warmup 5] [--images 1024] [--format rgb8|planar|bmp]

Prints one JSON line:
  default    per launch of pjd_batch_decode_timed (one chain of launches) the median, minimum, maximum and 10th..90th percentile
  libjpeg    the same for the flagged batch: "idct_std" (entry parser + islow IDCT into component planes) and "colour_std"
             (fancy upsampling + colour + store) stand where the unflagged batch has "idct_colour"
  backend    median of idct_colour against idct_std + colour_std, and their ratio
  planes     bytes of the plane buffer (written once by idct_std, read by colour_std: at 4:2:0 1.5 bytes a pixel each way, the cost
             a fused form with recomputed halo units would save), pictures' bytes written by colour_std, and what the two launches
             move in GB/s by that count
  identical  the unflagged batch's pictures equal those of a batch created before the flagged one existed (nothing leaks between them)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stat(v):
    s = sorted(v)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--format", default="rgb8", choices=["rgb8", "planar", "bmp"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import numpy as np
    import pjd_amd
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = [s.desc for s in scanned]
    fmt = {"rgb8": pjd_amd.OUT_RGB8, "planar": pjd_amd.OUT_RGB8_PLANAR, "bmp": pjd_amd.OUT_BMP}[args.format]
    ctx = pjd_amd.Context(0)
    out = {"probe": "libjpeg", "workload": label, "format": args.format, "rounds": args.rounds}
    with ctx.batch(descs, fmt) as plain:
        plain.upload(); plain.decode(); plain.sync()
        before, _ = plain.download()
        with ctx.batch(tensors.libjpeg_descs(descs), fmt) as lj:
            lj.upload()
            runs = {"default": {}, "libjpeg": {}}
            for r in range(args.warmup + args.rounds):
                for name, b in (("default", plain), ("libjpeg", lj)):
                    t, total = b.decode_timed()
                    b.sync()
                    if r >= args.warmup:
                        for k, ms in t.items():
                            runs[name].setdefault(k, []).append(ms)
                        runs[name].setdefault("total", []).append(total)
            after, st = plain.download()
            _, st_lj = lj.download()
            info, info_lj = plain.info(), lj.info()
    for name in runs:
        out[name] = {k: stat(v) for k, v in runs[name].items()}
    med = lambda name, k: statistics.median(runs[name][k])
    back_default, back_lj = med("default", "idct_colour"), med("libjpeg", "idct_std") + med("libjpeg", "colour_std")
    out["backend"] = {"default_ms": round(back_default, 4), "libjpeg_ms": round(back_lj, 4), "ratio": round(back_lj / back_default, 3)}
    plane_bytes = 0
    for d in descs:
        mx, my = (d.width + 8 * d.h_samp - 1) // (8 * d.h_samp), (d.height + 8 * d.v_samp - 1) // (8 * d.v_samp)
        plane_bytes += mx * my * 64 * (d.h_samp * d.v_samp + (2 if d.num_components == 3 else 0))
    out["planes"] = {"plane_bytes": plane_bytes, "bytes_per_pixel": round(plane_bytes / info["pixels"], 3), "out_bytes": info_lj["out_bytes"],
                     "idct_std_GBps": round(plane_bytes / med("libjpeg", "idct_std") / 1e6, 1),
                     "colour_std_GBps": round((plane_bytes + info_lj["out_bytes"]) / med("libjpeg", "colour_std") / 1e6, 1),
                     "device_bytes_default": info["device_bytes"], "device_bytes_libjpeg": info_lj["device_bytes"]}
    out["pixels"] = info["pixels"]
    out["statuses_ok"] = bool(list(st) == [0] * len(descs) and list(st_lj) == [0] * len(descs))
    out["identical"] = bool(all(np.array_equal(a, b) for a, b in zip(before, after)))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
