"""The three resize filters side by side: the `resize` launch of pjd_batch_decode_timed for the default bench workload (1024 ragged
pictures) to one [N, 3, H, W] tensor, bilinear, antialiased (the widened triangle) and bicubic, as uint8 and as normalised fp16.

    python tools/resize_filter_probe.py [--rounds 60] [--warmup 5] [--size 224] [--images 1024] [--no-prescale]

The pre-scale is the one pjd_amd.tensors chooses (pick_scale_flags) unless --no-prescale.  All six batches are resident on one context
and decoded in alternation, so clock and cache state are shared out evenly; every figure is a median over the rounds, with the
10th and 90th percentile beside it.  Prints one JSON line:
  kernel      per batch ("bilinear_u8", "antialias_f16", ...) the `resize` entry and the decode's total
  taps        per filter the mean number of taps per target sample along x and along y over the batch (bilinear: 2 and 2), the source
              rows a tile of 8 target rows streams (7 x the mean row step + y taps), and `work` = those rows x the x taps: the
              iterations of the horizontal tap loop per lane and tile, which is where the table-driven kernels spend their time
              (it means nothing for the bilinear gather)
  over_antialias   the ratio of each batch's `resize` median to the antialiased one of the same element type, beside the ratios of
              the x taps and of `work` that predict it
No device: the script fails (pjd_amd.Context raises)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(pct(v, 0.1), 4), "p90_ms": round(pct(v, 0.9), 4)}


def mean_taps(pjd_amd, filt, pairs):
    """Mean taps per target sample over the (sn, dn) axes of the batch, sampled at up to 16 target samples per axis."""
    if filt == "bilinear":
        return 2.0
    fn = pjd_amd.resize_aa_taps if filt == "antialias" else pjd_amd.resize_bicubic_taps
    cache, total = {}, 0.0
    for sn, dn in pairs:
        if (sn, dn) not in cache:
            idx = sorted({(k * dn) // 16 for k in range(16)})
            cache[(sn, dn)] = sum(len(fn(sn, dn, i)[1]) for i in idx) / len(idx)
        total += cache[(sn, dn)]
    return total / len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--no-prescale", action="store_true")
    args = ap.parse_args()
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
    if not args.no_prescale:
        descs = tensors.prescaled_descs(descs, (T, T))
    n = len(descs)
    hw = [tensors.output_hw(d) for d in descs]
    scale, bias = tensors.normalize_constants((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    filters = {"bilinear": None, "antialias": pjd_amd.RESIZE_ANTIALIAS, "bicubic": pjd_amd.RESIZE_BICUBIC}
    out = {"probe": "resize_filter", "workload": label, "size": T, "prescale": not args.no_prescale, "rounds": args.rounds, "kernel": {}, "taps": {}}
    step = sum(h for h, _ in hw) / n / T                  # source rows per target row, mean over the batch
    for f in filters:
        tx, ty = mean_taps(pjd_amd, f, [(w, T) for _, w in hw]), mean_taps(pjd_amd, f, [(h, T) for h, _ in hw])
        rows = 7 * step + ty                                # source rows a tile of 8 target rows streams
        out["taps"][f] = {"x": round(tx, 2), "y": round(ty, 2), "rows_per_tile": round(rows, 2), "work": round(rows * tx, 1)}
    ctx = pjd_amd.Context(0)
    batches = {}
    for f, value in filters.items():
        for et in ("u8", "f16"):
            b = ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR)
            b.set_resize([(T, T)] * n)
            if value is not None:
                b.set_resize_filter(value)
            if et == "f16":
                b.set_normalize(pjd_amd.DT_F16, scale, bias)
            b.upload()
            batches[f"{f}_{et}"] = b
    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
    samples = {k: {"resize": [], "total": []} for k in batches}
    for _ in range(args.rounds):
        for k, b in batches.items():
            per, total = b.decode_timed()
            samples[k]["resize"].append(per["resize"])
            samples[k]["total"].append(total)
    for k, b in batches.items():
        b.sync()
        out["kernel"][k] = {"resize": stat(samples[k]["resize"]), "total": stat(samples[k]["total"]), "n_fallback": b.info()["n_fallback"]}
        b.destroy()
    ctx.close()
    out["over_antialias"] = {}
    for k in out["kernel"]:
        f, et = k.rsplit("_", 1)
        out["over_antialias"][k] = {"measured": round(out["kernel"][k]["resize"]["median_ms"] / out["kernel"]["antialias_" + et]["resize"]["median_ms"], 3),
                                    "taps_x": round(out["taps"][f]["x"] / out["taps"]["antialias"]["x"], 3),
                                    "work": round(out["taps"][f]["work"] / out["taps"]["antialias"]["work"], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
