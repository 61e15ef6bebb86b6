"""What the affine warp on decode costs: the default bench workload (1024 ragged pictures, box pre-scale) to 224 x 224, planar, bound
into a torch buffer, as uint8 and as normalised bf16, with
(a) the existing bilinear `resize` launch -- the yardstick, (b) `warp` with the pure scaling matrix of the same geometry, (c) `warp`
with that scaling turned by 30 degrees about the two centres, (d) by 90 degrees.

    python tools/warp_probe.py [--rounds 15] [--warmup 3] [--size 224] [--images 1024] [--lib PATH]

Prints one JSON line: per dtype and batch the median, minimum and maximum of the resample launch (`resize` or `warp`) from
pjd_batch_decode_timed -- HIP events on the library's stream -- the sum of the other kernels of the decode, and device_bytes.  The
batches are resident on one context and decoded in alternation, so that clock and cache state are shared out evenly.  --lib loads
another build of libpjd.so: one made with HIPFLAGS_EXTRA="-DPJD_WARP_LX=64 -DPJD_WARP_RPL=8" has the warp in the resize tile's shape
(256 x 8); the tile is 4 * PJD_WARP_LX columns by 64 / PJD_WARP_LX * PJD_WARP_RPL rows."""
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


def turned(sw, sh, T, deg):
    """the scaling sw / T, sh / T of a T x T target, turned by deg about the two centres: (0: the resize's own geometry)"""
    q, r = divmod(deg, 90)
    c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[q % 4] if r == 0 else (math.cos(math.radians(deg)), math.sin(math.radians(deg)))
    sx, sy = sw / T, sh / T
    m = [sx * c, -sx * s, 0.0, sy * s, sy * c, 0.0]
    m[2] = sw / 2 - (m[0] + m[1]) * T / 2
    m[5] = sh / 2 - (m[3] + m[4]) * T / 2
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    # before anything loads libpjd.so: torch and the library then share one HIP runtime (pjd_amd/tensors.py)
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    if args.lib:
        pjd_amd.LIBPJD = os.path.abspath(args.lib)
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    T = args.size
    descs = tensors.prescaled_descs([s.desc for s in scanned], (T, T))
    n = len(descs)
    src = [tensors.output_hw(d) for d in descs]                  # (sh, sw) at the decode size
    ctx = pjd_amd.Context(0)
    scale, bias = tensors.normalize_constants((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    out = {"probe": "affine_warp", "workload": label, "size": T, "rounds": args.rounds, "lib": args.lib, "launch": {}}
    kinds = [("a_resize", None), ("b_warp_scale", 0), ("c_warp_30", 30), ("d_warp_90", 90)]
    batches, keep = {}, []
    for dname, dt, es in (("u8", None, 1), ("bf16", pjd_amd.DT_BF16, 2)):
        for key, deg in kinds:
            b = ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR)
            b.set_resize([(T, T)] * n)
            if deg is not None:
                b.set_resize_affine([turned(sw, sh, T, deg) for sh, sw in src], (0, 0, 0))
            if dt is not None:
                b.set_normalize(dt, scale, bias)
            plane = 3 * T * T * es
            buf = torch.empty(n * plane, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), n * plane, [i * plane for i in range(n)])
            b.upload()
            batches[(dname, key)] = b
            keep.append(buf)
    for _ in range(args.warmup):
        for b in batches.values():
            b.decode_timed()
    samples = {k: {"launch": [], "others": []} for k in batches}
    for _ in range(args.rounds):
        for k, b in batches.items():
            per, total = b.decode_timed()
            name = "resize" if k[1] == "a_resize" else "warp"
            samples[k]["launch"].append(per[name])
            samples[k]["others"].append(sum(v for nm, v in per.items() if nm != name))
    for (dname, key), b in batches.items():
        b.sync()
        r = stat(samples[(dname, key)]["launch"])
        r.update({"other_kernels": stat(samples[(dname, key)]["others"]), "device_bytes": b.info()["device_bytes"], "n_fallback": b.info()["n_fallback"]})
        out["launch"].setdefault(dname, {})[key] = r
        b.destroy()
    out["summary"] = {d: {k + "_ms": v["median_ms"] for k, v in per.items()} for d, per in out["launch"].items()}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
