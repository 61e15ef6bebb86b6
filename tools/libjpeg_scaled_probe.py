"""What libjpeg's reduced decode saves: the default bench workload flagged PJD_F_LIBJPEG at 1/1 and with PJD_F_LIBJPEG_SCALE_1_2, _1_4 and
_1_8, as PJD_OUT_RGB8_PLANAR and as PJD_OUT_GRAY8 -- the four batches of a format resident on one context and decoded in alternation
with pjd_batch_decode_timed, so that clock and cache state are shared out evenly and the baseline is the 1/1 batch OF THE SAME PROCESS.
Then the same flagged workload resized to 224 x 224 (pjd_batch_set_resize, bilinear): every picture at full size (prescale=False, what
libjpeg=True meant before) against draft=True (each picture at the scale tensors.pick_libjpeg_scale_flags chooses), alternating.  Prints
one JSON line: per batch the median, minimum and maximum of every kernel's time, of the back end (idct_std + colour_std, or
idct_gray_std), of the whole decode and of pjd_batch_download_packed over the rounds, device_bytes and out_bytes, and the ratios to 1/1.

    python tools/libjpeg_scaled_probe.py [--rounds 60] [--warmup 5] [--images 1024]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACK = ("idct_colour", "idct_std", "colour_std", "idct_gray", "idct_gray_std")


def alternate(pjd_amd, ctx, batches, n_images, rounds, warmup, download=True):
    """batches: {label: uploaded Batch}, decoded in alternation -> {label: {name: {median, min, max}, device_bytes, out_bytes}}"""
    L = pjd_amd.dev_lib()
    hosts = {k: (L.pjd_host_alloc(b.packed_size()), b.packed_size()) for k, b in batches.items()} if download else {}
    st = (C.c_int32 * max(n_images, 1))()

    def fetch(kind):
        host, size = hosts[kind]
        t0 = time.perf_counter()
        ctx._check(L.pjd_batch_download_packed(batches[kind]._h, host, size, st), "pjd_batch_download_packed")
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        for kind, b in batches.items():
            b.decode_timed()
            b.sync()
            if download:
                fetch(kind)
    samples = {kind: {} for kind in batches}
    for _ in range(max(rounds, 50)):
        for kind, b in batches.items():
            per_kernel, total = b.decode_timed()
            per_kernel["back_end"] = sum(ms for name, ms in per_kernel.items() if name in BACK)
            per_kernel["total"] = total
            b.sync()                                                        # the download below then times the copy alone
            if download:
                per_kernel["download_packed"] = fetch(kind)
            for name, ms in per_kernel.items():
                samples[kind].setdefault(name, []).append(ms)
    out = {}
    for kind, b in batches.items():
        info = b.info()
        out[kind] = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for name, v in samples[kind].items()}
        out[kind].update(device_bytes=info["device_bytes"], out_bytes=info["out_bytes"], n_fallback=info["n_fallback"],
                         statuses_nonzero=sum(1 for s in b.statuses() if s))
    for kind in hosts:
        L.pjd_host_free(hosts[kind][0])
    return out


def flagged_at(pjd_amd, descs, bits):
    import ctypes
    out = []
    for d in descs:
        c = pjd_amd.ImageDesc()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(pjd_amd.ImageDesc))
        c.flags = (int(d.flags) & ~pjd_amd.F_LIBJPEG_SCALE_MASK) | pjd_amd.F_LIBJPEG | bits
        out.append(c)
    return out


def ratios(res, base, name):
    return {k: round(v[name]["median_ms"] / res[base][name]["median_ms"], 4) for k, v in res.items() if name in v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = [d for d in tensors.libjpeg_descs([s.desc for s in scanned]) if pjd_amd.plan_check([d], pjd_amd.OUT_GRAY8)[0] == 0]
    ctx = pjd_amd.Context(0)
    out = {"probe": "libjpeg_scaled", "workload": label, "rounds": max(args.rounds, 50), "n_images": len(descs)}
    scales = {"1/1": 0, "1/2": pjd_amd.F_LIBJPEG_SCALE_1_2, "1/4": pjd_amd.F_LIBJPEG_SCALE_1_4, "1/8": pjd_amd.F_LIBJPEG_SCALE_1_8}
    for kind, fmt in (("planar", pjd_amd.OUT_RGB8_PLANAR), ("gray", pjd_amd.OUT_GRAY8)):
        keep = {k: flagged_at(pjd_amd, descs, bits) for k, bits in scales.items()}
        batches = {k: ctx.batch(v, fmt) for k, v in keep.items()}
        for b in batches.values():
            b.upload()
        res = alternate(pjd_amd, ctx, batches, len(descs), args.rounds, args.warmup)
        out[kind] = res
        out[kind + "_back_end_over_full"] = ratios(res, "1/1", "back_end")
        out[kind + "_total_over_full"] = ratios(res, "1/1", "total")
        out[kind + "_download_over_full"] = ratios(res, "1/1", "download_packed")
        out[kind + "_device_bytes_over_full"] = {k: round(v["device_bytes"] / res["1/1"]["device_bytes"], 4) for k, v in res.items()}
        for b in batches.values():
            b.destroy()
    # the ragged batch into one 224 x 224 tensor's worth: full-size decode + resample against drafted decode + resample
    size = (224, 224)
    keep = {"prescale=False": flagged_at(pjd_amd, descs, 0), "draft=True": tensors.drafted_descs(flagged_at(pjd_amd, descs, 0), size)}
    picked = {}
    for d in keep["draft=True"]:
        s = 1 << ((int(d.flags) & pjd_amd.F_LIBJPEG_SCALE_MASK) >> 7)
        picked[f"1/{s}"] = picked.get(f"1/{s}", 0) + 1
    batches = {}
    for k, v in keep.items():
        b = ctx.batch(v, pjd_amd.OUT_RGB8_PLANAR)
        b.set_resize([size] * len(v))
        b.upload()
        batches[k] = b
    res = alternate(pjd_amd, ctx, batches, len(descs), args.rounds, args.warmup, download=False)
    out["resize_224"] = res
    out["resize_224_scales_picked"] = picked
    out["resize_224_total_draft_over_full"] = ratios(res, "prescale=False", "total")["draft=True"]
    out["resize_224_back_end_draft_over_full"] = ratios(res, "prescale=False", "back_end")["draft=True"]
    for b in batches.values():
        b.destroy()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
