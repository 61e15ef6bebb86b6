"""What grey output saves: per-kernel times, the packed download and the byte counts of the default bench workload as
PJD_OUT_RGB8_PLANAR and as PJD_OUT_GRAY8, the two batches resident on one context and decoded in alternation with
pjd_batch_decode_timed; then the same for the workload flagged PJD_F_LIBJPEG.  Prints one JSON line: per batch kind the median, minimum
and maximum of every kernel's time and of pjd_batch_download_packed over the rounds, device_bytes and out_bytes, and the grey / planar
ratios of the back end and of the download.

    python tools/gray_probe.py [--rounds 60] [--warmup 5] [--images 1024]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(pjd_amd, ctx, descs, rounds, warmup):
    kinds = {"planar": pjd_amd.OUT_RGB8_PLANAR, "gray": pjd_amd.OUT_GRAY8}
    batches, hosts, out = {}, {}, {"kinds": {}}
    L = pjd_amd.dev_lib()
    for kind, fmt in kinds.items():
        b = ctx.batch(descs, fmt)
        b.upload()
        batches[kind] = b
        hosts[kind] = (L.pjd_host_alloc(b.packed_size()), b.packed_size())
    st = (C.c_int32 * max(len(descs), 1))()

    def download(kind):
        host, size = hosts[kind]
        t0 = time.perf_counter()
        ctx._check(L.pjd_batch_download_packed(batches[kind]._h, host, size, st), "pjd_batch_download_packed")
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        for kind in kinds:
            batches[kind].decode_timed()
            batches[kind].sync()
            download(kind)
    samples = {kind: {} for kind in kinds}
    for _ in range(max(rounds, 50)):
        for kind in kinds:                                                  # alternation: clock and cache state are shared out evenly
            per_kernel, total = batches[kind].decode_timed()
            per_kernel["total"] = total
            batches[kind].sync()                                            # the download below then times the copy alone
            per_kernel["download_packed"] = download(kind)
            for name, ms in per_kernel.items():
                samples[kind].setdefault(name, []).append(ms)
    for kind in kinds:
        info = batches[kind].info()
        out["kinds"][kind] = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                              for name, v in samples[kind].items()}
        out["kinds"][kind].update(device_bytes=info["device_bytes"], out_bytes=info["out_bytes"], packed_bytes=hosts[kind][1],
                                  n_fallback=info["n_fallback"], statuses_nonzero=sum(1 for s in st if s))
        out["pixels"] = info["pixels"]
    back = lambda k: sum(v["median_ms"] for n, v in out["kinds"][k].items() if isinstance(v, dict) and n in ("idct_colour", "idct_std", "colour_std", "idct_gray", "idct_gray_std"))
    out["back_end_ms"] = {k: round(back(k), 4) for k in kinds}
    out["back_end_gray_over_planar"] = round(back("gray") / back("planar"), 4)
    out["download_gray_over_planar"] = round(out["kinds"]["gray"]["download_packed"]["median_ms"] / out["kinds"]["planar"]["download_packed"]["median_ms"], 4)
    for kind in kinds:
        batches[kind].destroy()
        L.pjd_host_free(hosts[kind][0])
    return out


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
    descs = [s.desc for s in scanned]
    ctx = pjd_amd.Context(0)
    out = {"probe": "gray", "workload": label, "rounds": max(args.rounds, 50)}
    out["default"] = measure(pjd_amd, ctx, descs, args.rounds, args.warmup)
    flagged = [d for d in tensors.libjpeg_descs(descs) if pjd_amd.plan_check([d], pjd_amd.OUT_GRAY8)[0] == 0]
    out["libjpeg"] = measure(pjd_amd, ctx, flagged, args.rounds, args.warmup)
    out["libjpeg"]["n_images"] = len(flagged)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
