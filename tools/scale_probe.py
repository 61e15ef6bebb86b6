#!/usr/bin/env python3
"""scale_probe.py -- reduced-size output (PJD_F_SCALE_*) on the default workload of bench.py: one JSON line.

    python tools/scale_probe.py [--steps K] [--e2e-batches B] [--device D]

The cfg3 batch is generated exactly as bench.py generates it (tools/libjpegsynth.so, seed 3, picture 0 = the bundled ImageNet
sample re-encoded).  Parity first: picture 0 and a 64-picture sample are decoded at s = 1, 2, 4, 8 and compared with the box filter
of the full-size decode (include/pjd.h); any mismatch exits with status 1 before anything is timed.  Then, per scale (every picture
of the batch at that scale):
    resident        per-kernel milliseconds of pjd_batch_decode_timed (median of K) and the steady rate of SOURCE pixels with one
                    batch, captured graph replayed K times
    pcie_inclusive  source pixels per second and out_bytes through the pipelined batcher (pipe_run, image_flags = the scale),
                    BMP output, 3 slots -- as bench.py --full measures it at s = 1
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                   # noqa: E402  (workload generator and paths, nothing is run)
import numpy as np                             # noqa: E402
import pjd_amd                                 # noqa: E402

FLAGS = {1: 0, 2: pjd_amd.F_SCALE_1_2, 4: pjd_amd.F_SCALE_1_4, 8: pjd_amd.F_SCALE_1_8}


def box(rgb, s):
    if s == 1:
        return rgb
    h, w, _ = rgb.shape
    sh, sw = -(-h // s), -(-w // s)
    acc = np.zeros((sh * s, sw * s, 3), np.int64)
    acc[:h, :w] = rgb
    cnt = np.zeros((sh * s, sw * s), np.int64)
    cnt[:h, :w] = 1
    n = cnt.reshape(sh, s, sw, s).sum(axis=(1, 3))[..., None]
    return ((acc.reshape(sh, s, sw, s, 3).sum(axis=(1, 3)) + (n >> 1)) // n).astype(np.uint8)


def descs(scanned, s):
    """copies of the scanned descriptors (their bitstreams stay owned by `scanned`) with the scale flag of s"""
    out = []
    for x in scanned:
        d = pjd_amd.ImageDesc()
        C.memmove(C.byref(d), C.byref(x.desc), C.sizeof(pjd_amd.ImageDesc))
        d.flags = int(d.flags) | FLAGS[s]
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--e2e-batches", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    jpegs, label = bench.make_workload("cfg3", 1024, 3, 0, a.device)
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    assert all(x.valid for x in scanned)
    ctx = pjd_amd.Context(a.device)
    line = {"probe": "scale_probe", "workload": label, "images": len(jpegs)}

    # ---- parity first ---------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(11)
    sample = sorted({0} | set(int(i) for i in rng.choice(len(jpegs), 64, replace=False)))
    full, st_full = ctx.decode([scanned[i].desc for i in sample], pjd_amd.OUT_RGB8)
    bad = []
    for s in (2, 4, 8):
        sub = [scanned[i] for i in sample]
        outs, st = ctx.decode(descs(sub, s), pjd_amd.OUT_RGB8)
        bad += [(s, sample[k]) for k in range(len(sample)) if st[k] != st_full[k] or not np.array_equal(outs[k], box(full[k], s))]
    line["parity"] = {"pictures": len(sample), "scales": [2, 4, 8], "mismatches": len(bad)}
    if bad:
        line["parity"]["first"] = bad[:8]
        print(json.dumps(line))
        sys.exit(1)

    # ---- resident: kernels and one-batch rate -----------------------------------------------------------------------------------
    res = {}
    for s in (1, 2, 4, 8):
        with ctx.batch(descs(scanned, s), pjd_amd.OUT_RGB8) as b:
            b.upload()
            b.decode(); b.sync()
            kts = []
            for _ in range(a.steps):
                kt, tot = b.decode_timed()
                kts.append((kt, tot))
            b.sync()
            b.capture()
            for _ in range(3):
                b.decode()
            b.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                b.decode()
                b.sync()
            dt = (time.perf_counter() - t0) / a.steps
            info = b.info()
        names = kts[0][0].keys()
        res[str(s)] = {"kernels_ms": {k: round(statistics.median(x[0][k] for x in kts), 4) for k in names},
                       "timed_total_ms": round(statistics.median(x[1] for x in kts), 4),
                       "ms_per_batch": round(dt * 1e3, 4), "GPix_s": round(info["pixels"] / dt / 1e9, 2),
                       "out_bytes": info["out_bytes"], "n_fallback": info["n_fallback"]}
    line["resident"] = res

    # ---- PCIe-inclusive ---------------------------------------------------------------------------------------------------------
    pcie = {}
    pjd_amd.pipe_run(jpegs=jpegs * 4, batch_images=len(jpegs), scan_threads=8, slots=3, sink=None, device=a.device)
    for s in (1, 2, 4, 8):
        ps = pjd_amd.pipe_run(jpegs=jpegs * a.e2e_batches, batch_images=len(jpegs), scan_threads=8, slots=3, sink=None,
                              device=a.device, image_flags=FLAGS[s])
        pcie[str(s)] = {"GPix_s": round(ps["pixels"] / ps["wall_s"] / 1e9, 2), "out_bytes": ps["out_bytes"],
                        "d2h_GBps": round(ps["out_bytes"] / ps["wall_s"] / 1e9, 2), "wall_ms": round(ps["wall_s"] * 1e3, 1),
                        "batches": ps["n_batches"], "failures": ps["n_batch_failures"]}
    pjd_amd.pipe_release()
    line["pcie_inclusive"] = pcie
    ctx.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
