#!/usr/bin/env python3
"""lane_fill.py -- how full the entropy decoder's waves are (host only: no GPU needed).

    python tools/lane_fill.py [--images 1024] [--seed 3] [--odd-pct 0] [--mcus-x2 N]

Generates the default workload of bench.py (without the bundled picture 0, which only a GPU decode provides), plans it with the
library's planner (pjd_plan_info) in both plan modes and prints lanes, waves, workgroups and the fill lanes / (64 x waves).
pjd_batch_info has no per-picture figures, so wave-bytes (waves x S summed over the pictures: what the passes of the kernel
scale with) come from a model of the planner's rule applied to every picture's ecs_len -- `new` is the rule of pjd_plan.cpp,
`old` the one it replaced -- and the model is checked against the planner's own totals."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

S_MIN, S_MAX, LANES = 128, 1024, 64


def batch_size(descs, mcus_x2):
    total = sum(int(d.ecs_len) for d in descs)
    mcus = sum(((int(d.width) + 8 * d.h_samp - 1) // (8 * d.h_samp)) * ((int(d.height) + 8 * d.v_samp - 1) // (8 * d.v_samp)) for d in descs)
    by_total = S_MAX if total >= (64 << 20) else 512 if total >= (24 << 20) else 256 if total >= (2 << 20) else 128
    by_density = (total * mcus_x2 // 2 // mcus + 63) // 64 * 64 if mcus else 512
    return min(by_total, max(S_MIN, min(S_MAX, by_density)))


def lanes_for(n, s):
    return (n + s - 1) // s if n else 1


def size_old(n, sb):
    n0 = lanes_for(n, sb)
    if n0 <= LANES // 2 or n0 % LANES == 0:
        return sb
    kw = (n0 + LANES // 2) // LANES
    lo, hi = max(sb * 7 // 10 // 64 * 64, S_MIN), min(sb * 29 // 20, S_MAX)
    for s in range(lo, hi + 1, 64):
        if lanes_for(n, s) <= kw * LANES:
            return s
    return sb


def size_new(n, sb, odd_pct=0, step=16, counts=(-1, 0, 1)):
    n0 = lanes_for(n, sb)
    if n0 <= LANES // 2:
        return sb
    kw0 = (n0 + LANES // 2) // LANES
    lo, hi = max(sb * 7 // 10 // step * step, S_MIN), min(sb * 29 // 20, S_MAX) // step * step
    cands = []
    for kw in sorted({max(1, kw0 + c) for c in counts}):
        fit = [s for s in range(lo, hi + 1, step) if lanes_for(n, s) <= kw * LANES]
        if fit:
            s = fit[0]
            w = (lanes_for(n, s) + LANES - 1) // LANES
            cands.append(((w * 100 + (w & 1) * odd_pct) * s, w, s))
    if not cands:
        return sb
    cheapest = min(c[0] for c in cands)
    near = [c for c in cands if c[0] <= cheapest + cheapest // 100]
    pick = max(near, key=lambda c: (not (c[1] & 1), c[2]))
    wb = (n0 + LANES - 1) // LANES
    stay = (wb * 100 + (wb & 1) * odd_pct) * sb
    return pick[2] if pick[0] * 16 <= stay * 15 else sb


def tally(lens, sizes):
    lanes = sum(lanes_for(n, s) for n, s in zip(lens, sizes))
    waves = [(lanes_for(n, s) + LANES - 1) // LANES for n, s in zip(lens, sizes)]
    wave_bytes = sum(w * s for w, s in zip(waves, sizes))
    return {"lanes": lanes, "waves": sum(waves), "lanes_per_wave": lanes / sum(waves), "fill": lanes / (LANES * sum(waves)),
            "wave_bytes_over_ideal": wave_bytes / (sum(lens) / LANES), "mean_S": sum(n * s for n, s in zip(lens, sizes)) / sum(lens),
            "single_wave_workgroups": sum(w & 1 for w in waves), "workgroups": sum((w + 1) // 2 for w in waves)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--odd-pct", type=int, default=0, help="PJD_ODD_WAVE_PCT of the planner and of the model")
    ap.add_argument("--mcus-x2", type=int, default=0, help="PJD_SUB_MCUS_X2 (half-MCUs of stream per lane) for both plan modes; 0: the planner's 12 / 7")
    args = ap.parse_args()
    os.environ["PJD_ODD_WAVE_PCT"] = str(args.odd_pct)
    if args.mcus_x2:
        os.environ["PJD_SUB_MCUS_X2"] = str(args.mcus_x2)
    import pjd_amd
    import synth
    jpegs = synth.cfg3_imagenet_like(args.images, seed=args.seed, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = [s.desc for s in scanned]
    lens = [int(d.ecs_len) for d in descs]
    print(f"{len(descs)} pictures, {sum(lens)} bytes of entropy-coded stream")
    for mode, x2 in (("throughput", 12), ("latency", 7)):
        os.environ["PJD_PLAN_MODE"] = mode
        info = pjd_amd.plan_info(descs)
        sb = batch_size(descs, args.mcus_x2 or x2)
        real = {k: info[k] for k in ("n_subsequences", "n_huff_waves", "n_huff_workgroups", "sub_bytes")}
        print(f"\n{mode} plan, batch size {sb} B: planner {real}, fill {info['n_subsequences'] / (LANES * info['n_huff_waves']):.4f}")
        rows = [("old", [size_old(n, sb) for n in lens]),
                ("kw-1..kw+1, 64-byte steps", [size_new(n, sb, args.odd_pct, 64) for n in lens]),
                ("new (16-byte steps)", [size_new(n, sb, args.odd_pct) for n in lens])]
        for name, sizes in rows:
            t = tally(lens, sizes)
            print(f"  model {name:28s} lanes {t['lanes']:7d} waves {t['waves']:5d} lanes/wave {t['lanes_per_wave']:.1f} fill {t['fill']:.4f} "
                  f"wave-bytes/ideal {t['wave_bytes_over_ideal']:.3f} mean S {t['mean_S']:.0f} workgroups {t['workgroups']} (single-wave {t['single_wave_workgroups']})")
        t = tally(lens, rows[-1][1])
        ok = (t["lanes"], t["waves"], t["workgroups"]) == (real["n_subsequences"], real["n_huff_waves"], real["n_huff_workgroups"])
        print("  model of the new rule == planner:", ok)


if __name__ == "__main__":
    main()
