"""What views save: the default bench workload with V resampled outputs per picture, once as ONE batch of N pictures with V * N views
(pjd_batch_set_views) and once the only way there was before -- the batch that holds every descriptor V times.  Both deliver the same
V * N planar 8-bit pictures into caller-owned device memory (a torch buffer, bound), each a RandomResizedCrop window of its picture with
a flip, bilinear; the repeated batch's outputs are compared byte for byte with the views batch's before anything is timed.  The two
batches are resident on one context and decoded in alternation.  Prints one JSON line: per configuration (2 views of 224 x 224; 2 of
224 x 224 + 8 of 96 x 96) and per batch kind the median, minimum and maximum over the rounds of the HIP-event time of a decode
(pjd_batch_decode_timed: one chain of launches), of its "resize" launch alone and of every other launch, of the host clock around
pjd_batch_decode + pjd_batch_sync (the form a caller runs), and device_bytes, n_subsequences, n_data_units and out_bytes.

    python tools/views_probe.py [--rounds 30] [--warmup 3] [--images 1024]
"""
import torch                                                      # first: torch and libpjd.so then use one HIP runtime (pjd_amd.tensors)

import argparse                                                   # noqa: E402
import json                                                       # noqa: E402
import os                                                         # noqa: E402
import random                                                     # noqa: E402
import math                                                       # noqa: E402
import statistics                                                 # noqa: E402
import sys                                                        # noqa: E402
import time                                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_resized_crop(rng, w, h, scale, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision's RandomResizedCrop.get_params with a seeded generator of our own -> (x, y, w, h)."""
    area = w * h
    for _ in range(10):
        target = area * rng.uniform(*scale)
        ar = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if 0 < cw <= w and 0 < ch <= h:
            return rng.randint(0, w - cw), rng.randint(0, h - ch), cw, ch
    return 0, 0, w, h


def request(descs, per_picture, seed):
    """-> (views, sizes, windows): per_picture = [(target, crop scale range), ...], the views of every picture."""
    rng = random.Random(seed)
    views, sizes, windows = [], [], []
    for p, d in enumerate(descs):
        for t, scale in per_picture:
            x, y, w, h = random_resized_crop(rng, int(d.width), int(d.height), scale)
            views.append(p); sizes.append((t, t))
            windows.append(dict(x=x, y=y, w=w, h=h, flags=rng.randint(0, 1)))
    return views, sizes, windows


def build(pjd_amd, ctx, descs, views, sizes, windows, use_views):
    b = ctx.batch(descs if use_views else [descs[p] for p in views], pjd_amd.OUT_RGB8_PLANAR)
    if use_views:
        b.set_views(views)
    b.set_resize(sizes)
    b.set_resize_window(windows)
    cap = b.packed_size()
    buf = torch.empty(cap, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    torch.cuda.current_stream().synchronize()
    b.bind_output(buf.data_ptr(), cap)
    b.upload()
    return b, buf


def measure(pjd_amd, ctx, descs, per_picture, rounds, warmup, seed):
    views, sizes, windows = request(descs, per_picture, seed)
    kinds = {"views": True, "repeated": False}
    batches = {k: build(pjd_amd, ctx, descs, views, sizes, windows, use) for k, use in kinds.items()}
    out = {"views_per_picture": len(per_picture), "targets": [t for t, _ in per_picture], "n_views": len(views), "kinds": {}}
    for k in kinds:                                                          # the two deliver the same bytes
        batches[k][0].decode(); batches[k][0].sync()
    assert batches["views"][0].packed_size() == batches["repeated"][0].packed_size()
    out["outputs_equal"] = bool(torch.equal(batches["views"][1], batches["repeated"][1]))
    assert out["outputs_equal"], "the views batch and the repeated batch differ"
    for _ in range(warmup):
        for k in kinds:
            batches[k][0].decode_timed(); batches[k][0].sync()
            batches[k][0].decode(); batches[k][0].sync()
    samples = {k: {} for k in kinds}
    for _ in range(rounds):
        for k in kinds:                                                      # alternation: clock and cache state are shared out evenly
            b = batches[k][0]
            per_kernel, total = b.decode_timed()
            b.sync()
            per_kernel["events_total"] = total
            t0 = time.perf_counter()
            b.decode(); b.sync()
            per_kernel["decode_and_sync_host_clock"] = (time.perf_counter() - t0) * 1e3
            for name, ms in per_kernel.items():
                samples[k].setdefault(name, []).append(ms)
    for k in kinds:
        info = batches[k][0].info()
        out["kinds"][k] = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for name, v in samples[k].items()}
        out["kinds"][k].update({key: info[key] for key in ("n_images", "device_bytes", "n_subsequences", "n_data_units", "out_bytes", "n_fallback")})
    med = lambda k, name: out["kinds"][k][name]["median_ms"]
    out["views_over_repeated"] = {name: round(med("views", name) / med("repeated", name), 4) for name in ("events_total", "decode_and_sync_host_clock", "resize")}
    for k in kinds:
        batches[k][0].destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "torch sees no GPU"
    torch.zeros(1, device="cuda:0")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    import bench
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    descs = [s.desc for s in scanned]
    ctx = pjd_amd.Context(0)
    out = {"probe": "views", "workload": label, "rounds": args.rounds}
    glob, local = (224, (0.25, 1.0)), (96, (0.05, 0.25))                    # DINO's multi-crop ranges
    out["two_views"] = measure(pjd_amd, ctx, descs, [(224, (0.08, 1.0))] * 2, args.rounds, args.warmup, 1)
    out["two_plus_eight"] = measure(pjd_amd, ctx, descs, [glob] * 2 + [local] * 8, args.rounds, args.warmup, 2)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
