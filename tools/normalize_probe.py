"""What normalised float output costs: the default bench workload (1024 ragged pictures, box pre-scale, 224 x 224) as uint8, fp16, bf16
and fp32 tensors, and the two-step route (uint8 resize, then torch's conversion) the fused epilogue replaces.

    python tools/normalize_probe.py [--rounds 60] [--warmup 5] [--size 224] [--u8-only]

Prints one JSON line:
  resize     per output type (u8, f16, bf16, f32 planar; f16 interleaved) the median, minimum, maximum and the 10th..90th percentile
             spread of the `resize` launch from pjd_batch_decode_timed, the batches resident on one context and decoded in alternation;
             the bytes the launch has to move, computed from the shapes (the source footprint read once + the output written once), what
             that is in GB/s and as a share of the 6.3 TB/s a plain copy reaches; the sum of the other kernels of the decode
  two_step   HIP events on ONE stream (the library's, which torch wraps as an external stream): the conversion of the uint8 tensor
             [N, 3, H, W] by torch -- `chain`: x.float().div(255).sub(mean).div(std).to(dtype); `mul_add`: x.float().mul_(scale).add_(bias)
             .to(dtype) -- alone, and the whole path decode -> tensor for the two-step and the fused route, alternating
  device_bytes of the normalised batches, unbound and bound
--u8-only: the uint8 batch alone (also runs on a tree from before pjd_batch_set_normalize: the same figure at the parent commit).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.3e12          # bytes/s a plain device copy reaches on an MI355X (read + write counted)


def stat(v):
    s = sorted(v)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "p10_ms": round(s[len(s) // 10], 4), "p90_ms": round(s[(9 * len(s)) // 10], 4), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--u8-only", action="store_true")
    args = ap.parse_args()
    # before anything loads libpjd.so: torch and the library then share one HIP runtime (pjd_amd/tensors.py)
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
    import pjd_amd
    import bench
    from pjd_amd import tensors
    jpegs, label = bench.make_workload("cfg3", args.images, 3, 8192, 0)      # bench.py's default workload, rank 0's seed
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    T = args.size
    descs = tensors.prescaled_descs([s.desc for s in scanned], (T, T))
    n = len(descs)
    src_bytes = sum(3 * tensors.output_hw(d)[0] * tensors.output_hw(d)[1] for d in descs)
    ctx = pjd_amd.Context(0)
    out = {"probe": "normalize", "workload": label, "size": T, "rounds": args.rounds, "src_bytes": src_bytes, "resize": {}, "two_step": {},
           "device_bytes": {}}
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    kinds = [("u8", pjd_amd.OUT_RGB8_PLANAR, None, 1)]
    if not args.u8_only:
        scale, bias = tensors.normalize_constants(mean, std)
        kinds += [("f16", pjd_amd.OUT_RGB8_PLANAR, pjd_amd.DT_F16, 2), ("bf16", pjd_amd.OUT_RGB8_PLANAR, pjd_amd.DT_BF16, 2),
                  ("f32", pjd_amd.OUT_RGB8_PLANAR, pjd_amd.DT_F32, 4), ("f16_interleaved", pjd_amd.OUT_RGB8, pjd_amd.DT_F16, 2)]

    # ---- (a) the resize launch per output type
    batches = {}
    for key, fmt, dt, es in kinds:
        b = ctx.batch(descs, fmt)
        b.set_resize([(T, T)] * n)
        if dt is not None:
            b.set_normalize(dt, scale, bias)
        out["device_bytes"][key] = b.info()["device_bytes"]
        b.upload()
        batches[key] = (b, es)
    for _ in range(args.warmup):
        for b, _ in batches.values():
            b.decode_timed()
    samples = {k: {"resize": [], "others": []} for k in batches}
    for _ in range(args.rounds):
        for k, (b, _) in batches.items():                                    # alternation: clock and cache state are shared out evenly
            per, total = b.decode_timed()
            samples[k]["resize"].append(per["resize"])
            samples[k]["others"].append(sum(v for name, v in per.items() if name != "resize"))
    for k, (b, es) in batches.items():
        b.sync()
        r = stat(samples[k]["resize"])
        moved = src_bytes + n * 3 * T * T * es
        r.update({"dst_bytes": n * 3 * T * T * es, "moved_bytes": moved, "gb_per_s": round(moved / (r["median_ms"] * 1e-3) / 1e9, 1),
                  "share_of_copy_rate": round(moved / (r["median_ms"] * 1e-3) / COPY_RATE, 3),
                  "other_kernels": stat(samples[k]["others"]), "n_fallback": b.info()["n_fallback"]})
        out["resize"][k] = r
        b.destroy()

    if not args.u8_only:
        # ---- (d) memory, bound
        for key, fmt, dt, es in kinds[1:]:
            b = ctx.batch(descs, fmt)
            b.set_resize([(T, T)] * n)
            b.set_normalize(dt, scale, bias)
            buf = torch.empty(n * 3 * T * T * es, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), buf.numel(), [i * 3 * T * T * es for i in range(n)])
            out["device_bytes"][key + "_bound"] = b.info()["device_bytes"]
            b.destroy()
            del buf

        # ---- (c) the two-step route against the fused one, events on the library's stream
        lib_stream = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
        u8 = torch.empty(n, 3, T, T, dtype=torch.uint8, device="cuda:0")
        bu = ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR)
        bu.set_resize([(T, T)] * n)
        bu.bind_output(u8.data_ptr(), u8.numel(), [i * 3 * T * T for i in range(n)])
        bu.upload(); bu.capture(); bu.decode(); bu.sync()
        mean_t = torch.tensor(mean, device="cuda:0").view(1, 3, 1, 1)
        std_t = torch.tensor(std, device="cuda:0").view(1, 3, 1, 1)
        scale_t = torch.tensor(scale, device="cuda:0").view(1, 3, 1, 1)
        bias_t = torch.tensor(bias, device="cuda:0").view(1, 3, 1, 1)
        forms = {"chain": lambda x, dt: x.float().div(255).sub(mean_t).div(std_t).to(dt),
                 "mul_add": lambda x, dt: x.float().mul_(scale_t).add_(bias_t).to(dt)}
        for name, tdt, dt, es in (("f16", torch.float16, pjd_amd.DT_F16, 2), ("bf16", torch.bfloat16, pjd_amd.DT_BF16, 2), ("f32", torch.float32, pjd_amd.DT_F32, 4)):
            res = torch.empty(n, 3, T, T, dtype=tdt, device="cuda:0")
            bf = ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR)
            bf.set_resize([(T, T)] * n)
            bf.set_normalize(dt, scale, bias)
            bf.bind_output(res.data_ptr(), res.numel() * es, [i * 3 * T * T * es for i in range(n)])
            bf.upload(); bf.capture(); bf.decode(); bf.sync()
            times = {"fused_whole": [], **{f"{f}_convert": [] for f in forms}, **{f"{f}_whole": [] for f in forms}}
            with torch.cuda.stream(lib_stream):
                for rnd in range(args.warmup + args.rounds):
                    # every item alone on the device (its batch settled before the next starts): the library then issues each decode
                    # the same way, and the items alternate within a round
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 + 3 * len(forms))]
                    ev[0].record(lib_stream); bf.decode(); ev[1].record(lib_stream)
                    lib_stream.synchronize(); bf.sync()
                    k = 2
                    for f in forms.values():
                        ev[k].record(lib_stream); bu.decode(); ev[k + 1].record(lib_stream)
                        y = f(u8, tdt)
                        ev[k + 2].record(lib_stream)
                        lib_stream.synchronize(); bu.sync()
                        k += 3
                    if rnd < args.warmup:
                        continue
                    times["fused_whole"].append(ev[0].elapsed_time(ev[1]))
                    k = 2
                    for fname in forms:
                        times[f"{fname}_convert"].append(ev[k + 1].elapsed_time(ev[k + 2]))
                        times[f"{fname}_whole"].append(ev[k].elapsed_time(ev[k + 2]))
                        k += 3
                del y
            out["two_step"][name] = {k: stat(v) for k, v in times.items()}
            out["two_step"][name]["u8_resize_plus_chain_ms"] = round(out["resize"]["u8"]["median_ms"] + out["two_step"][name]["chain_convert"]["median_ms"], 4)
            out["two_step"][name]["u8_resize_plus_mul_add_ms"] = round(out["resize"]["u8"]["median_ms"] + out["two_step"][name]["mul_add_convert"]["median_ms"], 4)
            out["two_step"][name]["fused_resize_ms"] = out["resize"][name]["median_ms"]
            bf.destroy()
            del res
        bu.destroy()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
