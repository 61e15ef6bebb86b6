#!/usr/bin/env python3
"""Generate tests/golden/tensor_plan_calls.json: what the four public helpers of pjd_amd.tensors hand to a batch, over a matrix of their
keywords, as one digest per case.  No GPU and no library: a stand-in context, a stand-in Batch that records its calls, and torch on the
CPU for the result tensors.  Only public names of pjd_amd.tensors are used (and the module's `_torch` hook, replaced by a stand-in as
tests/test_resize_aa_cpu.py replaces it), so the script runs unchanged on any later version of the module:
tests/test_tensor_plan_cpu.py replays the matrix and compares.  The file is a record of the past: regenerate it only from a commit whose
behaviour is the wanted one, never from the code under test.     python tests/golden/make_tensor_plan_calls.py

Per case: the width, height and flags of the descriptors given to ctx.batch, the output format, every Batch call in order with its
arguments (windows as ResizeWindow field tuples, numpy arrays as dtype plus values, bind_output without the address), the shape, strides
and dtype of the result, the statuses, and the caller's descriptor flags afterwards; for a refused case the exception type and the fact
that no batch was created.  One line per case: [the case's keywords, true where it succeeds, sha256[:16] of the record]."""
import hashlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tensor_plan_calls.json")

SIZE = (56, 40)                                              # (H, W)
RESIZE_SHORT = 64                                            # at least both sides of SIZE: the centre crop always fits
PICTURES = [(1200, 900, 0), (333, 480, 1), (48, 40, 0), (640, 481, 0)]     # (w, h, flags); 1 = F_STANDARD_RESTART, outside the scale masks
VIEWS = [0, 2, 0, 3, 2]                                      # pictures 0 and 2 twice, picture 1 unused
ORIENTATIONS = {"none": None, "rot": (1, 3, 6, 8), "mirror": (2, 4, 5, 7)}
# the keywords of the two resizing helpers whose every combination is a case ...
PLAN = {"o": list(ORIENTATIONS), "c": ["none", "some", "all"], "f": ["none", "mixed"], "rs": ["none", "64"],
        "lb": ["none", "center", "topleft"], "ps": ["off", "box", "libjpeg", "draft"], "v": ["none", "views"]}
# ... and the ones that only ride along: two of their valid combinations per case
TAIL = {"fn": ["resized", "f16", "bf16", "f32"], "flt": ["bilinear", "antialias", "bicubic"], "g": ["0", "1"], "cl": ["0", "1"], "pv": ["0", "1"]}
REFUSALS = ["letterbox_crop_shape", "letterbox_resize_short", "letterbox_mode"]     # each must occur in a failing case


def _tails():
    out = []
    for g in TAIL["g"]:
        for flt in TAIL["flt"]:
            for fn, cl, pv in (("resized", "0", "0"), ("f16", "0", "0"), ("bf16", "0", "0"), ("f32", "0", "0"), ("f32", "0", "1"),
                               ("f16", "1", "0"), ("bf16", "1", "1")):
                if not (g == "1" and cl == "1"):             # one plane has no interleaved form: that refusal is an extra case
                    out.append({"fn": fn, "flt": flt, "g": g, "cl": cl, "pv": pv})
    return out


def cases():
    """The matrix -> list of dicts of symbolic keywords (strings), in a fixed order."""
    out, tails, i = [], _tails(), 0
    for o in PLAN["o"]:
        for c in PLAN["c"]:
            for f in PLAN["f"]:
                for rs in PLAN["rs"]:
                    for lb in PLAN["lb"]:
                        for ps in PLAN["ps"]:
                            for v in PLAN["v"]:
                                t = (i * 7 + i // len(tails)) % len(tails)
                                for tail in (tails[t], tails[(t + 17) % len(tails)]):
                                    kw = {"o": o, "c": c, "f": f, "rs": rs, "lb": lb, "ps": ps, "v": v}
                                    kw.update(tail)
                                    if lb == "none":
                                        kw["pv"] = "0"       # without a letterbox pad_value is refused: an extra case
                                    out.append(kw)
                                i += 1
    for name in EXTRAS:
        for fn in ("resized", "f32"):
            out.append({"fn": fn, "extra": name})
    for planar in ("1", "0"):
        for o in PLAN["o"]:
            for mode in ("off", "libjpeg", "draft2", "draft4", "draft8"):
                for g in ("0", "1"):
                    out.append({"fn": "tensors", "planar": planar, "o": o, "ps": mode, "g": g})
    for mode in ("off", "libjpeg"):
        for g in ("0", "1"):
            out.append({"fn": "batch", "ps": mode, "g": g})
    out.append({"fn": "batch", "ps": "off", "g": "0", "extra": "ragged"})
    out.append({"fn": "tensors", "planar": "1", "o": "none", "ps": "off", "g": "0", "extra": "draft_without_libjpeg"})
    out.append({"fn": "tensors", "planar": "1", "o": "none", "ps": "libjpeg", "g": "0", "extra": "draft_3"})
    out.append({"fn": "tensors", "planar": "1", "o": "rot", "ps": "off", "g": "0", "extra": "orientations_length"})
    return out


# a named departure from the case BASE: a function of the keyword dict of the call, which it edits
BASE = {"o": "rot", "c": "all", "f": "mixed", "rs": "none", "lb": "center", "ps": "off", "v": "none", "flt": "bilinear", "g": "0", "cl": "0", "pv": "0"}
EXTRAS = {
    "letterbox_crop_shape": lambda k: k.update(crops=[(0, 0, 5, 0)] + k["crops"][1:]),
    "letterbox_crop_length": lambda k: k.update(crops=[(0, 0, 5)] + k["crops"][1:]),
    "letterbox_resize_short": lambda k: k.update(crops=None, resize_short=RESIZE_SHORT),
    "letterbox_mode": lambda k: k.update(letterbox="middle"),
    "letterbox_crop_outside": lambda k: k.update(crops=[(0, 0, 1201, 10)] + k["crops"][1:]),
    "crops_length": lambda k: k.update(crops=k["crops"][:3]),
    "flips_length": lambda k: k.update(flips=k["flips"] + [True]),
    "orientations_length": lambda k: k.update(orientations=k["orientations"][:2]),
    "orientation_9": lambda k: k.update(orientations=[9] + k["orientations"][1:]),
    "crop_outside": lambda k: k.update(letterbox=None, crops=[(1195, 0, 10, 10)] + k["crops"][1:]),
    "crop_outside_no_orientations": lambda k: k.update(letterbox=None, orientations=None, crops=[(1195, 0, 10, 10)] + k["crops"][1:]),
    "crops_and_resize_short": lambda k: k.update(letterbox=None, resize_short=RESIZE_SHORT),
    "resize_short_too_small": lambda k: k.update(letterbox=None, crops=None, resize_short=39),
    "flips_length_no_orientations": lambda k: k.update(letterbox=None, orientations=None, crops=None, flips=[True]),
    "pad_value_without_letterbox": lambda k: k.update(letterbox=None, pad_value=0.0),
    "gray_channels_last": lambda k: k.update(gray=True, channels_last=True),
    "libjpeg_with_prescale": lambda k: k.update(libjpeg=True, prescale=True),
    "draft_without_libjpeg": lambda k: k.update(draft=True),
    "interpolation": lambda k: k.update(interpolation="nearest"),
    "fill": lambda k: k.update(fill=(0, 0, 256)),
    "views_empty": lambda k: k.update(views=[]),
    "views_outside": lambda k: k.update(views=[0, 4, 1, 2]),
    "no_pictures": lambda k: k.update(descs=[]),
    # these succeed: corners of the keywords that the product above does not reach
    "flips_all_false": lambda k: k.update(letterbox=None, orientations=None, crops=None, flips=[False] * 4),
    "flips_all_false_letterbox": lambda k: k.update(orientations=None, crops=None, flips=[False] * 4),
    "flips_all_false_orientations": lambda k: k.update(letterbox=None, crops=None, flips=[False] * 4),
    "crops_all_none": lambda k: k.update(letterbox=None, orientations=None, flips=None, crops=[None] * 4),
    "own_scale_flags": lambda k: [setattr(d, "flags", int(d.flags) | 32) for d in k["descs"]],       # F_SCALE_1_4 with prescale=False
    "own_scale_flags_no_orientations": lambda k: ([setattr(d, "flags", int(d.flags) | 16) for d in k["descs"]], k.update(letterbox=None, orientations=None, crops=[(10, 20, 30, 15)] * 4)),
    "full_picture_crop": lambda k: k.update(letterbox=None, orientations=None, flips=None, crops=[(0, 0, 1200, 900), None, None, None], prescale=True),
    "fill_and_pad_value": lambda k: k.update(fill=(114, 115, 116), pad_value=(0.5, -1, 2)),
    "gray_scalars": lambda k: k.update(gray=True, fill=114, mean=0.5, std=[0.25], pad_value=0),
}


def _descs(pictures=PICTURES):
    import pjd_amd
    out = []
    for w, h, flags in pictures:
        d = pjd_amd.ImageDesc()
        d.width, d.height, d.flags = w, h, flags
        out.append(d)
    return out


def _crop(k, uw, uh):
    """Crop k of an upright uw x uh picture: inside it, different for every k, k == 2 the whole picture."""
    if k == 2:
        return (0, 0, uw, uh)
    x, y = uw * (k + 1) // 9, uh * (k + 2) // 11
    return (x, y, max(1, (uw - x) * (2 + k % 3) // 5), max(1, (uh - y) * (3 - k % 3) // 4))


def _resize_keywords(kw):
    """The keywords of a call of a resizing helper for the symbolic case kw."""
    kw = dict(BASE, **kw) if "extra" in kw else kw
    pics = VIEWS if kw["v"] == "views" else list(range(len(PICTURES)))
    oris = ORIENTATIONS[kw["o"]]
    oris = None if oris is None else [oris[k % 4] for k in range(len(pics))]
    k = {"descs": _descs(), "size": SIZE}
    if kw["v"] == "views":
        k["views"] = list(VIEWS)
    if oris is not None:
        k["orientations"] = oris
    if kw["c"] != "none":
        crops = []
        for n, p in enumerate(pics):
            w, h, _ = PICTURES[p]
            uw, uh = (h, w) if oris is not None and oris[n] >= 5 else (w, h)
            crops.append(None if kw["c"] == "some" and n % 2 else _crop(n, uw, uh))
        k["crops"] = crops
    if kw["f"] != "none":
        k["flips"] = [n % 3 != 1 for n in range(len(pics))]
    if kw["rs"] != "none":
        k["resize_short"] = RESIZE_SHORT
    if kw["lb"] != "none":
        k["letterbox"] = kw["lb"]
        k["fill"] = (114, 7, 201)
    k["prescale"] = kw["ps"] == "box"
    if kw["ps"] in ("libjpeg", "draft"):
        k["libjpeg"] = True
    if kw["ps"] == "draft":
        k["draft"] = True
    if kw["flt"] == "antialias":
        k["antialias"] = True
    if kw["flt"] == "bicubic":
        k["interpolation"] = "bicubic"
        k["antialias"] = kw["o"] == "rot"                    # not consulted
    if kw["g"] == "1":
        k["gray"] = True
    k["mean"], k["std"] = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    if kw["cl"] == "1":
        k["channels_last"] = True
    if kw["pv"] == "1":
        k["pad_value"] = (0.0, -1.5, 2.0) if kw["g"] == "0" else 0.25
    if "extra" in kw:
        EXTRAS[kw["extra"]](k)
    if kw["fn"] == "resized":                                # the keywords only the normalised helper has
        for name in ("mean", "std", "channels_last", "pad_value"):
            k.pop(name, None)
    return k


class _Batch:
    """Stands in for a Batch: records every call, and answers packed_size / output_offset as a packed batch of its sizes would."""
    def __init__(self, descs, fmt, rec):
        from pjd_amd import tensors
        self.n, self.rec = len(descs), rec
        self.nc = 1 if fmt == 4 else 3
        self.sizes = [tensors.output_hw(d) for d in descs]
        self.es = 1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.rec["calls"].append(["close"])

    def _offsets(self):
        offs = [0]
        for h, w in self.sizes:
            offs.append(offs[-1] + self.nc * h * w * self.es)
        return offs

    def __getattr__(self, name):
        def call(*a, **k):
            assert not k, (name, k)
            import pjd_amd
            args = list(a)
            if name == "set_resize":
                self.sizes = [tuple(s) for s in a[0]]
            elif name == "set_normalize":
                self.es = {pjd_amd.DT_F16: 2, pjd_amd.DT_BF16: 2, pjd_amd.DT_F32: 4}[a[0]]
            elif name == "set_resize_window":
                recs = [None if w is None else pjd_amd.resize_window(w) for w in a[0]]
                args = [[None if r is None else [getattr(r, f) for f, _ in pjd_amd.ResizeWindow._fields_] for r in recs]]
            elif name == "bind_output":
                args = args[1:]                              # without the address
            self.rec["calls"].append([name] + [_plain(v) for v in args])
            if name == "packed_size":
                return self._offsets()[-1]
            if name == "output_offset":
                return self._offsets()[a[0]]
            if name == "statuses":
                return list(range(self.n))
        return call


def _plain(v):
    """A call argument as JSON can hold it."""
    import numpy as np
    if isinstance(v, np.ndarray):
        return ["ndarray", str(v.dtype), v.tolist()]
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def run_case(kw):
    """One case against the module as it is now -> its record (a dict that JSON can hold)."""
    import torch
    import pjd_amd
    from pjd_amd import tensors
    fake = types.SimpleNamespace(device=lambda *a: "cpu", float16=torch.float16, bfloat16=torch.bfloat16, float32=torch.float32, uint8=torch.uint8,
                                 empty=lambda n, dtype, device: torch.zeros(n, dtype=dtype),
                                 cuda=types.SimpleNamespace(current_stream=lambda d: types.SimpleNamespace(synchronize=lambda: rec["calls"].append(["drain"]))))
    rec = {"calls": [], "batches": []}

    def batch(descs, fmt):
        rec["batches"].append({"descs": [[int(d.width), int(d.height), int(d.flags)] for d in descs], "format": int(fmt)})
        return _Batch(descs, fmt, rec)

    ctx = types.SimpleNamespace(device=0, batch=batch)
    if kw["fn"] == "tensors":
        k = {"descs": _descs(), "planar": kw["planar"] == "1", "gray": kw["g"] == "1", "libjpeg": kw["ps"] != "off"}
        if kw["ps"].startswith("draft"):
            k["draft"] = int(kw["ps"][5:])
        if ORIENTATIONS[kw["o"]] is not None:
            k["orientations"] = list(ORIENTATIONS[kw["o"]])
        {"draft_without_libjpeg": lambda: k.update(draft=2), "draft_3": lambda: k.update(draft=3),
         "orientations_length": lambda: k.update(orientations=[1, 6]), None: lambda: None}[kw.get("extra")]()
        fn = tensors.decode_to_tensors
    elif kw["fn"] == "batch":
        k = {"descs": _descs([(640, 481, 1)] * 3 + ([(640, 480, 0)] if kw.get("extra") == "ragged" else [])), "gray": kw["g"] == "1", "libjpeg": kw["ps"] != "off"}
        fn = tensors.decode_to_batch_tensor
    else:
        k = _resize_keywords(kw)
        fn = tensors.decode_resized_batch_tensor if kw["fn"] == "resized" else tensors.decode_normalized_batch_tensor
        if kw["fn"] != "resized":
            k["dtype"] = {"f16": None, "bf16": torch.bfloat16, "f32": torch.float32}[kw["fn"]]
    descs = k.pop("descs")
    args = [k.pop(a) for a in ("size", "mean", "std") if a in k]
    real, tensors._torch = tensors._torch, lambda: fake
    try:
        out, st = fn(ctx, descs, *args, **k)
    except Exception as e:                                   # a refusal: its type, and that nothing was created or called
        return {"raises": type(e).__name__, "calls": rec["calls"], "batches": rec["batches"]}
    finally:
        tensors._torch = real
    outs = out if isinstance(out, list) else [out]
    rec["result"] = [[list(t.shape), list(t.stride()), str(t.dtype)] for t in outs]
    rec["statuses"] = _plain(st)
    rec["flags_after"] = [int(d.flags) for d in descs]
    return rec


def key(kw):
    return " ".join(f"{k}={v}" for k, v in kw.items())


def digest(rec):
    return hashlib.sha256(json.dumps(rec, sort_keys=True).encode()).hexdigest()[:16]


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "pim-jpeg-decoder_amd", "python"))
    lines = []
    for kw in cases():
        rec = run_case(kw)
        if "raises" in rec:
            assert rec["raises"] == "ValueError" and not rec["calls"] and not rec["batches"], (key(kw), rec)
        lines.append(json.dumps([key(kw), "raises" not in rec, digest(rec)]))
    with open(OUT, "w") as f:                                # one case per line
        f.write("[\n" + ",\n".join(lines) + "\n]\n")
    ok = sum(json.loads(ln)[1] for ln in lines)
    print(f"{len(lines)} cases, {ok} succeed ({100 * ok // len(lines)} %)")


if __name__ == "__main__":
    main()
