#!/usr/bin/env python3
"""make_fixtures.py -- writes tests/golden/libjpeg_progressive/: progressive files under scan scripts no encoder writes, each held to
libjpeg itself.

    python tests/golden/libjpeg_progressive/make_fixtures.py     # rewrites every file here but this one (needs Pillow; the tests do not)

For every member: Pillow encodes a seeded picture as a progressive JPEG; tests/jpeg_progressive.py reads its quantised coefficients
(decode) and writes them again under the member's own COMPLETE script with the file's own quantisers (build).  A member is written
only if (a) Pillow's RGB decode of the new stream equals Pillow's decode of the source file and (b) tests/libjpeg_model.py over
jpeg_progressive.decode of the new stream equals that decode too; a member that fails is named in the manifest under "left_out" and
nothing of it is written.  Committed per member: <name>.jpg, <name>.rgb (Pillow's RGB decode, H x W x 3), <name>.l8 (Pillow's
draft("L") decode, H x W) and its entry in manifest.json (Pillow's version, size, sampling, the script, hashes).

INCOMPLETE lists five members that are also rewritten with their last four scans dropped.  libjpeg smooths such a frame (interblock
smoothing, jdcoefct.c), the model and the library do not: <name>.incomplete.rgb is Pillow's decode of that stream and the manifest
records how many levels it lies from the model ("incomplete").  Those streams are no fixtures of the flag: they document its envelope.
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image, __version__ as PIL_VERSION

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jpeg_progressive as P                       # noqa: E402
import libjpeg_progressive_corpus as LP            # noqa: E402
from jpeg_progressive import S                     # noqa: E402
from progressive_corpus import full_script         # noqa: E402

CS = [0, 1, 2]


def dri_changes(fr):
    """progressive_corpus's prog_420_40x24_dri_changes: the restart interval changes between scans and goes back to 0; a table id is
    redefined between scans"""
    return [S(CS, al=1, ri=3), S(0, 1, 63, 0, 1, ri=5), S(1, 1, 63, 0, 1, ri=2), S(2, 1, 63, 0, 1, ri=0, tid=1), S(0, 1, 63, 1, 0, ri=7, shape="skew"),
            S(1, 1, 63, 1, 0, ri=0), S(2, 1, 63, 1, 0, ri=1, tid=0), S(CS, ah=1, al=0, ri=4)]


SLOT_BANDS = ((1, 47), (48, 48), (49, 49), (50, 50), (51, 51), (52, 52), (53, 63))
SMALL = lambda fr: full_script(fr)

# name -> (width, height, Pillow's subsampling or "L", quality, seed, content, script)
MEMBERS = {
    "lp_136x72_420_q50_skew_ri3": (136, 72, 2, 50, 9801, "detail", lambda fr: full_script(fr, ri=3, shape="skew", tids=(0, 3, 2))),
    "lp_259x19_422_q75_two_bands": (259, 19, 1, 75, 9802, "detail", lambda fr: full_script(fr, bands=((1, 5), (6, 63)))),
    "lp_515x21_422_q85_eob_random": (515, 21, 1, 85, 9803, "detail", lambda fr: full_script(fr, eob=("random", 9803))),
    "lp_40x24_444_q95_dri_changes": (40, 24, 0, 95, 9804, "detail", dri_changes),
    "lp_61x45_420_q90_three_levels": (61, 45, 2, 90, 9805, "detail", lambda fr: full_script(fr, dc_al=2, ac_al=3, shape="long")),
    "lp_33x31_grey_q85": (33, 31, "L", 85, 9806, "detail", lambda fr: full_script(fr, ri=3, shape="skew", tids=(3, 0, 0))),
    "lp_257x19_grey_q85": (257, 19, "L", 85, 9807, "detail", SMALL),
    "lp_6x3_420_q90": (6, 3, 2, 90, 9808, "detail", SMALL),
    "lp_7x2_420_q90": (7, 2, 2, 90, 9809, "detail", SMALL),
    "lp_10x1_420_q90": (10, 1, 2, 90, 9810, "detail", SMALL),
    "lp_6x1_422_q90": (6, 1, 1, 90, 9811, "detail", SMALL),
    "lp_11x2_422_q90": (11, 2, 1, 90, 9812, "detail", SMALL),
    "lp_4x9_420_q90": (4, 9, 2, 90, 9813, "detail", SMALL),
    "lp_4x9_422_q90": (4, 9, 1, 90, 9814, "detail", SMALL),
    "lp_3x5_420_q90": (3, 5, 2, 90, 9815, "detail", SMALL),
    "lp_3x5_422_q90": (3, 5, 1, 90, 9816, "detail", SMALL),
    "lp_sat67x35_420_q100": (67, 35, 2, 100, 9817, "saturating", lambda fr: full_script(fr, ri=2, tids=(1, 2, 3))),
    "lp_136x72_420_q90_slot48_alone": (136, 72, 2, 90, 9818, "detail", lambda fr: full_script(fr, dc_al=0, ac_al=1, bands=SLOT_BANDS)),
}
INCOMPLETE = ["lp_61x45_420_q90_three_levels", "lp_259x19_422_q75_two_bands", "lp_40x24_444_q95_dri_changes", "lp_136x72_420_q50_skew_ri3",
              "lp_33x31_grey_q85"]
DROPPED = 4
SAMPLING = {0: "4:4:4", 1: "4:2:2", 2: "4:2:0", "L": "grey"}


def picture(w, h, seed, content):
    """detail: smooth colour fields under noise strong enough to reach the last zigzag slots; saturating: 0 / 255 noise"""
    rng = np.random.default_rng(seed)
    if content == "saturating":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 - k) for k in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(rgb, sub, quality):
    im = Image.fromarray(rgb)
    buf = io.BytesIO()
    if sub == "L":
        im.convert("L").save(buf, "JPEG", quality=quality, progressive=True)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=sub, progressive=True)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_l8(data):
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert im.mode == "L", im.mode
    return np.asarray(im)


def scan_record(sc):
    """one line of the manifest per scan: the fields of jpeg_progressive.S as compact JSON"""
    return json.dumps(sc._asdict(), separators=(",", ":"))


def main():
    out = {"pillow": PIL_VERSION, "cases": {}, "left_out": {}, "incomplete": {}}
    for name, (w, h, sub, quality, seed, content, script_of) in MEMBERS.items():
        source = encode(picture(w, h, seed, content), sub, quality)
        frame = LP.frame_of_jpeg(source)
        coef = P.decode(source).coef
        script = script_of(frame)
        try:
            data = P.build(frame, coef, script).data
            want = pillow_rgb(source)
            got = pillow_rgb(data)
        except Exception as e:                                         # the writer or Pillow refuses the stream
            out["left_out"][name] = f"refused: {type(e).__name__}: {e}"
            continue
        status, _, model, luma = LP.model_expected(data, LP.frame_of_jpeg(data))
        if not np.array_equal(got, want):
            out["left_out"][name] = "Pillow's decode of the rewritten stream differs from its decode of the source"
            continue
        if status != 0 or not np.array_equal(model, want):
            out["left_out"][name] = "tests/libjpeg_model.py differs from Pillow's decode"
            continue
        l8 = pillow_l8(data)
        assert np.array_equal(l8, luma) and np.array_equal(l8, pillow_l8(source)), name
        files = {name + ".jpg": data, name + ".rgb": want.tobytes(), name + ".l8": l8.tobytes()}
        slots = P.decode(data).coef
        case = {"width": w, "height": h, "sampling": SAMPLING[sub], "quality": quality, "seed": seed, "content": content,
                "n_units": int(slots.shape[0]), "n_scans": len(script), "nonzero_at_slot_48": int((slots[:, 48] != 0).sum()),
                "script": [scan_record(s) for s in script], "sha256": {}}
        if name in INCOMPLETE:
            part = P.build(frame, coef, script[:-DROPPED]).data
            pil = pillow_rgb(part)
            _, _, model, _ = LP.model_expected(part, LP.frame_of_jpeg(part))
            files[name + ".incomplete.rgb"] = pil.tobytes()
            out["incomplete"][name] = {"dropped_scans": DROPPED, "jpg_sha256": LP.sha(part),
                                       "max_diff_pillow_to_model": int(np.abs(pil.astype(int) - model.astype(int)).max())}
        for fn, b in files.items():
            with open(os.path.join(HERE, fn), "wb") as f:
                f.write(b)
            case["sha256"][fn[len(name) + 1:]] = LP.sha(b)
        out["cases"][name] = case
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out['cases'])} members -> {HERE} (Pillow {PIL_VERSION}); left out: {sorted(out['left_out'])}")
    print("incomplete scripts, levels between Pillow and the model:", {n: v["max_diff_pillow_to_model"] for n, v in out["incomplete"].items()})


if __name__ == "__main__":
    main()
