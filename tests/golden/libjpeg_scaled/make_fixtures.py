#!/usr/bin/env python3
"""make_fixtures.py -- records tests/golden/libjpeg_scaled/: small JPEG files written by Pillow and Pillow's own DRAFT decode of each at
1/1, 1/2, 1/4 and 1/8 -- libjpeg's scale_num / scale_denom, its reduced IDCTs -- as RGB and as "L" (libjpeg's JCS_GRAYSCALE).

    python tests/golden/libjpeg_scaled/make_fixtures.py      # rewrites the directory (needs Pillow; the tests do not)

That is the picture PJD_F_LIBJPEG | PJD_F_LIBJPEG_SCALE_* promises byte for byte (include/pjd.h).  Per case: <name>.jpg, and per scale s
<name>.s<s>.rgb (oh x ow x 3 bytes, tight; a greyscale file's three equal channels) and <name>.s<s>.l8 (oh x ow bytes), ow x oh =
ceil(W / s) x ceil(H / s).  A scale is forced with im.draft(mode, (max(1, W // s), max(1, H // s))), and the generator asserts that the
size came out as ceil(W / s) x ceil(H / s).  Pillow picks the scale by floor division, so a picture with an axis shorter than s cannot be
made to take it (3 x 5 at 1/4, 5 x 4 at 1/8): those scales are listed in the manifest as "model_only" and have no recording; the tests
hold them to the model.  manifest.json also names the Pillow version that recorded the rest.  Pictures are seeded noise over gradients
and hard colour edges (tools/make_libjpeg_fixtures.py's).
"""
import io
import json
import os
import zlib

import numpy as np
from PIL import Image, __version__ as PIL_VERSION

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = (1, 2, 4, 8)

# name: (width, height, subsampling or None for greyscale, quality, extra save options)
CASES = {
    "ls_8x8_444_q90": (8, 8, "4:4:4", 90, {}),
    "ls_16x16_420_q50": (16, 16, "4:2:0", 50, {}),
    "ls_17x17_420_q100": (17, 17, "4:2:0", 100, {}),
    "ls_33x31_420_q90": (33, 31, "4:2:0", 90, {}),
    "ls_40x24_422_q90": (40, 24, "4:2:2", 90, {}),
    "ls_259x19_422_q50": (259, 19, "4:2:2", 50, {}),
    "ls_3x5_420_q90": (3, 5, "4:2:0", 90, {}),
    "ls_3x5_422_q100": (3, 5, "4:2:2", 100, {}),
    "ls_4x9_420_q50": (4, 9, "4:2:0", 50, {}),
    "ls_4x9_422_q90": (4, 9, "4:2:2", 90, {}),
    "ls_5x4_420_q90": (5, 4, "4:2:0", 90, {}),
    "ls_5x4_422_q90": (5, 4, "4:2:2", 90, {}),
    "ls_61x45_grey_q50": (61, 45, None, 50, {}),
    "ls_136x72_420_q90": (136, 72, "4:2:0", 90, {}),
    "ls_136x72_420_q100_rst4": (136, 72, "4:2:0", 100, {"restart_marker_blocks": 4}),
    "ls_33x31_420_q90_prog": (33, 31, "4:2:0", 90, {"progressive": True}),
}


def picture(name, w, h, grey):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 128 + 127 * np.sin(x / 3.0) * np.cos(y / 2.0)], axis=2)
    odd = (x.astype(int) // 5 + y.astype(int) // 3) % 2 == 1
    base[odd] = (base[odd] + (90, 170, 40)) % 256
    img = np.clip(base + rng.normal(0, 18, (h, w, 3)), 0, 255).astype(np.uint8)
    return img[:, :, 0] if grey else img


def draft(data, mode, s):
    """Pillow's decode at 1/s in `mode`, or None where Pillow cannot be made to take the scale."""
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if min(w, h) < s:
        return None
    im.draft(mode, (max(1, w // s), max(1, h // s)))
    assert im.size == (-(-w // s), -(-h // s)), (im.size, w, h, s)
    return np.asarray(im.convert(mode))


def main():
    manifest = {"pillow": PIL_VERSION, "cases": {}}
    n_rec = 0
    for name, (w, h, sub, q, extra) in CASES.items():
        buf = io.BytesIO()
        opts = dict(quality=q, **extra)
        if sub is not None:
            opts["subsampling"] = sub
        Image.fromarray(picture(name, w, h, sub is None)).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        open(os.path.join(HERE, name + ".jpg"), "wb").write(data)
        model_only = []
        for s in SCALES:
            rgb, l8 = draft(data, "RGB", s), draft(data, "L", s)
            if rgb is None:
                model_only.append(s)
                continue
            ow, oh = -(-w // s), -(-h // s)
            assert rgb.shape == (oh, ow, 3) and l8.shape == (oh, ow) and rgb.dtype == l8.dtype == np.uint8
            open(os.path.join(HERE, f"{name}.s{s}.rgb"), "wb").write(rgb.tobytes())
            open(os.path.join(HERE, f"{name}.s{s}.l8"), "wb").write(l8.tobytes())
            n_rec += 1
        manifest["cases"][name] = {"width": w, "height": h, "sampling": sub or "grey", "quality": q, "progressive": bool(extra.get("progressive")),
                                   "restart_marker_blocks": int(extra.get("restart_marker_blocks", 0)), "model_only": model_only}
    json.dump(manifest, open(os.path.join(HERE, "manifest.json"), "w"), indent=1, sort_keys=True)
    print(f"{len(CASES)} files, {n_rec} recorded scales -> {HERE} (Pillow {PIL_VERSION})")


if __name__ == "__main__":
    main()
