#!/usr/bin/env python3
"""make_libjpeg_fixtures.py -- records tests/golden/libjpeg/: small JPEG files written by Pillow and Pillow's own decode of each.

    python tools/make_libjpeg_fixtures.py            # rewrites the directory (needs Pillow; the tests do not)

Pillow decodes with libjpeg(-turbo)'s defaults -- jpeg_idct_islow, fancy upsampling, the JFIF colour tables -- which is the picture
PJD_F_LIBJPEG promises byte for byte (include/pjd.h).  Per case: <name>.jpg, <name>.rgb (H x W x 3 bytes, tight; a greyscale file's
three equal channels) and an entry of manifest.json, which also names the Pillow version that recorded them.  Pictures are seeded
noise over gradients and hard colour edges, so that every chroma neighbour differs and both rounding directions occur.
"""
import io
import json
import os
import zlib

import numpy as np
from PIL import Image, __version__ as PIL_VERSION

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "libjpeg")

# name: (width, height, subsampling or None for greyscale, quality, extra save options)
CASES = {
    "lj_8x8_444_q90": (8, 8, "4:4:4", 90, {}),
    "lj_16x16_420_q50": (16, 16, "4:2:0", 50, {}),
    "lj_17x17_420_q90": (17, 17, "4:2:0", 90, {}),
    "lj_17x17_420_q100": (17, 17, "4:2:0", 100, {}),
    "lj_33x31_420_q100": (33, 31, "4:2:0", 100, {}),
    "lj_33x31_420_q50": (33, 31, "4:2:0", 50, {}),
    "lj_40x24_422_q90": (40, 24, "4:2:2", 90, {}),
    "lj_61x45_grey_q50": (61, 45, None, 50, {}),
    "lj_3x5_420_q90": (3, 5, "4:2:0", 90, {}),
    "lj_3x5_422_q90": (3, 5, "4:2:2", 90, {}),
    "lj_4x9_420_q90": (4, 9, "4:2:0", 90, {}),
    "lj_4x9_422_q90": (4, 9, "4:2:2", 90, {}),
    "lj_5x4_420_q90": (5, 4, "4:2:0", 90, {}),
    "lj_5x4_422_q90": (5, 4, "4:2:2", 90, {}),
    "lj_136x72_420_q90": (136, 72, "4:2:0", 90, {}),
    "lj_136x72_420_q90_rst4": (136, 72, "4:2:0", 90, {"restart_marker_blocks": 4}),
    "lj_33x31_420_q90_prog": (33, 31, "4:2:0", 90, {"progressive": True}),
}


def picture(name, w, h, grey):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 128 + 127 * np.sin(x / 3.0) * np.cos(y / 2.0)], axis=2)
    base[(x.astype(int) // 5 + y.astype(int) // 3) % 2 == 1] = (base[(x.astype(int) // 5 + y.astype(int) // 3) % 2 == 1] + (90, 170, 40)) % 256
    img = np.clip(base + rng.normal(0, 18, (h, w, 3)), 0, 255).astype(np.uint8)
    return img[:, :, 0] if grey else img


def main():
    os.makedirs(OUT, exist_ok=True)
    manifest = {"pillow": PIL_VERSION, "cases": {}}
    for name, (w, h, sub, q, extra) in CASES.items():
        src = picture(name, w, h, sub is None)
        buf = io.BytesIO()
        opts = dict(quality=q, **extra)
        if sub is not None:
            opts["subsampling"] = sub
        Image.fromarray(src).save(buf, "JPEG", **opts)
        data = buf.getvalue()
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert rgb.shape == (h, w, 3)
        open(os.path.join(OUT, name + ".jpg"), "wb").write(data)
        open(os.path.join(OUT, name + ".rgb"), "wb").write(rgb.tobytes())
        manifest["cases"][name] = {"width": w, "height": h, "sampling": sub or "grey", "quality": q, "progressive": bool(extra.get("progressive")),
                                   "restart_marker_blocks": int(extra.get("restart_marker_blocks", 0))}
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    print(f"{len(CASES)} cases -> {OUT} (Pillow {PIL_VERSION})")


if __name__ == "__main__":
    main()
