#!/usr/bin/env python3
"""make_fixtures.py -- records tests/golden/libjpeg_gray/<name>.l8: what libjpeg delivers for the files of tests/golden/libjpeg/ with
out_color_space = JCS_GRAYSCALE, i.e. Pillow's draft("L", size) decode of each (H x W bytes, tight rows).

    python tests/golden/libjpeg_gray/make_fixtures.py        # rewrites the .l8 files and manifest.json (needs Pillow; the tests do not)

That picture is libjpeg's own luma plane, NOT a weighted sum of the clamped R, G and B of its colour decode: the generator checks that
it equals the Y plane of draft("YCbCr") byte for byte and records how far convert("L") of the colour decode is from it.
"""
import io
import json
import os

import numpy as np
from PIL import Image, __version__ as PIL_VERSION

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.path.dirname(HERE), "libjpeg")


def draft(data, mode):
    im = Image.open(io.BytesIO(data))
    im.draft(mode, im.size)
    assert im.mode == mode, (im.mode, mode)
    return np.asarray(im)


def main():
    cases = json.load(open(os.path.join(SRC, "manifest.json")))["cases"]
    out = {"pillow": PIL_VERSION, "cases": {}}
    for name, c in sorted(cases.items()):
        data = open(os.path.join(SRC, name + ".jpg"), "rb").read()
        l8 = draft(data, "L")
        assert l8.shape == (c["height"], c["width"]) and l8.dtype == np.uint8
        if c["sampling"] != "grey":
            assert np.array_equal(l8, draft(data, "YCbCr")[:, :, 0]), name
        via_rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB").convert("L"))
        open(os.path.join(HERE, name + ".l8"), "wb").write(l8.tobytes())
        out["cases"][name] = {"width": c["width"], "height": c["height"],
                              "max_diff_to_convert_L": int(np.abs(l8.astype(int) - via_rgb.astype(int)).max())}
    json.dump(out, open(os.path.join(HERE, "manifest.json"), "w"), indent=1, sort_keys=True)
    print(f"{len(cases)} planes -> {HERE} (Pillow {PIL_VERSION})")


if __name__ == "__main__":
    main()
