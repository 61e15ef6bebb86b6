"""Builds the EXIF fixtures of this folder from one small golden JPEG (../env_61x45_444_q85_opt.jpg): the same file with hand-built
APPn segments inserted right behind SOI, and manifest.json, which says for every fixture what pjd_scanned_orientation must return and
whether the segment is well formed (then Pillow must read the same tag).

    python3 tests/golden/exif/make_exif_fixtures.py

No library writes the segments: every byte is laid down here, so that the malformed ones are malformed in exactly one way -- one
fixture per clause of the rule in include/pjd_host.h.  Deterministic: running it again writes the same bytes."""
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = "env_61x45_444_q85_opt"


def entry(e, tag, typ, count, value4):
    """One 12-byte IFD entry; value4: the four bytes of the value field, already in the file's byte order."""
    return struct.pack(e + "HHI", tag, typ, count) + value4


def short_value(e, v):
    return struct.pack(e + "HH", v, 0)


def tiff(e, ifd0, ifd0_offset=8, next_ifd=0, after=b"", magic=42):
    """A TIFF header in byte order e ("<" or ">"), padding up to ifd0_offset, IFD0 with the given entries, the offset of the next IFD
    and whatever follows."""
    head = (b"II" if e == "<" else b"MM") + struct.pack(e + "HI", magic, ifd0_offset)
    body = head + b"\0" * (ifd0_offset - 8)
    return body + struct.pack(e + "H", len(ifd0)) + b"".join(ifd0) + struct.pack(e + "I", next_ifd) + after


def app(marker, payload, declared=None):
    """An APPn segment; declared: the length field where it is not the payload's length + 2."""
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2 if declared is None else declared) + payload


def exif(payload_tiff, **kw):
    return app(0xE1, b"Exif\0\0" + payload_tiff, **kw)


JFIF = app(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
XMP = app(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta xmlns:x='adobe:ns:meta/'><tiff:Orientation>7</tiff:Orientation></x:xmpmeta>")
WIDTH = lambda e: entry(e, 0x0100, 4, 1, struct.pack(e + "I", 61))          # ImageWidth, LONG: an entry in front of the tag


def orientation_tiff(e, v, typ=3, count=1, **kw):
    return tiff(e, [WIDTH(e), entry(e, 0x0112, typ, count, short_value(e, v))], **kw)


def fixtures():
    """[(name, bytes inserted behind SOI, expected orientation, well formed)]"""
    out = []
    for e, bo in (("<", "ii"), (">", "mm")):
        for v in range(1, 9):
            out.append((f"exif_{bo}_{v}", exif(orientation_tiff(e, v)), v, True))
    out.append(("exif_behind_jfif_6", JFIF + exif(orientation_tiff(">", 6)), 6, True))
    out.append(("exif_behind_xmp_8", XMP + exif(orientation_tiff("<", 8)), 8, True))
    out.append(("exif_ifd0_at_offset_26_5", exif(orientation_tiff("<", 5, ifd0_offset=26)), 5, True))
    # ---- one malformed case per clause: all give 1 --------------------------------------------------------------------------------
    e = "<"
    # a truncated segment: the length field reaches past the end of the FILE (the fixture ends inside the segment; not a JPEG any more)
    out.append(("bad_truncated_segment", None, 1, False))
    # the TIFF header is cut off by the segment's end
    out.append(("bad_short_tiff_header", exif(b"II*\0\x08\0"), 1, False))
    out.append(("bad_byte_order", exif(b"IM" + orientation_tiff(e, 6)[2:]), 1, False))
    out.append(("bad_magic_43", exif(orientation_tiff(e, 6, magic=43)), 1, False))
    # the IFD0 offset points outside the segment
    out.append(("bad_ifd0_offset_outside", exif((b"II" + struct.pack("<HI", 42, 4096)) + orientation_tiff(e, 6)[8:]), 1, False))
    # the entry count promises entries the segment does not hold: the tag would be the third entry, cut off after 6 bytes
    t = tiff(e, [WIDTH(e), WIDTH(e), entry(e, 0x0112, 3, 1, short_value(e, 6))])
    out.append(("bad_entry_cut_off", exif(t[:8 + 2 + 24 + 6]), 1, False))
    out.append(("bad_type_long", exif(tiff(e, [entry(e, 0x0112, 4, 1, struct.pack("<I", 6))])), 1, False))
    out.append(("bad_count_2", exif(orientation_tiff(e, 6, count=2)), 1, False))
    out.append(("bad_value_0", exif(orientation_tiff(e, 0)), 1, False))
    out.append(("bad_value_9", exif(orientation_tiff(">", 9)), 1, False))
    # the tag only in IFD1 (the thumbnail's directory)
    ifd0 = [WIDTH(e)]
    ifd1_off = 8 + 2 + 12 * len(ifd0) + 4
    ifd1 = struct.pack("<H", 1) + entry(e, 0x0112, 3, 1, short_value(e, 6)) + struct.pack("<I", 0)
    out.append(("bad_only_in_ifd1", exif(tiff(e, ifd0, next_ifd=ifd1_off, after=ifd1)), 1, False))
    # the tag only in the Exif sub-IFD (tag 0x8769 of IFD0 points to it)
    sub_off = 8 + 2 + 12 * 2 + 4
    ifd0 = [WIDTH(e), entry(e, 0x8769, 4, 1, struct.pack("<I", sub_off))]
    out.append(("bad_only_in_exif_subifd", exif(tiff(e, ifd0, after=ifd1)), 1, False))
    # a second Exif segment is not looked at: the first one (without the tag) decides
    out.append(("bad_tag_in_second_exif_segment", exif(tiff(e, [WIDTH(e)])) + exif(orientation_tiff(e, 6)), 1, False))
    # "Exif" without the two zero bytes is not an Exif segment, and APP2 is not APP1
    out.append(("bad_identifier", app(0xE1, b"Exif\0\x01" + orientation_tiff(e, 6)), 1, False))
    out.append(("bad_app2", app(0xE2, b"Exif\0\0" + orientation_tiff(e, 6)), 1, False))
    return out


def main():
    with open(os.path.join(HERE, "..", BASE + ".jpg"), "rb") as f:
        base = f.read()
    assert base[:2] == b"\xff\xd8"
    manifest = {"base": BASE, "fixtures": {}}
    for name, seg, want, well_formed in fixtures():
        if name == "bad_truncated_segment":
            whole = exif(orientation_tiff("<", 6), declared=4000)
            data = base[:2] + whole                       # the file ends inside the segment whose length field says 4000
            valid = False
        else:
            data = base[:2] + seg + base[2:]
            valid = True
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(data)
        manifest["fixtures"][name] = {"orientation": want, "well_formed": well_formed, "valid_jpeg": valid}
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(manifest["fixtures"]), "fixtures")


if __name__ == "__main__":
    main()
