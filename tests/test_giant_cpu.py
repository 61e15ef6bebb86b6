"""The size-limit family (tests/giant_corpus.py), the parts that need no GPU: that a spliced file decodes to the tiling of its two period
pictures (the oracle port, and the libjpeg model where it applies, on whole decodes at 203 x 213), that the planner takes every member
in every format the GPU tests decode it in without routing it to the exact kernel, that every member's plan holds the offset above
2^32 -- or the bit position above 2^32 - 2^21 -- it exists for, that one byte more than 2^29 - 1 is refused, and the size functions at
65535 x 65535 against Python's integers."""
import numpy as np
import pytest

import giant_corpus as GC
import libjpeg_corpus as LC

synth = GC.synth
FMT = {"rgb8": 0, "bmp": 1, "planar": 2, "gray": 4}      # pjd_amd.OUT_*
TWO32 = 1 << 32
SMALL_W, SMALL_H = 203, 213


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for k in ("PJD_SUB_BYTES", "PJD_PLAN_MODE", "PJD_ODD_WAVE_PCT"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scanned():
    """name -> Scanned of every member (flags left to the test)"""
    import pjd_amd
    out = {}
    for name in GC.NAMES:
        s = pjd_amd.Scanned(GC.jpeg(name), name + ".jpg")
        assert s.valid, (name, s.log)
        out[name] = s
    return out


def _with_flags(s, flags):
    import ctypes as C
    import pjd_amd
    d = pjd_amd.ImageDesc()
    C.memmove(C.byref(d), C.byref(s.desc), C.sizeof(pjd_amd.ImageDesc))
    d.flags = flags
    return d


# ---- the construction, held against whole decodes at a size the CPU decodes -------------------------------------------------------------
@pytest.mark.parametrize("tag,sub", [("444", GC.S444), ("422", GC.S422), ("420", GC.S420)])
def test_a_spliced_file_decodes_to_the_tiling_of_its_periods(port, tag, sub):
    """203 x 213: 27 segments of 8 rows (14 of 16 rows in 4:2:0), the last one cut by the picture's height; DRI 26 or 13, where the
    reference's restart rule and T.81's coincide (13 is odd), so the port decodes the subsampled files as every decoder does."""
    hs, vs = GC.LUMA[sub]
    per, ri = 8 * vs, -(-SMALL_W // (8 * hs))
    n = -(-SMALL_H // per)
    marks = (0, 5, 6, n - 1)
    main = synth.make(SMALL_W, 8 * per, 7301, 30, sub, ri, 0.25)
    alt = synth.make(SMALL_W, 8 * per, 7351, 30, sub, ri, 0.25)
    giant = GC.splice(main, SMALL_H, marks, alt)
    d = port.decode(giant)
    assert d["valid"] and d["huff_rc"] == 0
    assert (d["info"]["width"], d["info"]["height"], d["info"]["restart_interval"]) == (SMALL_W, SMALL_H, ri)
    pm, pa = port.decode(main), port.decode(alt)
    assert pm["huff_rc"] == pa["huff_rc"] == 0 and not np.array_equal(pm["rgb"], pa["rgb"])
    want = GC.tile(pm["rgb"], pa["rgb"], marks, per, 0, SMALL_H)
    assert want.shape == (SMALL_H, SMALL_W, 3) and np.array_equal(d["rgb"], want)
    assert not np.array_equal(want, GC.tile(pm["rgb"], pa["rgb"], (), per, 0, SMALL_H))      # the marked segments show
    assert np.array_equal(GC.tile(pm["rgb"], pa["rgb"], marks, per, 37, 150), want[37:150])
    if sub != GC.S420:                                    # libjpeg's h2v2 upsampling reads across MCU rows: no flagged 4:2:0 giant
        st, lj = LC.expected(port, giant)
        (sm, lm), (sa, la) = LC.expected(port, main), LC.expected(port, alt)
        assert st == sm == sa == 0
        assert np.array_equal(lj, GC.tile(lm, la, marks, per, 0, SMALL_H))
        import gray_expected
        sy, y = gray_expected.model_y_plane(port, giant, broken=True)
        planes = [gray_expected.model_y_plane(port, p) for p in (main, alt)]
        assert sy == 0 and np.array_equal(y, GC.tile(planes[0], planes[1], marks, per, 0, SMALL_H))
    if sub == GC.S444:
        import gray_expected
        sy, y = gray_expected.ref_plane(port, giant)
        planes = [gray_expected.ref_plane(port, p)[1] for p in (main, alt)]
        assert sy == 0 and np.array_equal(y, GC.tile(planes[0], planes[1], marks, per, 0, SMALL_H))


def test_a_padded_stream_and_a_damaged_last_segment_at_a_small_size(port):
    """What g444_full and g444_full_err do, at 203 x 213: zero bytes before the EOI change nothing, and an erring code in the last
    segment's last bytes leaves every earlier segment the tiling."""
    per, ri = 8, 26
    main = synth.make(SMALL_W, 64, 7301, 85, GC.S444, ri, 1.0)
    alt = synth.make(SMALL_W, 64, 7351, 85, GC.S444, ri, 1.0)
    n = -(-SMALL_H // per)
    marks = (0, n - 1)
    plain = GC.splice(main, SMALL_H, marks, alt)
    total = sum(GC.destuffed_len(b) for b in GC.bodies(main)) * 4      # more than the 27 segments hold
    padded = GC.splice(main, SMALL_H, marks, alt, pad_to=total)
    assert port.parse(padded)["info"]["ecs_len"] == total > port.parse(plain)["info"]["ecs_len"]
    a, b = port.decode(plain), port.decode(padded)
    assert a["huff_rc"] == b["huff_rc"] == 0 and np.array_equal(a["rgb"], b["rgb"])
    bad = None
    for back in range(4, 40):
        bad = GC.damaged_body(GC.bodies(alt)[(n - 1) % 8], back)
        if bad is not None:
            break
    broken = port.decode(GC.splice(main, SMALL_H, marks, alt, pad_to=total, last_body=bad))
    assert broken["huff_rc"] != 0
    assert np.array_equal(broken["rgb"][:(n - 1) * per], a["rgb"][:(n - 1) * per])


# ---- the members' plans -----------------------------------------------------------------------------------------------------------------
def test_members_are_what_the_table_says(scanned):
    assert GC.NAMES == ["g444", "g420_std", "g422_tall", "g444_full"]
    for name, (w, h) in {"g444": (65535, 24571), "g420_std": (65535, 24571), "g422_tall": (21851, 65535)}.items():
        d = scanned[name].desc
        assert (int(d.width), int(d.height)) == (w, h) == (GC.spec(name)[0], GC.height(name))
        assert (int(d.h_samp), int(d.v_samp)) == GC.LUMA[GC.spec(name)[2]]
        assert int(d.n_segments) == GC.n_segments(name) and int(d.ecs_len) < 128 << 20
    assert [int(scanned[n].desc.restart_interval) for n in GC.NAMES] == [8192, 4096, 1366, 8192]
    assert GC.n_segments("g422_tall") == 8192
    for name in GC.NAMES:
        mk = GC.marks(name)
        assert mk[0] == 0 and mk[-1] == GC.n_segments(name) - 1
        for rows in GC.crossings(name).values():
            for y in rows:
                assert y // GC.seg_rows(GC.spec(name)[2]) in mk, (name, y)


@pytest.mark.parametrize("name", GC.NAMES)
def test_plan_of_every_member_in_every_format_it_is_decoded_in(scanned, name):
    import pjd_amd
    w, _, _, _, _, _, member_flags, formats = GC.spec(name)
    h = GC.height(name)
    n = 0
    for flags in member_flags:
        for fmt in formats:
            if fmt == "gray" and name == "g422_tall" and not flags & GC.F_LIBJPEG:
                continue
            d = _with_flags(scanned[name], flags)
            pi = pjd_amd.plan_info([d], FMT[fmt])
            assert pi["n_sequential"] == 0 and pi["n_fallback"] == 0, (name, flags, fmt)
            assert pi["pixels"] == w * h
            assert pi["out_bytes"] == GC.out_bytes(w, h, fmt) == pjd_amd.image_output_size(d, FMT[fmt]), (name, flags, fmt)
            assert pi["n_subsequences"] >= GC.n_segments(name)
            n += 1
    assert n == {"g444": 4, "g420_std": 2, "g422_tall": 5, "g444_full": 1}[name]


def test_every_member_holds_the_offset_it_exists_for(scanned):
    x = GC.crossings("g444")
    w, h = 65535, 24571
    assert x["rgb8"] == [21845] and 21845 * 3 * w < TWO32 < 21846 * 3 * w                   # passed inside row 21845
    assert x["gray"] == [] and w * h < TWO32
    (yb,) = x["planar"]
    assert 2 * w * h + yb * w < TWO32 < 2 * w * h + (yb + 1) * w and 3 * w * h > TWO32      # in the B plane
    (ybmp,) = x["bmp"]
    stride = 3 * w + 3
    assert 26 + (h - 1 - ybmp) * stride < TWO32 <= 26 + (h - ybmp) * stride                 # counted from the bottom
    assert GC.out_bytes(w, h, "bmp") % TWO32 == (26 + h * stride) - TWO32                   # the header's size field is taken mod 2^32
    x = GC.crossings("g420_std")
    assert x["rgb8"] == [21845] and len(x["planar"]) == 1
    w, h = 21851, 65535
    x = GC.crossings("g422_tall")
    assert x["rgb8"] == [65519] and 3 * w * h > TWO32 and x["gray"] == []
    (yb,) = x["planar"]
    assert 2 * w * h + yb * w < TWO32 < 2 * w * h + (yb + 1) * w
    # under PJD_F_LIBJPEG: the component planes (whole MCUs: Y, Cb, Cr) and the colour launch's items of four pixels
    mcux, mcuy = -(-w // 16), -(-h // 8)
    assert (mcux, mcuy) == (1366, 8192) and h - 1 == 65534
    planes = mcux * 16 * mcuy * 8 + 2 * mcux * 8 * mcuy * 8
    assert 2.8e9 < planes < TWO32 and ((w + 3) // 4) * h > 1 << 28
    # the stream limit
    d = scanned[GC.FULL].desc
    assert int(d.ecs_len) == (1 << 29) - 1 == GC.ECS_CAP
    offs = scanned[GC.FULL].seg_offsets()
    n = GC.n_segments(GC.FULL)
    assert len(offs) == n and GC.height(GC.FULL) == 8 * n
    last = GC.bodies(GC.period_jpeg(GC.FULL, alt=True))[(n - 1) % 8]
    pad = int(d.ecs_len) - int(offs[-1]) - GC.destuffed_len(last)
    assert 0 <= pad < GC.destuffed_len(last) and pad < 200_000                               # shorter than one segment
    # a unit is at most 27 + 63 * 26 bits = 209 bytes: the last one starts within 256 bytes of its segment's end
    assert (int(offs[-1]) + GC.destuffed_len(last) - 256) * 8 > TWO32 - (1 << 21)
    assert int(offs[-1]) * 8 > TWO32 - (1 << 22)                                            # base_bit of the last segment


def test_one_byte_more_is_refused_on_both_sides_of_the_cap(scanned):
    import pjd_amd
    good = scanned[GC.FULL]
    assert pjd_amd.plan_check([good.desc]) == (0, "")
    data = GC.jpeg(GC.FULL)
    longer = pjd_amd.Scanned(data[:-2] + b"\x00\xff\xd9")
    assert longer.valid and int(longer.desc.ecs_len) == 1 << 29
    code, reason = pjd_amd.plan_check([longer.desc])
    assert code == -3 and "512 MiB" in reason, (code, reason)                                # PJD_E_ARG
    with pytest.raises(pjd_amd.PjdError):
        pjd_amd.plan_info([longer.desc])


def test_the_reference_rule_routes_the_subsampled_giant_to_the_exact_kernel(scanned):
    """Why g420_std is never decoded without its flag: under the reference's restart rule a DRI of 4096 MCUs is no multiple of what
    that rule counts, the planner gives the picture to the one-lane kernel, and 1.6 GPix there would take minutes."""
    import pjd_amd
    assert pjd_amd.plan_info([_with_flags(scanned["g420_std"], 0)])["n_sequential"] == 1
    assert pjd_amd.plan_info([_with_flags(scanned["g420_std"], GC.F_STANDARD_RESTART)])["n_sequential"] == 0
    assert pjd_amd.plan_info([_with_flags(scanned["g422_tall"], 0)])["n_sequential"] == 1


def test_size_functions_at_65535_squared():
    import pjd_amd
    L = pjd_amd.dev_lib()
    n = 65535
    want = {0: 3 * n * n, 1: 26 + n * (3 * n + n % 4), 2: 3 * n * n, 4: n * n}
    d = pjd_amd.ImageDesc()
    d.width = d.height = n
    d.num_components, d.h_samp, d.v_samp = 3, 1, 1
    for fmt, size in want.items():
        assert size > TWO32 or fmt == 4
        assert int(L.pjd_output_size(n, n, fmt)) == size
        assert pjd_amd.image_output_size(d, fmt) == size
    assert want[4] == 4294836225 < TWO32 < want[0] == 12884508675
    for hs, vs in ((1, 1), (2, 1), (2, 2), (1, 2)):
        w8 = h8 = 8192
        assert int(L.pjd_coefficients_size(n, n, hs, vs)) == (w8 * h8 + 99) // 100 * 19200 == 12884908800
    assert int(L.pjd_coefficients_size(65521, 65535, 2, 1)) == ((8191 + 1) * 8192 + 99) // 100 * 19200
