"""The dimension-limit family (tests/geometry_corpus.py), the parts that need no GPU: the scanner against the oracle's parse, the segment
counts, the planner (routing, lanes, subsequence size in both plan modes, pixels and output bytes in every format at every scale),
pjd_split_plan over thousands of one-MCU segments and over a DRI of 65535, and the host's resize taps against the numpy model at the
sizes where the 32-bit branch ends and the 64-bit branch begins."""
import numpy as np
import pytest

import geometry_corpus as G
import resize_model

FORMATS = (0, 1, 2)                 # OUT_RGB8, OUT_BMP, OUT_RGB8_PLANAR
SCALE_FLAGS = (0, 16, 32, 48)       # 1, 1/2, 1/4, 1/8


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for k in ("PJD_SUB_BYTES", "PJD_PLAN_MODE", "PJD_ODD_WAVE_PCT"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scanned():
    """name -> Scanned, with the member's flags"""
    import pjd_amd
    out = {}
    for name, data, flags in G.family():
        s = pjd_amd.Scanned(data, name + ".jpg")
        s.desc.flags = int(s.desc.flags) | flags
        out[name] = s
    return out


def test_scanner_agrees_with_the_oracle_and_counts_the_segments(port, scanned):
    assert len(scanned) == len(G.NAMES) == 15
    for name, data, _ in G.family():
        s, want = scanned[name], port.parse(data, name + ".jpg")["info"]
        w, h, sub, ri = G.geometry(name)
        assert s.valid == bool(want["valid"]) and s.valid, name
        assert (int(s.desc.width), int(s.desc.height)) == (w, h) == (want["width"], want["height"]), name
        assert (int(s.desc.h_samp), int(s.desc.v_samp)) == G.SAMPLING[sub] == (want["hsamp"], want["vsamp"]), name
        assert int(s.desc.restart_interval) == ri == want["restart_interval"], name
        assert int(s.desc.n_segments) == G.n_segments(name) == (-(-G.n_mcu(name) // ri) if ri else 1), name
        assert int(s.desc.ecs_len) == want["ecs_len"], name
    assert G.n_segments("segs_65535x72_444_ri1") == 73728 > 65536 and G.n_segments(G.DRI65535) == 2
    assert G.jpeg(G.STD_RULE) == G.jpeg(G.REF_RULE) and G.oracle_bytes(G.STD_RULE) != G.jpeg(G.STD_RULE)


def _with_flags(s, flags):
    import ctypes as C
    import pjd_amd
    d = pjd_amd.ImageDesc()
    C.memmove(C.byref(d), C.byref(s.desc), C.sizeof(pjd_amd.ImageDesc))
    d.flags = int(d.flags) | flags
    return d


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_plan_of_every_member_alone_and_of_the_family(scanned, monkeypatch, mode):
    import pjd_amd
    monkeypatch.setenv("PJD_PLAN_MODE", mode)
    n_checked = 0
    for name in G.NAMES:
        s = scanned[name]
        w, h, _, _ = G.geometry(name)
        info = pjd_amd.plan_info([s.desc])
        assert info["plan_mode"] == (1 if mode == "throughput" else 0)
        assert info["n_sequential"] == (1 if name == G.REF_RULE else 0), name
        if name != G.REF_RULE:
            assert info["n_subsequences"] >= G.n_segments(name), name
        assert info["sub_bytes"] % 16 == 0 and 128 <= info["sub_bytes"] <= 1024, (name, info["sub_bytes"])
        for fmt in FORMATS:
            for flags in SCALE_FLAGS:
                d = _with_flags(s, flags)
                pi = pjd_amd.plan_info([d], fmt)
                sw, sh = pjd_amd.scaled_dims(w, h, flags)
                size = pjd_amd.image_output_size(d, fmt)
                assert (sw, sh) == (-(-w >> (flags >> 4)), -(-h >> (flags >> 4))), (name, flags)
                assert size == (26 + sh * (3 * sw + sw % 4) if fmt == 1 else 3 * sw * sh), (name, fmt, flags)
                assert pi["pixels"] == w * h and pi["out_bytes"] == size, (name, fmt, flags)
                n_checked += 1
    assert n_checked == 15 * 12
    lane = [n for n in G.NAMES if n != G.REF_RULE]
    for fmt in FORMATS:
        for flags in SCALE_FLAGS:
            descs = [_with_flags(scanned[n], flags) for n in G.NAMES]
            pi = pjd_amd.plan_info(descs, fmt)
            assert pi["n_images"] == 15 and pi["n_sequential"] == 1
            assert pi["n_subsequences"] >= sum(G.n_segments(n) for n in lane)
            assert pi["sub_bytes"] % 16 == 0 and 128 <= pi["sub_bytes"] <= 1024
            assert pi["pixels"] == sum(G.geometry(n)[0] * G.geometry(n)[1] for n in G.NAMES)
            assert pi["out_bytes"] == sum(pjd_amd.image_output_size(d, fmt) for d in descs)


@pytest.mark.parametrize("world", [2, 3, 8, 64])
@pytest.mark.parametrize("name", G.RI1 + [G.DRI65535])
def test_split_plan_tiles_segments_and_mcus(scanned, name, world):
    import pjd_amd
    d = scanned[name].desc
    nseg, n_mcu, ri = G.n_segments(name), G.n_mcu(name), G.geometry(name)[3]
    assert int(d.n_segments) == nseg
    next_seg, next_mcu, next_byte, with_work = 0, 0, 0, 0
    for r in range(world):
        got = pjd_amd.split_plan(d, world, r)
        if got is None:
            continue
        with_work += 1
        assert got["n_segs"] >= 1 and got["first_seg"] == next_seg, (name, world, r)         # disjoint, ordered, no gap
        assert got["first_mcu"] == next_mcu == min(got["first_seg"] * ri, n_mcu), (name, world, r)
        assert got["last_mcu"] == min((got["first_seg"] + got["n_segs"]) * ri, n_mcu) > got["first_mcu"], (name, world, r)
        assert got["byte_lo"] == next_byte < got["byte_hi"], (name, world, r)
        next_seg, next_mcu, next_byte = got["first_seg"] + got["n_segs"], got["last_mcu"], got["byte_hi"]
    assert (next_seg, next_mcu, next_byte) == (nseg, n_mcu, int(d.ecs_len)), (name, world)
    assert with_work == min(world, nseg), (name, world)
    if name == G.DRI65535:
        assert with_work == 2


def _indices(dn):
    if dn <= 4096:
        return np.arange(dn)
    rng = np.random.default_rng(65535)
    return np.unique(np.concatenate([np.arange(300), np.arange(dn - 300, dn), rng.integers(0, dn, 2000)]))


def _check_taps(sn, dn):
    import pjd_amd
    i0, i1, w = resize_model.taps(sn, dn)
    idx = _indices(dn)
    for i in idx:
        assert pjd_amd.resize_tap(sn, dn, int(i)) == (int(i0[i]), int(i1[i]), int(w[i])), (sn, dn, int(i))
    return len(idx)


@pytest.mark.parametrize("sn,dn", [(32768, 65535), (32769, 65535), (65535, 65535), (65535, 1), (1, 65535), (65535, 32769)])
def test_host_taps_at_the_dimension_limits(sn, dn):
    """(32768, 65535) is the top of the 32-bit branch (sn * dn = 2^31 - 32768, (2i+1) * sn up to 2^32 - 98304); (32769, 65535) is
    the first width past it.  Every index where there are at most 4096, else both ends and 2000 seeded ones."""
    n = _check_taps(sn, dn)
    assert n == dn if dn <= 4096 else n >= 600


def test_host_tap_branches_agree_below_the_threshold():
    """Three (sn, dn) with sn * dn just under 2^31, where the 32-bit branch is taken, and the same pairs swapped: both equal the
    model, whose int64 arithmetic is what the 64-bit branch computes."""
    pairs = [(46340, 46340), (65535, 32768), (33025, 65025)]
    for sn, dn in pairs:
        assert 2 ** 31 - 2 ** 17 < sn * dn < 2 ** 31, (sn, dn)
        assert _check_taps(sn, dn) >= 600 and _check_taps(dn, sn) >= 600
    for sn, dn in [(46341, 46341), (65535, 32769), (32771, 65533)]:      # the first products past it
        assert 2 ** 31 <= sn * dn < 2 ** 31 + 2 ** 17, (sn, dn)
        assert _check_taps(sn, dn) >= 600
