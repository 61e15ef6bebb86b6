"""The planner statements tests/test_gpu_group_forms.py rests on, as assertions that need no GPU (pjd_plan_info and the check functions
are host only): every batch of the GPU file plans three picture groups, every resample request it makes is one the library accepts, and
the PJD_GROUP_CUTS parser returns on every list.  A GPU case whose batch does not plan three groups then fails here first, instead of
passing on the single chain."""
import os
import subprocess
import sys
import textwrap

import pytest

import group_corpus as G
from conftest import golden_bytes, ROOT

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in G.ENV_OFF:
        monkeypatch.delenv(k, raising=False)


def _dims(scanned):
    return [(int(s.desc.width), int(s.desc.height)) for s in scanned]


def _info(scanned, fmt="rgb8"):
    import pjd_amd
    return pjd_amd.plan_info([s.desc for s in scanned], G.out_format(fmt))


def test_the_corpus_as_measured(monkeypatch):
    """85 pictures in 91 waves, 87 workgroups and 44 table sets; three groups in every output format; the planner's own lane size is 176
    bytes, PJD_SUB_BYTES=128 holds where set."""
    sc = G.scan(G.jpegs())
    assert len(sc) == 85 and _dims(sc)[30:33] == [(203, 149), (320, 240), (161, 300)]
    for fmt in ("rgb8", "bmp", "planar", "gray"):
        i = _info(sc, fmt)
        assert i["dc_plan"] >> 8 == 3, (fmt, i["dc_plan"])
        assert (i["n_huff_waves"], i["n_huff_workgroups"], i["n_table_sets"], i["sub_bytes"], i["n_sequential"]) == (91, 87, 44, 176, 0), (fmt, i)
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    assert _info(sc)["sub_bytes"] == 128 and _info(sc)["dc_plan"] >> 8 == 3


def test_the_damaged_copies_differ_from_their_originals_in_four_bytes_at_most():
    j, s = G.jpegs(), G.small()
    for pos, k in zip((83, 84), G.DAMAGED_OF):
        assert len(j[pos]) == len(s[k]) and 0 < sum(a != b for a, b in zip(j[pos], s[k])) <= 4
        assert b"\xff\x00\xff\x00" in j[pos][j[pos].rfind(b"\xff\xda"):]


def test_pictures_of_several_waves_and_every_sampling_in_each_third_of_the_density_order():
    """The larger pictures are alone several waves long.  By stream bytes per pixel, densest first, every third of the batch holds every
    sampling.  The planner's own key is bytes per MCU, and a grey MCU is one block: by that key every third holds the four colour
    samplings, and the grey pictures lie in the second and the last third -- so in at least two of the three groups."""
    import pjd_amd
    sc = G.scan(G.jpegs())
    waves = [pjd_amd.plan_info([s.desc], pjd_amd.OUT_RGB8)["n_huff_waves"] for s in sc]
    assert sum(w >= 2 for w in waves) >= 2 and max(waves) >= 3, sorted(waves)[-5:]

    def sampling(d):
        return "grey" if int(d.num_components) == 1 else "%d%d" % (int(d.h_samp), int(d.v_samp))

    def per_pixel(d):
        return int(d.ecs_len) / (int(d.width) * int(d.height))

    def per_mcu(d):
        mw, mh = 8 * int(d.h_samp), 8 * int(d.v_samp)
        return int(d.ecs_len) / ((-(-int(d.width) // mw)) * (-(-int(d.height) // mh)))
    every = {sampling(s.desc) for s in sc}
    assert len(every) == 5, every
    for density, want in ((per_pixel, [every] * 3), (per_mcu, [every - {"grey"}, every, every])):
        order = sorted(range(len(sc)), key=lambda i: -density(sc[i].desc))
        for t in range(3):
            third = order[t * len(order) // 3:(t + 1) * len(order) // 3]
            assert {sampling(sc[i].desc) for i in third} == want[t], (density.__name__, t)


def test_three_groups_under_every_flag_mix_of_the_gpu_file(monkeypatch):
    import pjd_amd
    import fallback_corpus as F
    jp = list(G.jpegs())
    # a: grey, the scales cycling; the same with one picture routed to the exact kernel
    flags = [f for f, _ in G.scale_cycle()]
    for fmt in ("gray", "planar", "rgb8"):
        assert G.groups(G.scan(jp, flags), fmt) == 3, fmt
    flags[11] |= pjd_amd.F_FORCE_SEQUENTIAL
    sc = G.scan(jp, flags)
    assert _info(sc, "planar")["dc_plan"] >> 8 == 3 and _info(sc, "planar")["n_sequential"] == 1
    # e: three pictures on the exact path inside the grouped batch
    label, prog, _ = G.progressive_member()
    sc = G.scan(G.inserted(jp, {20: golden_bytes("huff_oversub_96x64_444")}), [pjd_amd.F_FORCE_SEQUENTIAL if k == 11 else 0 for k in range(86)])
    p = pjd_amd.Scanned(prog, options=pjd_amd.SCAN_PROGRESSIVE)
    assert p.valid and int(p.desc.flags) & pjd_amd.F_PROGRESSIVE, label
    sc.insert(60, p)
    for fmt in ("rgb8", "gray"):
        i = _info(sc, fmt)
        assert i["dc_plan"] >> 8 == 3 and i["n_sequential"] == 3, (fmt, i["dc_plan"], i["n_sequential"])
    # g: the throughput plan
    monkeypatch.setenv("PJD_PLAN_MODE", "throughput")
    assert G.groups(G.scan(jp), "planar") == 3
    monkeypatch.delenv("PJD_PLAN_MODE")
    # f: a stream that falls back in pjd_batch_sync, lanes of 128 bytes
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    fall = F.falling()["lock_420_130"].data
    sc = G.scan(G.inserted(jp, {40: fall}))
    assert _dims(sc)[40] == (208, 160)
    for fmt in ("planar", "gray"):
        i = _info(sc, fmt)
        assert i["dc_plan"] >> 8 == 3 and i["sub_bytes"] == 128 and i["n_sequential"] == 0, (fmt, i)


def test_no_groups_with_a_libjpeg_picture_or_fewer_than_64_fast_pictures():
    import pjd_amd
    jp = list(G.jpegs())
    assert G.groups(G.scan(jp, [pjd_amd.F_LIBJPEG if k == 20 else 0 for k in range(85)]), "planar") == 0
    seq = [pjd_amd.F_FORCE_SEQUENTIAL if k == 11 else 0 for k in range(85)]
    assert G.groups(G.scan(jp[:64], seq), "rgb8") == 0          # 63 fast pictures
    assert G.groups(G.scan(jp[:65], seq), "rgb8") == 3          # 64
    assert G.groups(G.scan(jp[:64]), "rgb8") == 3


def test_every_resample_request_of_the_gpu_file_is_accepted():
    """The setters of a batch refuse a whole call for one bad record: checked here, record by record, with the library's own functions."""
    import pjd_amd
    sc = G.scan(G.jpegs())
    dims = _dims(sc)
    assert max(w for w, _ in dims) == 320 and max(h for _, h in dims) == 300
    for filt in G.FILTERS:
        req = G.resize_request(dims, filt)
        assert G.request_ok(dims, req, filt) is None, (filt, G.request_ok(dims, req, filt))
        assert sum(r["win"] is not None for r in req) == 29 and {r["o"] for r in req} == set(range(1, 9))
        assert {r["pad"] for r in req} == set(G.PADS)
        if filt == "bilinear":
            assert {r["target"][0] for r in req} == set(G.WIDTHS) and {r["target"][1] for r in req} == set(G.HEIGHTS)
        else:                                                # the 16x limit against the 320- and 300-sample axes: a larger target stood in
            for (w, h), r in zip(dims, req):
                sw, sh = (r["win"]["w"], r["win"]["h"]) if r["win"] else (w, h)
                assert sw <= 16 * r["target"][0] and sh <= 16 * r["target"][1], (filt, w, h, r)
            assert req[31]["target"][0] >= 20 and req[32]["target"][1] >= 19, (req[31], req[32])
            assert any(r["target"] == (1, 7) for r in req), "the smallest target stays where a picture admits it"
    # d, e, f
    assert G.request_ok(dims, G.fixed_request(dims, 37, 29, "bilinear"), "bilinear") is None
    edims = dims[:20] + [(96, 64)] + dims[20:]
    assert G.request_ok(edims, G.fixed_request(edims, 41, 30, "antialias"), "antialias") is None
    fdims = dims[:40] + [(208, 160)] + dims[40:]
    assert G.request_ok(fdims, G.fixed_request(fdims, 37, 29, "bilinear", (1, 1, 1, 1)), "bilinear") is None
    # c
    wr = G.warp_request(dims)
    assert len(wr["views"]) == 170 and wr["views"] != sorted(wr["views"])
    for v, (p, (tw, th), m) in enumerate(zip(wr["views"], wr["sizes"], wr["mats"])):
        assert pjd_amd.resize_affine_check(dims[p][0], dims[p][1], tw, th, m), (v, p, m)
    assert all(pjd_amd.colour_check(m) for m in wr["colours"]) and len({tuple(m) for m in wr["colours"]}) == 8


CUTS_CHILD = """
    import os, resource, sys
    resource.setrlimit(resource.RLIMIT_AS, (4 << 30, 4 << 30))      # a parser that appends for ever fails fast instead of eating the machine
    sys.path[:0] = %r
    import pjd_amd, group_corpus as G
    for k in G.ENV_OFF:
        os.environ.pop(k, None)
    keep = G.scan(G.jpegs())
    for cuts, want in %r:
        os.environ["PJD_GROUP_CUTS"] = cuts
        got = G.groups(keep, "rgb8")
        print("CUTS", repr(cuts), got, flush=True)
        assert got == want, (cuts, got, want)
    print("RESULT ok")
"""
CUTS = [("30;65", 3), ("abc", 3), ("30,,65", 3), ("65,30", 3), ("0,50", 3), ("30,65x", 3), ("20,55", 3), ("25,50,75", 4), ("", 3), ("30,100", 3), ("50", 2), (" 20 , 55 ", 3)]


def test_group_cuts_parser_returns_on_every_list():
    """PJD_GROUP_CUTS with a character strtoul does not consume ("30;65") made the planner append to a vector until memory ran out, in
    every pjd_batch_create of the process.  A list with a value outside 1..99, not strictly ascending or with trailing junk gives the
    default cuts (three groups); good lists still cut where they say.  In a child process with its address space limited."""
    path = [os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"), HERE, os.path.join(ROOT, "tools")]
    code = textwrap.dedent(CUTS_CHILD) % (path, CUTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout[-600:] + r.stderr[-2000:])
