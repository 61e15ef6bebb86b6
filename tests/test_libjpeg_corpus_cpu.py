"""The seeded family of tests/libjpeg_corpus.py on the host (no GPU): its expectation chain -- tests/libjpeg_model.py over the oracle
port's coefficients under the T.81 zigzag -- equals Pillow's live decode of every member libjpeg still takes (an axis of at most
65500), byte for byte and with no case left out; the family covers the shapes it was made for; the array form of the model's two
loops equals the model; and pjd_libjpeg_upsample_row equals the model on the chroma rows of the W = 6, 7, 10, 11 members."""
import io

import numpy as np
import pytest

import libjpeg_corpus as LC
import libjpeg_model as M

TAGS = list(LC.SAMPLINGS)


def pillow(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def same(got, want, label):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.array_equal(got, want), f"{label}: {int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("tag", TAGS)
def test_small_family_equals_pillow(port, tag):
    n = 0
    for name, data in LC.small(tag):
        status, got = LC.expected(port, LC.model_bytes(name))
        assert status == 0, name
        same(got, pillow(data), name)
        n += 1
    assert n == 180


def test_edges_equal_pillow(port):
    n = 0
    for name, data in LC.edges():
        status, got = LC.expected(port, LC.model_bytes(name))
        assert status == 0, name
        same(got, pillow(data), name)
        n += 1
    assert n == 16


@pytest.mark.parametrize("name", list(LC.LIMITS_65500))
def test_limits_up_to_65500_equal_pillow(port, name):
    assert LC.pillow_decodes(name)
    status, got = LC.expected(port, LC.model_bytes(name))
    assert status == 0
    same(got, pillow(LC.jpeg(name)), name)


def test_pillow_refuses_what_lies_beyond_65500():
    """libjpeg's limit: above it the model is the only expectation (include/pjd.h: streams outside libjpeg's envelope)."""
    Image = pytest.importorskip("PIL.Image")
    assert not LC.pillow_decodes("w65535x1_grey")
    with pytest.raises(Exception):
        Image.open(io.BytesIO(LC.jpeg("w65535x1_grey"))).convert("RGB")


@pytest.mark.parametrize("tag", TAGS)
def test_array_form_of_the_model_equals_the_model(port, tag):
    """libjpeg_corpus.unit_grids / upsample against libjpeg_model's loops, on the small family and the short edge members."""
    members = LC.small(tag) + [(n, d) for n, d in LC.edges() if LC.dims(n)[2] == LC.SAMPLINGS[tag] and LC.dims(n)[0] <= 600]
    for name, _ in members:
        status, coef, args = LC.port_coefficients(port, LC.model_bytes(name))
        same(LC.decode(coef, *args), M.decode(coef, *args), name)
        for a, b in zip(LC.unit_grids(coef, *args[1:]), M.unit_grids(coef, *args[1:])):
            assert np.array_equal(a, b), name
    assert len(members) >= 181


def test_the_family_covers_what_it_is_for(port):
    every = [n for t in TAGS for n, _ in LC.small(t)] + [n for n, _ in LC.edges()] + [n for n, _ in LC.limits()]
    assert len(every) == len(set(every))
    sub2 = [n for n in every if LC.LUMA[LC.dims(n)[2]][0] == 2]             # horizontally subsampled: fancy upsampling where n >= 3
    nm = {}
    for name in sub2:
        w, h, sub = LC.dims(name)
        nm[name] = (w, h, (w + 1) // 2, -(-h // LC.LUMA[sub][1]), sub)
    for sub in (LC.S422, LC.S420):
        mine = [v for v in nm.values() if v[4] == sub]
        assert {w % 4 for w, h, n, m, _ in mine if n >= 3} == {0, 1, 2, 3}
        assert {w for w, h, n, m, _ in mine if n == 3} == {5, 6}
        assert any(m == 1 and n >= 3 for w, h, n, m, _ in mine)
        if sub == LC.S420:                                                   # a second chroma row that holds one picture row
            assert any(m == 2 and n >= 3 and h == 3 for w, h, n, m, _ in mine)
    for sub in LC.LUMA:
        short = [n for n, _ in LC.edges() if LC.dims(n)[2] == sub]
        assert any(LC.dims(n)[0] > 256 for n in short), sub
    for name in ("e6x3_420", "e7x2_420", "e10x1_420", "e6x1_422", "e11x2_422"):
        w, h, n, m, _ = nm[name]
        assert n >= 3 and w % 4 in (2, 3) and m == (2 if name in ("e6x3_420", "e11x2_422") else 1), name
    for name in LC.SATURATING:
        _, rgb = LC.expected(port, LC.model_bytes(name))
        share = float(((rgb == 0) | (rgb == 255)).mean())
        assert share >= 0.15, (name, share)
    axes = [max(LC.dims(n)[:2]) for n, _ in LC.limits()]
    assert max(axes) == 65535 and 65500 in axes
    for sub in (LC.S444, LC.S422, LC.S420, LC.GREY):
        assert any(max(LC.dims(n)[:2]) > 65500 for n, _ in LC.limits() if LC.dims(n)[2] == sub), sub
    assert all(LC.dims(n)[2] in LC.LUMA for n in every)                     # nothing outside the mode's envelope


@pytest.mark.parametrize("name", ["e6x3_420", "e7x2_420", "e10x1_420", "e6x1_422", "e11x2_422"])
def test_host_upsample_row_equals_the_model_on_the_members_rows(port, name):
    """The chroma planes of the member, every output row: pjd_libjpeg_upsample_row (the inline the colour kernel runs) against the
    model's row and against the array form's plane."""
    import pjd_amd
    _, coef, (qts, w, h, ncomp, hs, vs) = LC.port_coefficients(port, LC.model_bytes(name))
    grids = M.unit_grids(coef, w, h, ncomp, hs, vs)
    n, m = (w + 1) // 2, -(-h // vs)
    assert n >= 3
    rows = 0
    for c in (1, 2):
        plane = M.plane_from_units(M.idct_units(grids[c], np.asarray(qts[c]).reshape(64)))
        whole = LC.upsample(plane, w, h, hs, vs)
        for y in range(h):
            r = y // vs
            cur = np.ascontiguousarray(plane[r, :n])
            if vs == 1:
                got, want = pjd_amd.libjpeg_upsample_row(cur), M.upsample_row(cur)
            else:
                nb = np.ascontiguousarray(plane[max(r - 1, 0) if y % 2 == 0 else min(r + 1, m - 1), :n])
                got, want = pjd_amd.libjpeg_upsample_row(cur, nb, y % 2), M.upsample_row(cur, nb)
            assert np.array_equal(got, want) and np.array_equal(got[:w], whole[y]), (name, c, y)
            rows += 1
    assert rows == 2 * h


def test_entropy_cut_is_the_geometry_corpus_rule():
    import geometry_corpus as G
    assert LC.entropy_cut(G.jpeg(LC.WIDE_420), 0.5) == G.truncated(LC.WIDE_420)
    assert LC.jpeg(LC.WIDE_420) == G.jpeg(LC.WIDE_420) and LC.model_bytes(G.STD_RULE) == G.oracle_bytes(G.STD_RULE)


def test_plan_check_sorts_out_the_picture_the_flag_does_not_take():
    """pjd_plan_check, host only: the planner's own test on one descriptor, with its reason -- what the batcher and bin/decoder run on
    every scanned picture before image_flags = PJD_F_LIBJPEG reaches a batch."""
    import ctypes as C
    import pjd_amd
    from conftest import golden_bytes
    bad, good = pjd_amd.Scanned(golden_bytes("h1v2_48x64")), pjd_amd.Scanned(LC.jpeg("e7x2_420"))
    assert pjd_amd.plan_check([bad.desc]) == (0, "") and pjd_amd.plan_check([good.desc]) == (0, "")
    for s in (bad, good):
        s.desc.flags = int(s.desc.flags) | pjd_amd.F_LIBJPEG
    assert pjd_amd.plan_check([good.desc], pjd_amd.OUT_BMP) == (0, "")
    assert pjd_amd.plan_check([bad.desc], pjd_amd.OUT_BMP) == (-3, "image 0: PJD_F_LIBJPEG does not take 4:4:0 (h1v2) sampling")
    assert pjd_amd.plan_check([good.desc, bad.desc])[1].startswith("image 1: ")
    L = pjd_amd.dev_lib()
    arr = (pjd_amd.ImageDesc * 1)()
    C.memmove(C.byref(arr[0]), C.byref(bad.desc), C.sizeof(pjd_amd.ImageDesc))
    assert L.pjd_plan_check(arr, 1, pjd_amd.OUT_RGB8, None, 0) == -3                       # no text asked for
    small = C.create_string_buffer(b"x" * 16, 16)
    assert L.pjd_plan_check(arr, 1, pjd_amd.OUT_RGB8, small, 9) == -3 and small.raw[:9] == b"image 0:\0" and small.raw[9:] == b"x" * 7
