"""PJD_F_LIBJPEG on progressive frames, on the host (no GPU): the expectation chain of tests/test_gpu_libjpeg_progressive.py.

The fixtures of tests/golden/libjpeg_progressive/ -- Pillow's coefficients under scan scripts no encoder writes -- equal their
manifest, and tests/libjpeg_model.py over the bit-level model of tests/jpeg_progressive.py equals Pillow's recorded decode of every
one, colour and draft("L"), at zero tolerance.  pjd_libjpeg_idct equals the model on every unit of three streams, the -32768
coefficients of the int16-edge streams among them; pjd_plan_check refuses the 4:4:0 members of the hand-built corpus and takes the
rest; and what an INCOMPLETE script costs against libjpeg (its interblock smoothing, which the library does not reproduce) is
measured against Pillow's recorded decode and printed (run with -s)."""
import io
import os

import numpy as np
import pytest

import libjpeg_model as M
import libjpeg_progressive_corpus as LP

EXPECTED_MEMBERS = {(136, 72, "4:2:0"), (259, 19, "4:2:2"), (515, 21, "4:2:2"), (40, 24, "4:4:4"), (61, 45, "4:2:0"), (33, 31, "grey"),
                    (257, 19, "grey"), (6, 3, "4:2:0"), (7, 2, "4:2:0"), (10, 1, "4:2:0"), (6, 1, "4:2:2"), (11, 2, "4:2:2"), (4, 9, "4:2:0"),
                    (4, 9, "4:2:2"), (3, 5, "4:2:0"), (3, 5, "4:2:2"), (67, 35, "4:2:0")}


def test_fixture_set_is_the_one_the_tests_are_written_for():
    man = LP.manifest()
    cases = man["cases"]
    assert man["pillow"] and not man["left_out"], man["left_out"]
    assert {(c["width"], c["height"], c["sampling"]) for c in cases.values()} == EXPECTED_MEMBERS
    big = [c for c in cases.values() if (c["width"], c["height"]) == (136, 72)]
    assert len(big) == 2 and all(c["n_units"] == 270 > 2 * 96 for c in big)                  # three back-end ranges
    assert cases["lp_259x19_422_q75_two_bands"]["n_units"] == 204 > 2 * 96
    slot48 = cases["lp_136x72_420_q90_slot48_alone"]
    assert slot48["nonzero_at_slot_48"] >= 50
    scans = LP.script_of(slot48["script"])
    assert {(s.ss, s.se) for s in scans if s.ss} >= {(z, z) for z in range(48, 53)}
    assert sum(c["nonzero_at_slot_48"] > 0 for c in cases.values()) >= 8
    assert max(s.al for s in LP.script_of(cases["lp_61x45_420_q90_three_levels"]["script"])) == 3
    ris = [s.ri for s in LP.script_of(cases["lp_40x24_444_q95_dri_changes"]["script"])]
    assert len({r for r in ris if r}) >= 4 and 0 in ris[1:]
    assert {t for c in cases.values() for s in LP.script_of(c["script"]) for t in s.tid} == {0, 1, 2, 3}
    on_disk = {f for f in os.listdir(LP.GOLD) if f not in ("manifest.json", "make_fixtures.py") and not f.startswith("__")}
    assert on_disk == {f"{n}.{ext}" for n, c in cases.items() for ext in c["sha256"]}
    assert all(os.path.getsize(os.path.join(LP.GOLD, f)) < 35 * 1024 for f in on_disk)


def test_fixtures_equal_their_manifest_and_the_model_equals_pillows_record():
    n = 0
    for name, data, frame, c in LP.fixtures():
        rgb, l8 = LP.record(name)
        assert LP.sha(data) == c["sha256"]["jpg"] and LP.sha(rgb.tobytes()) == c["sha256"]["rgb"] and LP.sha(l8.tobytes()) == c["sha256"]["l8"], name
        assert (frame.width, frame.height, LP.SAMPLING_NAMES[frame.sampling()]) == (c["width"], c["height"], c["sampling"]), name
        status, coef, got, luma = LP.model_expected(data, frame)
        assert status == 0, name
        assert len(LP.decoded(data).scans) == c["n_scans"] and LP.decoded(data).coef.shape[0] == c["n_units"], name
        assert got.shape == rgb.shape and np.array_equal(got, rgb), f"{name}: {int((got != rgb).sum())} bytes differ from Pillow's decode"
        assert luma.shape == l8.shape and np.array_equal(luma, l8), f"{name}: {int((luma != l8).sum())} bytes differ from Pillow's draft('L')"
        n += 1
    print(f"\n{n} fixtures compared with Pillow's recorded decode")
    assert n == len(LP.manifest()["cases"]) == 18


def test_recorded_decode_is_this_pillows():
    """Where Pillow is installed its decode of every fixture is the recorded one (a libjpeg whose defaults differ would show here)."""
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for name, data, _, _ in LP.fixtures():
        rgb, l8 = LP.record(name)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), rgb), name
        im = Image.open(io.BytesIO(data))
        im.draft("L", im.size)
        assert im.mode == "L" and np.array_equal(np.asarray(im), l8), name
        n += 1
    for name in LP.manifest()["incomplete"]:
        data, _ = LP.incomplete_stream(name)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), LP.incomplete_record(name)), name
        n += 1
    assert n == 18 + 5


def _units(data, frame):
    """[(component's natural quantisers, int16 coefficients in natural order)] of every data unit of the stream"""
    qts = LP.natural_quantisers(frame)
    _, coef = LP.model_coefficients(data, frame)
    grids = M.unit_grids(coef, frame.width, frame.height, len(frame.comps), frame.hs, frame.vs)
    return [(np.asarray(qts[c]), u) for c, g in enumerate(grids) for u in g.reshape(-1, 64)]


def test_host_idct_equals_the_model_on_every_unit_of_three_streams():
    """The saturating member (the IDCT's clamp) and the two int16-edge streams: coefficients of -32768 at natural 0 and at slot 52's
    natural position, where the product with the quantiser needs more than 16 bits."""
    import pjd_amd
    sat = next(x for x in LP.fixtures() if x[0] == "lp_sat67x35_420_q100")
    n = n_min = 0
    for label, data, frame in [sat[:3]] + LP.edge_items():
        for q, u in _units(data, frame):
            want = M.idct_units(u[None, :], q)[0].reshape(64)
            assert np.array_equal(pjd_amd.libjpeg_idct(u, (q & 0xFFFF).astype(np.uint16)), want), label
            n += 1
            n_min += int((u == -32768).any())
    assert n >= 60 + 8 + 24 and n_min >= 8, (n, n_min)


def test_plan_check_refuses_the_440_members_and_takes_the_rest():
    import pjd_amd
    taken = refused = 0
    for label, data, frame in LP.corpus_items() + LP.refused_items():
        s = pjd_amd.Scanned(data, options=pjd_amd.SCAN_PROGRESSIVE)
        assert s.valid and int(s.desc.flags) & pjd_amd.F_PROGRESSIVE, label
        s.desc.flags = int(s.desc.flags) | pjd_amd.F_LIBJPEG
        for fmt in (pjd_amd.OUT_RGB8, pjd_amd.OUT_GRAY8):
            rc, why = pjd_amd.plan_check([s.desc], fmt)
            if frame.sampling() == "440":
                assert rc == -3 and why == "image 0: PJD_F_LIBJPEG does not take 4:4:0 (h1v2) sampling", (label, rc, why)
            else:
                assert (rc, why) == (0, ""), (label, rc, why)
        refused += frame.sampling() == "440"
        taken += frame.sampling() != "440"
    assert (taken, refused) == (46, 9)                   # 15 named + 40 seeded streams: one named and every fifth seeded one are 4:4:0
    assert len(LP.broken_items()) >= 90 and {LP.decoded(d).status for _, d, _ in LP.broken_items()} == set(range(1, 8))


def test_what_an_incomplete_script_costs_against_libjpeg():
    """Five members rewritten with their last four scans dropped: the coefficients are not fully refined, libjpeg smooths such a frame
    between blocks and the library does not.  The figures are levels between PILLOW'S recorded decode and the model -- the distance
    from libjpeg outside the envelope include/pjd.h states, no tolerance on the library."""
    inc = LP.manifest()["incomplete"]
    assert len(inc) == 5
    figures = {}
    for name, rec in sorted(inc.items()):
        data, frame = LP.incomplete_stream(name, rec["dropped_scans"])
        assert LP.sha(data) == rec["jpg_sha256"], name
        status, _, model, _ = LP.model_expected(data, frame)
        assert status == 0, name
        figures[name] = int(np.abs(LP.incomplete_record(name).astype(int) - model.astype(int)).max())
    print("\nincomplete scripts, levels between Pillow's decode and the model:", figures)
    assert figures == {n: r["max_diff_pillow_to_model"] for n, r in inc.items()}
    assert max(figures.values()) >= 1
