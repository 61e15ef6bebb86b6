"""The streams of tests/fallback_corpus.py held on the CPU (no GPU): every stream parses and means what the oracle port makes of it, is
cut into the lanes and waves the corpus claims, and is taken by the planner (only the device can flag it); the shard files are a sound
construction -- cut from the UNBROKEN fixtures they decode to exactly their rows of the whole picture; and the numpy models the GPU
tests expect with agree, on these streams' own coefficients, with the host exports of the inlines the kernels run, so that a model
error and a kernel error cannot cancel."""
import numpy as np
import pytest

import fallback_corpus as F
import libjpeg_corpus as LC
import libjpeg_model as M
import libjpeg_scaled_model as SM
import nosync_corpus as N

FALLING = sorted(F.falling())


@pytest.fixture
def lanes128(monkeypatch):
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    for k in ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE"):
        monkeypatch.delenv(k, raising=False)


def test_members():
    assert set(F.FROM_NOSYNC) | set(F.NEW) == set(FALLING) == set(F.WAVES) and len(FALLING) == 7
    assert {F.falling()[n].sub for n in F.NEW} == {"422", "444", "440"}
    for n in F.NEW:
        s = F.falling()[n]
        assert s.cls == 1 and s.fr.width * s.fr.height < 100_000, (n, s.fr.width, s.fr.height)


@pytest.mark.parametrize("name", FALLING)
def test_stream_parses_and_its_intent_is_the_oracle_s(port, name):
    import pjd_amd
    s = F.falling()[name]
    sc = pjd_amd.Scanned(s.data)
    assert sc.valid and (sc.desc.width, sc.desc.height) == (s.fr.width, s.fr.height)
    o = port.decode(s.data)
    assert o["valid"] and o["huff_rc"] == s.it.status == 0, (name, o["huff_rc"], s.it.status)


@pytest.mark.parametrize("name", FALLING)
def test_lanes_and_waves(name):
    """Nine waves for the new streams; seven (grey) and six for the ones tests/test_gpu_nosync.py records the routes of."""
    s = F.falling()[name]
    assert F.waves(s) == F.WAVES[name], (name, s.n_lanes(F.S))
    if name in F.LANES:
        assert s.n_lanes(F.S) == F.LANES[name]
    if name in F.NEW:
        assert F.waves(s) >= 9 and N.scan_bytes(s) == 63 * s.fr.n_units()


def test_new_streams_never_reach_the_true_state():
    """Class 1 as in tests/test_nosync_cpu.py: at least 90 % of the lanes never equal the true state, the rest start in it."""
    for n in F.NEW:
        lanes = N.Model(F.falling()[n]).lockstep_distances(F.S)
        assert all(d is None or d == 0 for _, _, d in lanes) and lanes[0][2] == 0, n
        assert sum(d is None for _, _, d in lanes) >= 0.9 * len(lanes), n


def test_the_planner_routes_none_of_them(lanes128):
    import pjd_amd
    datas = [(n, F.falling()[n].data) for n in FALLING] + [(f"broken{k}", j) for k, j in enumerate(F.broken())]
    assert len(datas) >= 7 + 6
    for n, d in datas:
        sc = pjd_amd.Scanned(d)
        assert sc.valid, n
        info = pjd_amd.plan_info([sc.desc])
        assert info["n_sequential"] == 0 and info["sub_bytes"] == 128, (n, info)
        if n in F.falling():
            assert info["n_subsequences"] == F.falling()[n].n_lanes(F.S), (n, info)
    for sh in F.shards():
        sc = pjd_amd.Scanned(sh.data)
        sc.desc.shard_first_seg, sc.desc.shard_n_segs = sh.r0, sh.r1 - sh.r0
        assert pjd_amd.plan_info([sc.desc])["n_sequential"] == 0, sh.name


def test_shard_files_cut_from_the_unbroken_fixtures_are_their_rows_of_the_whole_picture(port):
    """What validates the construction: the file that holds segments [r0, r1) under a frame header of their height decodes, with the
    oracle, to rows [8 * r0, ...) of the oracle's whole picture -- so the same cut of a broken stream is what a shard must write."""
    shards = F.shards()
    assert len(shards) == 6 and sum(s.holds_broken for s in shards) == 4
    assert {s.fixture for s in shards} == set(F.SHARD_FIXTURES)
    for sh in shards:
        whole, part = port.decode(sh.good), port.decode(sh.good_file)
        y0, rows = sh.rows
        assert whole["valid"] and part["valid"] and whole["huff_rc"] == 0 and part["huff_rc"] == 0, sh.name
        assert 0 < rows and y0 + rows <= whole["rgb"].shape[0]
        assert (y0 + rows == whole["rgb"].shape[0]) == (sh.r1 == len(F.restart_marks(sh.good)) + 1)
        assert part["rgb"].shape == (rows,) + whole["rgb"].shape[1:], sh.name
        assert np.array_equal(part["rgb"], whole["rgb"][y0:y0 + rows]), sh.name
        broken = port.decode(sh.file)
        assert broken["valid"], sh.name
        assert sh.holds_broken or np.array_equal(broken["rgb"], part["rgb"])        # the sibling holds none of the changed bytes
    assert any(sh.rows[1] % 8 for sh in shards), "no shard reaches a last MCU row that is cut by the picture's height"


def _flag_takes(data, port):
    info = port.parse(data)["info"]
    return (info["hsamp"], info["vsamp"]) != (1, 2)


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_models_equal_the_host_inlines_on_these_streams(port, s):
    """A seeded sample of units of every stream the flag takes: tests/libjpeg_scaled_model.py's transform of the size the scale asks for
    equals pjd_libjpeg_idct_scaled, and the colour of sampled (Y, Cb, Cr) triples equals pjd_libjpeg_ycc_to_rgb."""
    import pjd_amd
    rng = np.random.default_rng(4200 + s)
    datas = [(n, F.falling()[n].data) for n in FALLING] + [(f"broken{k}", j) for k, j in enumerate(F.broken())]
    n_units = n_pixels = 0
    for name, data in datas:
        if not _flag_takes(data, port):
            continue
        _, coef, (qts, w, h, ncomp, hs, vs) = LC.port_coefficients(port, data)
        grids = M.unit_grids(coef, w, h, ncomp, hs, vs)
        n = 8 // s
        sizes = [n] + [SM.chroma_size(n, hs, vs)] * (ncomp - 1)
        samples = []
        for c in range(ncomp):
            g = grids[c].reshape(-1, 64)
            q = np.asarray(qts[c]).reshape(64)
            pick = rng.choice(len(g), size=min(12, len(g)), replace=False)
            want = SM.idct_units(g[pick], q, sizes[c])
            for k, u in enumerate(pick):
                got = pjd_amd.libjpeg_idct_scaled(g[u], q, sizes[c])
                assert np.array_equal(got, want[k].reshape(-1)), (name, s, c, int(u))
                n_units += 1
            samples.append(want.reshape(-1))
        if ncomp == 3:
            m = min(len(x) for x in samples)
            idx = rng.choice(m, size=min(48, m), replace=False)
            y, cb, cr = (x[idx] for x in samples)
            want = M.ycc_to_rgb(y, cb, cr)
            for k in range(len(idx)):
                assert pjd_amd.libjpeg_ycc_to_rgb(y[k], cb[k], cr[k]) == tuple(int(v) for v in want[k]), (name, s, k)
                n_pixels += 1
    assert n_units >= 200 and n_pixels >= 100, (n_units, n_pixels)      # at 1/8 a unit is one sample: 12 triples a colour stream
