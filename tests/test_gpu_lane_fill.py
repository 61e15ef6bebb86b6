"""GPU: pictures whose subsequence size is no multiple of 64 bytes decode like any other (run with -m gpu on an MI355X).

The planner gives every picture the subsequence size S that fills its waves best, in steps of 16 bytes (pjd_plan.cpp;
tests/test_planner_fill.py).  The kernels take S from the picture: word rows (S / 4 + 8, a multiple of 4), checkpoint spacing
(2 S bits), walker threshold, lane regions.  A small batch plans at 128 bytes, so its pictures come out at 128, 144, 160 or 176."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def pictures(port):
    """Eight dense 4:2:0 pictures of about 200 x 152 with fitted tables and one 4:4:4 picture with a restart interval per MCU row
    (1 x 1 luma: the reference's restart rule is the standard one there), scanned; the oracle's answers; each picture's own S."""
    import pjd_amd
    import synth
    D = synth.DENSE_DETAIL
    jpegs = [synth.make(200 + 3 * k, 152 - 5 * k + 8 * (k % 3), 40 + k, (88, 92, 95, 97)[k % 4], synth.SUB_420, 0, D, True) for k in range(8)]
    jpegs.append(synth.make(203, 149, 50, 95, synth.SUB_444, (203 + 7) // 8, D, True))
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    assert all(s.valid for s in scanned)
    want = [port.decode(j) for j in jpegs]
    sizes = []
    for s in scanned:
        info = pjd_amd.plan_info([s.desc])
        assert info["n_sequential"] == 0 and info["n_subsequences"] > 32       # the per-picture choice applies
        sizes.append(info["sub_bytes"])
    return jpegs, scanned, want, sizes


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for k in ("PJD_SUB_BYTES", "PJD_PLAN_MODE", "PJD_ODD_WAVE_PCT", "PJD_WALK_MAX"):
        monkeypatch.delenv(k, raising=False)


def _check(b, want, which):
    b.upload(); b.decode(); b.sync()
    outs, st = b.download()
    info = b.info()
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0 and sum(info["flag_waves"]) == 0, info["flag_waves"]
    for k, i in enumerate(which):
        assert st[k] == want[i]["huff_rc"] == 0, i
        assert np.array_equal(outs[k], want[i]["rgb"]), i
        assert np.array_equal(b.coefficients(k), want[i]["coef"]), i
    return info


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_batch_with_odd_subsequence_sizes(pictures, mode):
    import pjd_amd
    jpegs, scanned, want, sizes = pictures
    assert all(S in (128, 144, 160, 176) for S in sizes), sizes
    assert any(S % 64 for S in sizes), sizes
    c = pjd_amd.Context(0, plan_mode=pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
    try:
        with c.batch([s.desc for s in scanned]) as b:
            info = _check(b, want, range(len(jpegs)))
            assert info["sub_bytes"] == max(sizes)
            assert info["n_subsequences"] <= 64 * info["n_huff_waves"]
    finally:
        c.close()


@pytest.mark.parametrize("walk_max", ["0", "32"])
def test_one_picture_alone_with_the_walker_off_and_wide(pictures, monkeypatch, walk_max):
    import pjd_amd
    jpegs, scanned, want, sizes = pictures
    i = next(k for k, S in enumerate(sizes) if S % 64)
    monkeypatch.setenv("PJD_WALK_MAX", walk_max)
    c = pjd_amd.Context(0)
    try:
        with c.batch([scanned[i].desc]) as b:
            info = _check(b, want, [i])
            assert info["sub_bytes"] == sizes[i]
            assert (info["walks"] == 0) if walk_max == "0" else (info["walk_lanes"] >= info["walks"])
    finally:
        c.close()
