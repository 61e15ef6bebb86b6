"""How full the planner makes the entropy decoder's waves (pjd_plan.cpp, the per-picture subsequence size).

A wave holds lanes of one picture and every pass of it costs what 64 lanes cost, so the planner moves each picture's subsequence
size S to where its lanes fill whole waves: the cheapest in wave-bytes (waves x S) of the nearest wave count, one more and one
fewer, S a multiple of 16 bytes.  Host only, through pjd_plan_info: the totals of a batch (lanes, waves) and, for a picture
planned alone, its own S (a batch's sub_bytes is the largest S of its pictures)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

S_MIN, S_MAX = 128, 1024


@pytest.fixture(scope="module")
def default_set():
    """256 pictures of bench.py's default generator (seed 3; without the bundled picture, which takes a GPU decode), scanned."""
    import pjd_amd
    import synth
    jpegs = synth.cfg3_imagenet_like(256, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    assert all(s.valid for s in scanned)
    return scanned


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for k in ("PJD_SUB_BYTES", "PJD_PLAN_MODE", "PJD_ODD_WAVE_PCT"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_fill_on_the_default_set(default_set, monkeypatch, mode):
    import pjd_amd
    monkeypatch.setenv("PJD_PLAN_MODE", mode)
    info = pjd_amd.plan_info([s.desc for s in default_set])
    assert info["plan_mode"] == (1 if mode == "throughput" else 0) and info["n_sequential"] == 0
    fill = info["n_subsequences"] / (64.0 * info["n_huff_waves"])
    print(f"{mode}: {info['n_subsequences']} lanes in {info['n_huff_waves']} waves, fill {fill:.4f}")
    assert fill >= 0.96, (mode, fill)


def test_per_picture_plans(default_set):
    """Every picture planned alone: its S is a multiple of 16 within the limits (a batch this small plans at 128 bytes, so within
    128..176: -30 % / +45 %, and never under the lower limit), its lanes fit its waves, and they are what S cuts its stream into."""
    import pjd_amd
    sizes = set()
    for s in default_set[:64]:
        info = pjd_amd.plan_info([s.desc])
        S, lanes, waves = info["sub_bytes"], info["n_subsequences"], info["n_huff_waves"]
        assert S % 16 == 0 and S_MIN <= S <= min(S_MAX, 128 * 29 // 20), S
        assert lanes <= 64 * waves and waves == (lanes + 63) // 64
        assert lanes == (int(s.desc.ecs_len) + S - 1) // S
        sizes.add(S)
    assert any(S % 64 for S in sizes), sizes          # the 16-byte steps are used


def test_restart_segments():
    """One restart interval per MCU row: lanes are cut per segment (none crosses a restart marker), whatever S the picture got."""
    import pjd_amd
    import synth
    for sub, flags in ((synth.SUB_444, 0), (synth.SUB_420, pjd_amd.F_STANDARD_RESTART)):
        w, h = 400, 304
        mcux = (w + (15 if sub == synth.SUB_420 else 7)) // (16 if sub == synth.SUB_420 else 8)
        s = pjd_amd.Scanned(synth.make(w, h, 21, 95, sub, mcux, synth.DENSE_DETAIL, True))
        assert s.valid
        s.desc.flags = int(s.desc.flags) | flags
        info = pjd_amd.plan_info([s.desc])
        assert info["n_sequential"] == 0
        S = info["sub_bytes"]
        assert S % 16 == 0 and S_MIN <= S <= S_MAX
        offs = [int(x) for x in s.seg_offsets()] + [int(s.desc.ecs_len)]
        assert len(offs) - 1 == (h + (15 if sub == synth.SUB_420 else 7)) // (16 if sub == synth.SUB_420 else 8)
        want = sum(max(1, (b - a + S - 1) // S) for a, b in zip(offs, offs[1:]))
        assert want > 32                               # enough lanes for the per-picture choice to apply
        assert info["n_subsequences"] == want
        assert info["n_subsequences"] <= 64 * info["n_huff_waves"]


def test_override(default_set, monkeypatch):
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    descs = [s.desc for s in default_set[:8]]
    info = pjd_amd.plan_info(descs)
    assert info["sub_bytes"] == 128
    assert info["n_subsequences"] == sum((int(d.ecs_len) + 127) // 128 for d in descs)
    for s in default_set[:8]:
        assert pjd_amd.plan_info([s.desc])["sub_bytes"] == 128
