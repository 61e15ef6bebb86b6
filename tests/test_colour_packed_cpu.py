"""The arithmetic of the colour stage's packed fast path and of the division-free unit tables (pjd_colour_store, pjd_idct_range in
pim-jpeg-decoder_amd/csrc/pjd_k_backend.hip; the named instructions in pjd_device_common.h), modelled in numpy and compared with the
formula of pjd_ycc_to_rgb (reference src/decoder_dpu.c:376-382).  No GPU.

* saturating int16 add, then saturation to uint8, equals clamp255(y + term + 128) for EVERY int16 luma whenever the chroma samples
  are in [-16384, 16383] -- and does not outside (so the range test is needed);
* a task goes to the 32-bit path exactly when a chroma sample is outside that range;
* the reciprocal multiply that replaces the divisions of the unit tables is exact over its whole domain;
* the pictures of tests/test_gpu_colour_packed.py hold chroma samples on both sides of each edge of the range."""
import itertools

import numpy as np

import colour_packed_cases as M

EDGE = [-32768, -32767, -16385, -16384, -16383, -1, 0, 1, 16382, 16383, 16384, 32767]
Y_ALL = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)


def _pairs(y):
    """Every int16 luma as the low half of a pair and as the high half (the other half runs the opposite way)."""
    return np.stack([y, y[::-1]], axis=-1)


def test_packed_sum_equals_clamp_for_every_luma_when_chroma_is_in_range():
    y01 = _pairs(Y_ALL)
    n_in = 0
    for cb, cr in itertools.product(EDGE, EDGE):
        if not M.in_range(cb, cr):
            continue
        n_in += 1
        assert all(-32768 <= int(t) <= 32767 for t in M.chroma_terms(cb, cr)), (cb, cr)       # the terms fit int16
        c = np.full(y01.shape, cb, np.int16), np.full(y01.shape, cr, np.int16)
        for got, want in zip(M.fast_path_rgb(y01, *c), M.reference_rgb(y01, *c)):
            assert np.array_equal(got, want), (cb, cr)
    assert n_in == 7 * 7                                                                     # -16384 .. 16383 of EDGE, squared


def test_packed_sum_with_two_different_chroma_samples_in_a_pair():
    """4:4:4 and 4:4:0 pack the terms of two different chroma samples into one dword: the halves must not interact."""
    y01 = _pairs(Y_ALL)
    inside = [v for v in EDGE if M.in_range(v)]
    for (cb0, cr0), (cb1, cr1) in zip(itertools.product(inside, inside), itertools.product(inside[::-1], inside[2:] + inside[:2])):
        cb = np.broadcast_to(np.array([cb0, cb1], np.int16), y01.shape)
        cr = np.broadcast_to(np.array([cr0, cr1], np.int16), y01.shape)
        for got, want in zip(M.fast_path_rgb(y01, cb, cr), M.reference_rgb(y01, cb, cr)):
            assert np.array_equal(got, want), (cb0, cr0, cb1, cr1)


def test_outside_the_range_the_packed_sum_can_differ():
    """Why the range test exists: with chroma at the int16 extremes a term no longer fits int16 and the packed sum is wrong for
    some luma.  (Not every sample outside the range breaks it: the range is the sufficient condition the kernel tests.)"""
    y01 = _pairs(Y_ALL)
    wrong = 0
    for cb, cr in [(32767, 0), (-32768, 0), (0, 32767), (0, -32768), (-32768, -32768), (32767, 32767)]:
        assert not M.in_range(cb, cr)
        c = np.full(y01.shape, cb, np.int16), np.full(y01.shape, cr, np.int16)
        wrong += any(not np.array_equal(g, w) for g, w in zip(M.fast_path_rgb(y01, *c), M.reference_rgb(y01, *c)))
    assert wrong >= 4


def test_a_task_takes_the_slow_path_exactly_when_a_sample_is_outside_the_range():
    allv = np.arange(-32768, 32768, dtype=np.int64)
    assert np.array_equal(M.in_range(allv), (allv >= M.LO) & (allv <= M.HI))                 # the bit test, every int16
    for group in itertools.product(EDGE, repeat=2):                                           # the samples of a task: any one decides
        for others in [(0, 0), (M.HI, M.LO)]:
            assert bool(M.in_range(*group, *others)) == all(M.LO <= v <= M.HI for v in group)
    # the terms' bounds quoted in pjd_device_common.h
    r, g, b = M.chroma_terms(np.array([M.LO, M.HI, M.LO, M.HI]), np.array([M.LO, M.LO, M.HI, M.HI]))
    assert np.abs(r).max() <= 23100 and np.abs(b).max() <= 29162 and np.abs(g).max() <= 17465


def test_reciprocal_division_is_exact_over_its_domain():
    u = np.arange(160, dtype=np.int64)
    for d in range(1, 11):                                                                    # unit -> MCU of the range
        assert np.array_equal(M.div_small(u, d), u // d), d
    i = np.arange(7 * 96, dtype=np.int64)                                                     # row task -> unit (rows 1..7 of 96 units)
    assert np.array_equal(M.div_small(i, 7), i // 7)
    assert [-(-65536 // d) for d in range(1, 11)] == [65536, 32768, 21846, 16384, 13108, 10923, 9363, 8192, 7282, 6554]   # c_recip16


def test_the_gpu_pictures_hold_samples_on_both_sides_of_each_edge(port):
    """The premise of tests/test_gpu_colour_packed.py, checked with the oracle port's IDCT: in the 4:4:4 and the 4:2:0 picture the
    chroma blocks hold groups of four samples inside the range that touch its ends, groups with one sample just outside, and the
    int16 extremes; luma reaches -32768 and 32767; in-range and out-of-range chroma blocks are neighbours in an MCU row."""
    for w, h, sub in [(80, 112, "420"), (72, 40, "444")]:
        data, fr, it, names = M.picture(w, h, sub)
        s = M.samples_after_idct(port, data, fr, it).astype(np.int32)
        luma, chroma = s[:, :, :4], s[:, :, 4:].reshape(-1, 8, 2, 4)                          # chroma: rows x two groups of four
        assert luma.max() == 32767 and luma.min() == -32768
        mx, mn = chroma.max(-1), chroma.min(-1)
        inside = (mn >= M.LO) & (mx <= M.HI)
        n_out = ((chroma > M.HI) | (chroma < M.LO)).sum(-1)
        assert (inside & (mx == M.HI)).any() and (inside & (mn == M.LO)).any()
        assert ((mx == M.HI + 1) & (n_out == 1)).any() and ((mn == M.LO - 1) & (n_out == 1)).any()
        assert chroma.max() == 32767 and chroma.min() == -32768
        # also as pairs (the two chroma samples under four pixels when luma is sampled twice horizontally)
        pairs = chroma.reshape(-1, 2)
        ok = (pairs.min(-1) >= M.LO) & (pairs.max(-1) <= M.HI)
        assert (ok & (pairs.max(-1) == M.HI)).any() and (ok & (pairs.min(-1) == M.LO)).any()
        per = len(fr.unit_comps())
        cb_names = [names[m * per + per - 2] for m in range(len(fr.mcus()))]
        assert any(a.startswith("in_") and b.startswith("out_") for a, b in zip(cb_names, cb_names[1:]))
