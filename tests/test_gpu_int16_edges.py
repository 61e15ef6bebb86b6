"""int16 edges on the GPU (run with -m gpu on an MI355X): the edge family of tests/symbol_corpus.py -- absolute DCs of exactly -32768,
32767 and -32767 in every component and sampling, at the last unit and after restarts, beside an explicit zero and a value at slot 52,
and AC values whose dequantised product is at those values at natural positions 0, 1, 38, 58 (T.81 map) and 63 -- on every decode
path: lane streams (both plan modes, picture groups), the table-driven exact kernel, the literal kernel, up-front routing, reduced-size
output on the lane and dense back ends, and split decode.

The exact kernels keep an absolute DC in slot 0 of the dense scratch and mark an explicit zero at slot 52 with -32768: a DC of -32768
must stay a value there.  Status, pictures and coefficients must equal the streams' intent (tests/jpeg_symbols.py) and, where the
reference's restart rule applies, the oracle port, which follows the reference: (int16)(-32768 * q) is -32768 for an odd quantiser."""
import functools

import numpy as np
import pytest

import jpeg_symbols as J
import symbol_corpus as SC
from test_gpu_scaled import SCALES, box
from test_gpu_symbol_streams import _decode_and_check, _scan, intent_rgb

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def family():
    """[(label, jpeg, frame, intent)]: the fixed edge family and its seeded corpus variants."""
    items = [(n, d, fr, it) for n, (d, fr, it) in SC.edge_family().items()]
    return items + SC.edge_variants(np.random.default_rng(31338), 12)


def _lane_items():
    return [x for x in family() if not SC.expect_sequential(x[2], x[3])]


def _has_dc_min(items):
    return sum("dc_abs_min" in it.forms for *_, it in items)


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_edge_family_one_batch_lane_path(port, mode):
    """The whole family in one batch: the pictures the planner takes stay on the lane streams (no fallback, no flagged wave), the
    routed ones go to the exact kernel; everything equals the intent."""
    import pjd_amd
    items = family()
    assert _has_dc_min(items) >= 20 and sum(SC.expect_sequential(fr, it) for *_, fr, it in items) >= 3
    ctx = pjd_amd.Context(0)
    try:
        ctx.set_plan_mode(pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
        _decode_and_check(ctx, port, items, _scan(items))
    finally:
        ctx.close()


def test_edge_family_picture_groups(port):
    """>= 64 pictures of the lane-path members: the picture-group form of the DC prediction (pjd_k_group_dc) carries the int16 sums."""
    import pjd_amd
    lane = _lane_items()
    items = (lane * (64 // len(lane) + 1))[:max(64, len(lane))]
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["n_sequential"] == 0 and len(items) >= 64
    finally:
        ctx.close()


def test_edge_family_exact_kernel(port):
    """PJD_F_FORCE_SEQUENTIAL: every picture through the table-driven exact kernel and the dense back end, where slot 0 holds the
    absolute DC beside the slot-52 mark."""
    import pjd_amd
    items = family()
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items, force_sequential=True), check_routing=False)
        assert info["n_sequential"] == len(items)
    finally:
        ctx.close()


def test_edge_family_literal_kernel(port):
    """Every DC frame of the family rebuilt with an over-subscribed AC table, which the planner gives no decode table: the literal
    kernel (pjd_k_huff_sequential) decodes them all."""
    import pjd_amd
    rng = np.random.default_rng(65535)
    items = []
    for name, (w, h, sub, q, q16, ri, std, _) in SC.DC_EDGE_FRAMES.items():
        fr = SC.edge_frame(w, h, sub, q, q16, ri=ri, std=std, ac={0: SC.ac_oversub(), 1: SC.ac_oversub()})
        data, it = J.write(fr, SC.dc_edge_units(fr, rng))
        assert not SC.tables_fit(fr)
        items.append((name + ":oversub", data, fr, it))
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["n_sequential"] == len(items)
    finally:
        ctx.close()


def test_subsampled_restart_under_the_reference_rule_is_routed(port):
    """Subsampled luma with DRI under the reference's restart rule: routed to the exact kernel up front, equal to the port."""
    import pjd_amd
    items = [x for x in family() if x[2].ri and not x[2].standard_restart and (x[2].hs, x[2].vs) != (1, 1)]
    assert len(items) >= 2 and all(SC.expect_sequential(fr, it) for *_, fr, it in items)
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["n_sequential"] == len(items)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["lanes", "dense"])
def test_edge_family_scaled(port, mode):
    """PJD_F_SCALE_1_2 / _1_4 / _1_8 on the lane back end and on the dense one (pjd_k_idct_colour<true>): the box filter of the
    intent's picture, in one batch with the full-size pictures."""
    import pjd_amd
    items = family()
    want = {}
    for label, data, fr, it in items:
        port.standard_zigzag(fr.standard_zigzag)
        try:
            want[label] = intent_rgb(port, data, fr, it)
        finally:
            port.standard_zigzag(False)
    rows, scanned = [], []
    for flags, s in [(0, 1)] + SCALES:
        for x, sc in zip(items, _scan(items, force_sequential=mode == "dense")):
            sc.desc.flags = int(sc.desc.flags) | flags
            rows.append((x, s))
            scanned.append(sc)
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([sc.desc for sc in scanned]) as b:
            b.upload(); b.decode()
            outs, st = b.download()
            info = b.info()
    finally:
        ctx.close()
    for k, ((label, data, fr, it), s) in enumerate(rows):
        assert st[k] == it.status, (label, s)
        assert np.array_equal(outs[k], box(want[label], s)), (label, s)
    if mode == "dense":
        assert info["n_sequential"] == len(scanned)
    else:
        assert info["n_fallback"] == 0


def test_split_decode_of_restart_segmented_edge_pictures(port, monkeypatch):
    """pjd_split_decode of the restart-segmented 4:4:4 and grey edge pictures (the predictor restarts at 0 in each segment, a range
    starts on a segment): the same picture as the unsplit decode and as the intent, at full size and at 1/2."""
    import pjd_amd
    monkeypatch.setenv("PJD_PIPE_ALLOW_DUP_DEVICES", "1")
    F = SC.edge_family()
    ctx = pjd_amd.Context(0)
    try:
        for name in ("sym_edge_dc_444_q3_ri21", "sym_edge_dc_grey_q1_ri24", "sym_edge_dc_grey_q2_ri21"):
            data, fr, it = F[name]
            want = intent_rgb(port, data, fr, it)
            for flags, s in [(0, 1), SCALES[0]]:
                sc = _scan([(name, data, fr, it)])[0]
                sc.desc.flags = int(sc.desc.flags) | flags
                whole, st = ctx.decode([sc.desc], pjd_amd.OUT_RGB8)
                assert st == [0] and np.array_equal(whole[0], box(want, s)), (name, s)
                for world in (2, 3):
                    got, status, stats = pjd_amd.split_decode(sc.desc, [0] * world, pjd_amd.OUT_RGB8)
                    assert status == 0 and stats["n_ranks"] == min(world, int(sc.desc.n_segments)), (name, s, world, stats)
                    assert np.array_equal(got, whole[0]), (name, s, world)
    finally:
        ctx.close()
        pjd_amd.dev_lib().pjd_split_release()


def _progressive_frame(sub, w, h):
    fr = SC.frame(w, h, sub, {0: SC.dc_general()}, {0: SC.ac_162()}, assign=[(0, 0)] * len(SC.SAMPLINGS[sub]))
    fr.standard_zigzag = True
    for t in fr.qt:
        fr.qt[t] = [2 * ((k * 7 + t * 3) % 20) + 1 for k in range(64)]        # odd quantisers: (int16)(-32768 * q) stays -32768
    return fr


def test_progressive_stores_that_truncate_to_int16_min():
    """Progressive frames (tests/jpeg_progressive.py) whose stores truncate to -32768: a DC first scan with pred << 3 at +-4096, a DC
    refinement scan over it, AC first scans at Al = 13 with v = +-4 at slot 52 and elsewhere.  pjd_k_progressive never writes the
    slot-52 mark, so every -32768 is a value.  Decoded with PJD_F_STANDARD_ZIGZAG as test_gpu_parity's baseline-twin test does: the
    coefficient download equals the T.81 G.1.2 model, and the picture equals the oracle port's back end run on the model's
    coefficients.  The four procedures themselves are pinned to the reference's decode_MCU_component by tests/test_progressive_streams.py
    (this writer's full form, a bit-level model, oracle/ref_driver.cpp); the reference cannot decode a progressive FILE."""
    import oracle_lib
    import pjd_amd
    import jpeg_progressive as P
    port = oracle_lib.Port()
    ctx = pjd_amd.Context(0)
    port.standard_zigzag(True)
    try:
        for label, fr, scans in P.edge_streams(_progressive_frame):
            data, it = P.write(fr, scans, SC.dc_general(), SC.ac_162())
            assert (it.slots[:, 52] == -32768).any() and (it.slots[:, 0] == -32768).any() and (it.slots[:, 0] == -32764).any(), label
            twin, _ = J.write(fr, [[J.dcv(0), J.EOB]] * fr.n_units())                  # the same frame as baseline: the port's metadata
            s = pjd_amd.Scanned(data, options=pjd_amd.SCAN_PROGRESSIVE)
            assert s.valid and int(s.desc.n_scans) == len(scans), label
            s.desc.flags = int(s.desc.flags) | pjd_amd.F_STANDARD_ZIGZAG
            with ctx.batch([s.desc]) as b:
                b.upload(); b.decode()
                outs, st = b.download()
                coef = b.coefficients(0)
            assert st == [0], label
            bad = np.argwhere(coef != J.intent_buffer(fr, it))
            assert bad.size == 0, (label, "coefficients differ from the model at", bad[:4].tolist())
            assert np.array_equal(outs[0], intent_rgb(port, twin, fr, it)), label
    finally:
        port.standard_zigzag(False)
        ctx.close()
