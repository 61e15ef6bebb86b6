"""Hand-built entropy streams on the GPU (run with -m gpu on an MI355X): the seeded corpus of tests/symbol_corpus.py in one batch on the
parallel path (both plan modes, 128-byte lanes) and on the exact kernel, errors planted at lane and checkpoint edges, and the routing.
Status, pictures and coefficients must equal the streams' intent (tests/jpeg_symbols.py) and, where the reference's restart rule
applies, the oracle port."""
import functools

import numpy as np
import pytest

import jpeg_symbols as J
import symbol_corpus as SC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def corpus():
    return SC.corpus()


def intent_rgb(port, data, fr, it):
    """The intent's coefficients through the port's back end (dequantisation, IDCT, colour) -> the picture."""
    o = port.parse(data)
    meta = o["metadata"]
    mcus = J.intent_buffer(fr, it).copy()
    for d in range(mcus.shape[0]):
        port.dpu_exec(meta, mcus[d])
    rgb = np.zeros((fr.height, fr.width, 3), np.uint8)
    port.L.orc_rgb_from_mcus(meta.ctypes.data, mcus.ctypes.data, rgb.ctypes.data)
    return rgb


def _scan(items, force_sequential=False):
    import pjd_amd
    scanned = []
    for label, data, fr, it in items:
        s = pjd_amd.Scanned(data)
        assert s.valid, label
        s.desc.flags = ((pjd_amd.F_STANDARD_RESTART if fr.standard_restart else 0) | (pjd_amd.F_FORCE_SEQUENTIAL if force_sequential else 0)
                        | (pjd_amd.F_STANDARD_ZIGZAG if fr.standard_zigzag else 0))
        scanned.append(s)
    return scanned


def _decode_and_check(ctx, port, items, scanned, check_routing=True):
    with ctx.batch([s.desc for s in scanned]) as b:
        b.upload(); b.decode(); b.sync()
        outs, st = b.download()
        info = b.info()
        for k, (label, data, fr, it) in enumerate(items):
            assert st[k] == it.status, (label, st[k], it.status)
            coef = b.coefficients(k)
            want = J.intent_buffer(fr, it)
            bad = np.argwhere(coef != want)
            assert bad.size == 0, (label, "coefficients differ from the intent at", bad[:4].tolist())
            port.standard_zigzag(fr.standard_zigzag)            # a frame decoded with T.81's map (PJD_F_STANDARD_ZIGZAG)
            try:
                assert np.array_equal(outs[k], intent_rgb(port, data, fr, it)), label
                if not (fr.standard_restart and fr.ri and (fr.hs, fr.vs) != (1, 1)):
                    assert np.array_equal(outs[k], port.decode(data)["rgb"]), label
            finally:
                port.standard_zigzag(False)
    if check_routing:
        assert info["n_sequential"] == sum(SC.expect_sequential(fr, it) for _, _, fr, it in items), info["n_sequential"]
        assert info["n_fallback"] == 0, info["flag_waves"]
        if all(it.status == J.OK for *_, it in items):
            # a wave may be flagged behind an entropy-coding error (a restart segment that then ends early): that costs nothing, as the
            # decode stops at the error; in a batch without errors any flagged wave is a slow path nobody asked for
            assert sum(info["flag_waves"]) == 0, info["flag_waves"]
    return info


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_corpus_one_batch_parallel_path(port, mode):
    """~300 streams of every symbol form, table shape, frame and error class in ONE batch: status, pictures and coefficients equal the
    intent; every stream whose tables and restart layout the planner takes stays on the parallel path (no re-decode, no flagged wave)."""
    import pjd_amd
    items = corpus()
    ctx = pjd_amd.Context(0)
    try:
        ctx.set_plan_mode(pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
        _decode_and_check(ctx, port, items, _scan(items))
        clean = [x for x in items if x[3].status == J.OK]
        assert len(clean) > 150
        _decode_and_check(ctx, port, clean, _scan(clean))
    finally:
        ctx.close()


def test_corpus_one_batch_128_byte_lanes(port, monkeypatch):
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    items = corpus()
    ctx = pjd_amd.Context(0)
    try:
        _decode_and_check(ctx, port, items, _scan(items))
        clean = [x for x in items if x[3].status == J.OK]
        _decode_and_check(ctx, port, clean, _scan(clean))
    finally:
        ctx.close()


def test_corpus_one_batch_exact_kernel(port):
    import pjd_amd
    items = corpus()
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items, force_sequential=True), check_routing=False)
        assert info["n_sequential"] == len(items)
    finally:
        ctx.close()


def test_fixtures_stay_on_the_parallel_path():
    """The committed sym_* fixtures: the planner takes every one of their table sets."""
    import pjd_amd
    for name, (data, fr, it) in SC.fixtures().items():
        assert not SC.expect_sequential(fr, it), name
        s = pjd_amd.Scanned(data)
        assert pjd_amd.plan_info([s.desc])["n_sequential"] == 0, name


def _edge_streams(sub_bytes=128, nchk=4):
    """For every error class: the erring symbol planted so that it starts within +-1 byte of a lane boundary (every sub_bytes of the
    entropy-coded segment) or of a checkpoint boundary (every sub_bytes / nchk) of a long grey stream.  A DC-class error goes into the
    unit after the one that holds the boundary, cut short (EOB) where the boundary lies; an AC-class error after as many of the unit's
    AC symbols as bring it there."""
    rng = np.random.default_rng(4711)
    dct, act = SC.dc_general(), SC.ac_general()
    fr = SC.frame(64, 256, "grey", {0: dct}, {0: act}, assign=[(0, 0)])
    base = SC.fill(fr, rng, p_eob=0.08)
    _, it0 = J.write(fr, base)
    starts = it0.unit_bit + [10 ** 9]
    nbits = lambda t, table: len(J._token_bits(t, table)[0])
    lane, chk = sub_bytes * 8, sub_bytes * 8 // nchk
    bounds = [("lane", b) for b in range(lane, starts[-2], lane)][:5] + [("checkpoint", b) for b in range(chk, starts[-2], chk) if b % lane][:5]
    out = []
    for cls in range(1, 8):
        for kind, b in bounds:
            v = max(u for u in range(len(base)) if starts[u] <= b)
            unit = base[v]
            body = unit[1:-1] if unit[-1] == J.EOB else unit[1:]
            pos = starts[v] + nbits(unit[0], dct)           # where each AC symbol of unit v starts
            cand = []
            for n in range(len(body) + 1):
                cand.append((n, pos))
                if n < len(body):
                    pos += nbits(body[n], act)
            units = [list(x) for x in base]
            if cls in (J.DC_SYM, J.DC_LEN, J.DC_BITS):
                ends = [(n, p + nbits(J.EOB, act)) for n, p in cand]
                n, e = min(ends, key=lambda x: abs(x[1] - b))
                units[v] = unit[:1] + body[:n] + [J.EOB]
                units = SC.plant(fr, units, v + 1, cls, rng, pick=len(out))
            else:
                n, e = min(cand, key=lambda x: abs(x[1] - b))
                units = SC.plant(fr, units, v, cls, rng, keep_n=n, pick=len(out))
            if abs(e - b) > 8:
                continue
            try:
                data, it = J.write(fr, units)
            except (ValueError, AssertionError):
                continue
            out.append((f"{J.STATUS_NAMES[cls]}@{kind}{b}", data, fr, it))
    return out


def test_errors_at_lane_and_checkpoint_edges(port, monkeypatch):
    """Each error class with its erring symbol within a byte of a 128-byte lane boundary or a checkpoint boundary: the lane behind the
    boundary is synchronised as if the stream went on; status, picture and coefficients still equal the intent (the reference stops at
    the error and keeps what the erring unit had), on the parallel path."""
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    items = _edge_streams()
    seen = {it.status for *_, it in items}
    assert seen == set(range(1, 8)), seen
    assert len(items) >= 40, len(items)
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["sub_bytes"] == 128
    finally:
        ctx.close()


def test_streams_at_the_step_bound_stay_on_the_parallel_path(port):
    """The streams of test_symbol_streams.bound_cases() repeat the cheapest units their tables allow, i.e. they run at the density bound
    that sizes the lane regions: no lane may overflow its region (PJD_FLAG_OVERFLOW would mean the bound is wrong), nothing is flagged
    or re-decoded, and the coefficients equal the intent."""
    import test_symbol_streams as T
    import pjd_amd
    items = []
    for label, fr in T.bound_cases():
        data, it = J.write(fr, SC.dense_frame(fr))
        items.append((label, data, fr, it))
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["n_sequential"] == 0
    finally:
        ctx.close()
