"""Hand-built entropy streams (tests/jpeg_symbols.py, tests/symbol_corpus.py) against the oracle port, the live reference and the
step bound that sizes the lane regions (CPU only).

Each stream is written from symbol tokens, and its intent -- the status class, the first erring unit, every coefficient -- follows from
the tokens alone.  The port (oracle/jpeg_port.c) must equal the intent; where oracle/_ref is built, the reference's own decoder must
equal the port."""
import functools
import itertools

import numpy as np
import pytest

import jpeg_symbols as J
import symbol_corpus as SC
from conftest import golden_bytes


@functools.lru_cache(maxsize=1)
def fixtures():
    return SC.fixtures()


@functools.lru_cache(maxsize=1)
def corpus():
    return SC.corpus()


FIXTURE_NAMES = sorted(SC.fixtures())


def check_port(port, data, fr, it, label):
    port.standard_zigzag(fr.standard_zigzag)          # the frame is decoded with T.81's map (PJD_F_STANDARD_ZIGZAG)
    try:
        o = port.decode(data)
    finally:
        port.standard_zigzag(False)
    assert o["valid"], label
    assert o["huff_rc"] == it.status, (label, o["huff_rc"], it.status)
    want = J.intent_buffer(fr, it)
    assert o["coef"].shape == want.shape, label
    bad = np.argwhere(o["coef"] != want)
    assert bad.size == 0, (label, "first differing (dpu, index)", bad[:4].tolist())
    return o


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_fixture_is_committed_and_port_equals_intent(port, name):
    data, fr, it = fixtures()[name]
    assert golden_bytes(name) == data, "tests/golden/make_fixtures.py writes what symbol_corpus.fixtures() builds"
    check_port(port, data, fr, it, name)


def test_corpus_port_equals_intent(port):
    n_err = 0
    for label, data, fr, it in corpus():
        if fr.standard_restart and (fr.hs, fr.vs) != (1, 1) and fr.ri:
            continue              # written with T.81's restart rule, which the reference does not follow (the GPU test decodes these)
        check_port(port, data, fr, it, label)
        n_err += it.status != 0
    assert n_err > 50


def test_live_reference_equals_port(port, live_ref, tmp_path):
    """The reference's own read_JPEG + decode_Huffman_data (coefficients, status) and its CLI (stdout, BMP) against the port."""
    if live_ref is None:
        pytest.skip("oracle/_ref not built (the fixtures' manifest entries pin the port to it)")
    items = [(n, d) for n, (d, _, _) in fixtures().items()] + [(lab, d) for lab, d, _, _ in corpus()[::3]]
    items += [(n, d) for n, (d, _, _) in SC.edge_family().items() if n not in SC.COMMITTED_EDGE]     # every int16-edge stream
    for k, (label, data) in enumerate(items):
        jp, bp = tmp_path / f"s{k}.jpg", tmp_path / f"s{k}.bmp"
        jp.write_bytes(data)
        r = live_ref.parse_and_huffman(str(jp))
        o = port.decode(data, name=str(jp))
        assert bool(r["info"]["valid"]) == o["valid"], label
        assert np.array_equal(r["coef"], o["coef"]), label
        assert bool(r["huff_ok"]) == (o["huff_rc"] == 0), label
        rc, out = live_ref.run_cli(str(jp), str(bp))
        assert rc == 0 and out == o["log"], (label, out, o["log"])
        assert bp.read_bytes() == o["bmp"], label


REQUIRED_FORMS = (
    [f"ac_size0_run_{r}" for r in range(1, 16)]
    + ["lands_on_63", "ac_run_to_64", "no_eob", "explicit_zero_slot52_after_48", "nonzero_slot52_after_48",
       "dc11_bits_zero", "dc11_bits_ones", "dc_wrap_up", "dc_wrap_down", "ac10_1023", "ac10_-1023", "ac10_512", "ac10_-512",
       "mostly_ones", "restart", "raw_dc", "raw_ac", "dc_sym_ff", "ac_sym_ff", "cut_in_code", "cut_in_dc_bits", "cut_in_ac_bits",
       "end_at_unit_boundary"]
    + [f"dc_size_{s}" for s in range(12, 16)] + [f"ac_size_{s}" for s in range(11, 16)]
    # int16 edges: absolute DCs at -32768 (in every component and sampling, both ways, at the last unit, after a restart, beside
    # either kind of slot 52, odd and even DC quantisers in 8- and 16-bit tables), 32767 and -32767; dequantised products at the edges
    + ["dc_abs_min", "dc_abs_max", "dc_abs_min_plus1", "dc_abs_min_by_descent", "dc_abs_min_by_wrap", "dc_abs_min_last_unit",
       "dc_abs_min_after_restart", "dc_abs_min_zero52", "dc_abs_min_value52", "dc_abs_min_q_odd", "dc_abs_min_q_even"]
    + [f"dc_abs_min_{c}" for c in ("y", "cb", "cr")] + [f"dc_abs_min_{s}" for s in ("grey", "444", "422", "420", "440")]
    + [f"dc_abs_min_q{q}_{b}bit" for q, b in [(1, 8), (3, 8), (2, 8), (32767, 16), (65535, 16), (32768, 16)]]
    + [f"deq_{e}_nat{n}" for e in ("min", "max", "minp1") for n in ("0", "1", "38_slot48", "38_slot52", "58", "63")])


def test_coverage_of_forms_statuses_tables_and_frames():
    """Every symbol form, error class, table shape and frame the issue lists occurs in the fixtures and corpus, so that a later edit
    cannot drop one quietly."""
    items = [(n, d, fr, it) for n, (d, fr, it) in fixtures().items()] + corpus()
    forms, statuses, err_where = set(), set(), set()
    tables, frames = set(), set()
    for label, data, fr, it in items:
        forms |= it.forms
        statuses.add(it.status)
        if it.status:
            u = it.err_unit
            per = len(fr.unit_comps())
            if u == 0:
                err_where.add("first")
            if u == fr.n_units() - 1:
                err_where.add("last")
            if fr.ri and u // per in fr.restarts_before() and u % per == 0:
                err_where.add("after_restart")
        for t in list(fr.dc.values()) + list(fr.ac.values()):
            if sum(t.counts) == 1:
                tables.add("single_code")
            if t.counts[15] == len(t.symbols):
                tables.add("all_16_bit")
            if t.counts[8] and t.counts[9]:
                tables.add("codes_9_and_10")
            if len(t.symbols) == 162:
                tables.add("162_symbols")
            if SC.kraft(t.counts) < 1:
                tables.add("incomplete")
            if 0xFF in t.symbols:
                tables.add("holds_ff")
            if len(set(t.symbols)) < len(t.symbols):
                tables.add("duplicates")
        dcs, acs = [c.td for c in fr.comps], [c.ta for c in fr.comps]
        if len(set(zip(dcs, acs))) == 3 and len(fr.dc) == 4 and len(fr.ac) == 4:
            tables.add("ids_0_3")
        if any(dcs[a] == dcs[b] and acs[a] != acs[b] for a, b in itertools.combinations(range(len(dcs)), 2)):
            tables.add("shared_dc_not_ac")
        if any(acs[a] == acs[b] and dcs[a] != dcs[b] for a, b in itertools.combinations(range(len(dcs)), 2)):
            tables.add("shared_ac_not_dc")
        sub = {(1, 1, 1): "grey", (1, 1, 3): "444", (2, 1, 3): "422", (2, 2, 3): "420", (1, 2, 3): "440"}[(fr.hs, fr.vs, len(fr.comps))]
        frames.add(sub)
        frames.add(f"{fr.width}x{fr.height}")
        mcux = (fr.width + 8 * fr.hs - 1) // (8 * fr.hs)
        if fr.ri == 1:
            frames.add("ri_1")
        if fr.ri and fr.ri == mcux and mcux > 1:
            frames.add("ri_row")
        if fr.ri in (5, 7, 23, 38) and fr.ri != mcux:
            frames.add("ri_prime" if fr.ri != 38 else "ri_other")
        if fr.ri and fr.standard_restart and (fr.hs, fr.vs) != (1, 1):
            frames.add(f"std_restart_{sub}")
    missing = [f for f in REQUIRED_FORMS if f not in forms]
    assert not missing, missing
    assert statuses == set(range(8)), statuses
    assert err_where == {"first", "last", "after_restart"}, err_where
    want_tables = {"single_code", "all_16_bit", "codes_9_and_10", "162_symbols", "incomplete", "holds_ff", "duplicates", "ids_0_3",
                   "shared_dc_not_ac", "shared_ac_not_dc"}
    assert want_tables <= tables, want_tables - tables
    want_frames = {"grey", "444", "422", "420", "440", "1x1", "8x8", "17x9", "1x300", "300x1", "ri_1", "ri_row", "ri_prime",
                   "std_restart_420", "std_restart_422", "std_restart_440"}
    assert want_frames <= frames, want_frames - frames


# ---- the step bound, realised -----------------------------------------------------------------------------------------------------
LANE_SLACK_STEPS = 48           # pjd_internal.h PJD_LANE_SLACK_STEPS


def _table(h):
    """pjd_huff_table (offsets, symbols) -> jpeg_symbols.Table."""
    return J.Table([h.offsets[i + 1] - h.offsets[i] for i in range(16)], list(h.symbols[:h.offsets[16]]))


def _frame_like(desc, w, h):
    """A frame with the sampling and Huffman tables of a scanned picture."""
    sub = {(1, 1, 1): "grey", (1, 1, 3): "444", (2, 1, 3): "422", (2, 2, 3): "420", (1, 2, 3): "440"}[(desc.h_samp, desc.v_samp, desc.num_components)]
    dc = {i: _table(desc.dc[i]) for i in sorted({desc.comp_dc[c] for c in range(desc.num_components)})}
    ac = {i: _table(desc.ac[i]) for i in sorted({desc.comp_ac[c] for c in range(desc.num_components)})}
    return SC.frame(w, h, sub, dc, ac, assign=[(desc.comp_dc[c], desc.comp_ac[c]) for c in range(desc.num_components)])


def bound_cases():
    """(label, frame) at the density bound: the Annex-K and fitted table sets of tests/test_planner_bound.py and the adversarial
    tables of the corpus, each frame filled with its components' cheapest units."""
    import pjd_amd
    import test_planner_bound
    out = []
    for label, jpeg in test_planner_bound._cases():
        s = pjd_amd.Scanned(jpeg)
        out.append((label, _frame_like(s.desc, 256, 192)))
    for dn, an in [("single", "ones"), ("ones", "ones"), ("dup", "edge9_10"), ("general", "all16"), ("single", "general"),
                   ("ones", "all162")]:
        out.append((f"{dn}+{an} grey", SC.frame(256, 192, "grey", {0: SC.TABLES_DC[dn]()}, {0: SC.TABLES_AC[an]()})))
        out.append((f"{dn}+{an} 4:2:0", SC.frame(256, 192, "420", {0: SC.TABLES_DC[dn](), 1: SC.dc_single(0)},
                                                 {0: SC.TABLES_AC[an](), 1: SC.ac_ones()})))
    return out


def _steps(fr, units):
    return sum(SC.unit_steps(SC.unit_symbols(u, *SC.tables_of(fr, k))) for k, u in enumerate(units))


def test_streams_at_the_step_bound_fit_their_lanes():
    """Lane regions hold 8 * S / mu + PJD_LANE_SLACK_STEPS steps (mu = pjd_plan_step_bits).  A stream that repeats the cheapest units its
    tables allow, written for real, takes no more steps than that: counted with a pairing counter that takes every pair (an upper
    bound of the write pass, which may break a pair at a lane end but never makes one the format does not allow)."""
    import pjd_amd
    for label, fr in bound_cases():
        units = SC.dense_frame(fr)
        data, it = J.write(fr, units)
        s = pjd_amd.Scanned(data)
        assert s.valid and it.status == J.OK, label
        mu = pjd_amd.plan_step_bits(s.desc)
        nbytes = int(s.desc.ecs_len)
        steps = _steps(fr, units)
        assert steps <= 8 * nbytes / mu + LANE_SLACK_STEPS, (label, steps, nbytes, mu)
        assert steps * mu <= 8 * nbytes, (label, steps, nbytes, mu)       # whole units are closed walks of the step graph: no slack needed


@pytest.mark.parametrize("dc_syms,ac_syms", [
    ({1: [0], 2: [1]}, {1: [0x00], 2: [0x01], 3: [0xF0]}),
    ({1: [2]}, {2: [0x00, 0x11], 3: [0x01, 0xE0, 0xF0], 4: [0x02, 0x0B]}),
    ({2: [0, 1, 0xFF], 3: [3]}, {1: [0x01], 3: [0x00, 0xF0, 0xFF], 9: [0x21, 0x13], 10: [0x0A, 0xD0]}),
])
def test_every_short_unit_of_tiny_tables_respects_the_step_bound(dc_syms, ac_syms):
    """Brute force over tiny tables (with invalid symbols among them): every unit of up to four AC symbols, with or without an EOB,
    consumes at least mu bits per step.  Pairs never reach across units, so this covers every sequence of such units."""
    import pjd_amd
    dct, act = J.table_from_lengths(dc_syms), J.table_from_lengths(ac_syms)
    fr = SC.frame(8, 8, "grey", {0: dct}, {0: act})
    data, _ = J.write(fr, [next(SC.unit_shapes(dct, act))])
    s = pjd_amd.Scanned(data)                 # keep it alive: the descriptor points into it
    mu = pjd_amd.plan_step_bits(s.desc)
    best = min(SC.bits_per_step(u, dct, act) for u in SC.unit_shapes(dct, act, max_ac=4, n_dc=99, n_ac=99))
    assert best >= mu, (best, mu)
    assert best <= mu + 2, (best, mu)         # and the bound is not far below what a real unit can do
