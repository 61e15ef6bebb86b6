"""The sized second-level decode tables on the GPU (run with -m gpu on an MI355X): hand-built 64 x 64 4:2:0 pictures whose streams use
a code of every length 10 to 16 in the luma AC, the chroma AC and a DC table, in lanes of 128 bytes, through every reader of the blob --
the passes of the parallel path (lut_lookup_pair), the cooperative walker (WALK_FIX), careful_span behind a planted error and the
table-driven exact kernel -- against the streams' intent and the oracle port; a batch that mixes a table set without a second level
with complete 16-bit trees; and the LDS the entropy decoder asks for, which must be the host builder's largest blob + the wave areas.
tests/test_lut_layout.py checks the tables themselves, window by window, on the CPU."""
import functools

import numpy as np
import pytest

import jpeg_symbols as J
import symbol_corpus as SC
import test_gpu_symbol_streams as G
import test_lut_layout as L

pytestmark = pytest.mark.gpu

LONG = set(range(10, 17))


def _tables():
    # luma AC: one prefix per code length 10..15 and a 16-bit code in a seventh (k = 1..7); chroma AC: a prefix that holds the lengths
    # 10, 11 and 12 and one that holds 13 to 16; DC: '0', '10' and one code of every length 10..16 under ONE prefix
    ac_y = L.ac_table([1, 1, 1, 1, 1, 1, 0, 0, 0, 2, 4, 8, 16, 32, 64, 1])
    ac_c = L.ac_table([1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 2, 4, 8, 16, 32])
    dc_y = J.Table([1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5, 6, 7, 8])
    dc_c = J.Table([1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1], [1, 0, 8, 7, 6, 5, 4, 3, 2])
    return {0: dc_y, 1: dc_c}, {0: ac_y, 1: ac_c}


def _lengths_used(fr, units):
    """{('dc' | 'ac', table id): code lengths the stream uses}."""
    per = fr.unit_comps()
    used = {}
    for u, toks in enumerate(units):
        c = fr.comps[per[u % len(per)]]
        for t in toks:
            if t[0] == "DC":
                used.setdefault(("dc", c.td), set()).add(fr.dc[c.td].code_of[t[1]][0])
            elif t[0] == "AC":
                used.setdefault(("ac", c.ta), set()).add(fr.ac[c.ta].code_of[(t[1] << 4) | t[2]][0])
    return used


def _cover(fr, units):
    """Make the first units of every component use a code of every length 10 to 16 of its DC and its AC table (a random draw may miss
    a length that has a single code)."""
    per = fr.unit_comps()
    for c, comp in enumerate(fr.comps):
        dct, act = fr.dc[comp.td], fr.ac[comp.ta]
        mine = [u for u in range(fr.n_units()) if per[u % len(per)] == c]
        by_len = lambda t, ok: {ln: min((x for x in t.symbols if t.code_of[x][0] == ln and ok(x)), key=lambda x: x >> 4) for ln in LONG}
        dcs, acs = by_len(dct, lambda x: x <= 11), by_len(act, lambda x: 1 <= (x & 15) <= 10)
        bodies, body, slot = [], [], 1
        for ln in sorted(LONG):
            run, size = acs[ln] >> 4, acs[ln] & 15
            if slot + run > 63:
                bodies.append(body + [J.EOB])
                body, slot = [], 1
            body.append(J.AC(run, size, (1 << size) - 1))
            slot += run + 1
        bodies.append(body + ([J.EOB] if slot < 64 else []))
        for k, ln in enumerate(sorted(LONG)):
            u = mine[k]
            units[u] = [J.DC(dcs[ln], 1 if dcs[ln] else 0)] + (bodies[k] if k < len(bodies) else units[u][1:])
    return units


@functools.lru_cache(maxsize=1)
def _streams():
    """[(label, jpeg, frame, intent)]: three clean streams, and two with an error planted right behind a long code."""
    rng = np.random.default_rng(1016)
    dc, ac = _tables()
    out = []
    for k in range(3):
        fr = SC.frame(64, 64, "420", dc, ac, ri=(0, 0, 5)[k], std=k == 2)
        units = _cover(fr, SC.fill(fr, rng, p_eob=0.2))
        used = _lengths_used(fr, units)
        for key in (("ac", 0), ("ac", 1), ("dc", 0), ("dc", 1)):
            assert LONG <= used[key], (key, used[key])
        data, it = J.write(fr, units)
        assert it.status == J.OK
        out.append((f"clean{k}", data, fr, it))
        if k == 2:
            continue
        # an error right behind a 16-bit code, in the second half of the stream: the lane that meets it decodes its whole subsequence,
        # long codes included, with careful_span
        cls = (J.AC_SYM, J.DC_SYM)[k]
        u = fr.n_units() // 2 + 1 + k
        act = SC.tables_of(fr, u)[1]
        sym = next(x for x in act.symbols if act.code_of[x][0] == 16 and 1 <= (x & 15) <= 10)
        long_code = J.AC(sym >> 4, sym & 15, 1)
        bad = [list(x) for x in units]
        if cls == J.AC_SYM:                              # DC, the long code, then no code at all
            bad[u] = [units[u][0], long_code, J.EOB]
            bad = SC.plant(fr, bad, u, cls, rng, keep_n=1, pick=0)
        else:                                            # the long code fills slot 63: the next symbol is unit u + 1's DC, which is no code
            bad[u] = [units[u][0]] + [J.AC(0, 1, 1)] * (62 - (sym >> 4)) + [long_code]
            bad = SC.plant(fr, bad, u + 1, cls, rng, pick=0)
        data, it = J.write(fr, bad)
        assert it.status == cls, it.status
        out.append((f"{J.STATUS_NAMES[cls]} behind a long code", data, fr, it))
    return out


def _run(port, items, force_sequential=False, check_routing=True):
    import pjd_amd
    ctx = pjd_amd.Context(0)
    try:
        return G._decode_and_check(ctx, port, items, G._scan(items, force_sequential), check_routing=check_routing)
    finally:
        ctx.close()


def test_long_codes_on_the_parallel_path(port, monkeypatch):
    """Clean streams and the planted errors (careful_span) in lanes of 128 bytes: status, coefficients and pictures equal the intent and
    the oracle port; nothing is routed to the exact kernel or re-decoded."""
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    items = _streams()
    assert {it.status for *_, it in items} == {J.OK, J.AC_SYM, J.DC_SYM}
    info = _run(port, items)
    assert info["sub_bytes"] == 128 and info["n_sequential"] == 0 and info["n_fallback"] == 0
    assert info["n_subsequences"] >= 4 * len(items)                                   # several lanes a picture


@pytest.mark.parametrize("walk_max", ["64", "0"])
def test_long_codes_with_the_walker_forced_on_and_off(port, monkeypatch, walk_max):
    """PJD_WALK_MAX=64: every re-sync round is a cooperative walk, whose chase stops at a pointer entry and fetches the one second-level
    entry it needs (WALK_FIX); 0: never a walk."""
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    monkeypatch.setenv("PJD_WALK_MAX", walk_max)
    info = _run(port, _streams())
    assert (info["walks"] > 0) == (walk_max == "64"), info["walks"]
    assert info["n_fallback"] == 0


def test_long_codes_on_the_exact_kernel(port):
    """PJD_F_FORCE_SEQUENTIAL: pjd_k_huff_exact_lut reads the same blob."""
    items = _streams()
    info = _run(port, items, force_sequential=True, check_routing=False)
    assert info["n_sequential"] == len(items)


def test_mixed_table_sets_decoded_twice_from_one_upload(port, monkeypatch):
    """A set with no code over 9 bits (its blob is first levels only) beside one of complete 16-bit trees (128-entry tables in its last
    prefixes), each blob copied into an LDS region sized for the larger; two decodes of one upload give the same, right pictures."""
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    rng = np.random.default_rng(511)
    short_dc = J.Table([0, 0, 0, 9] + [0] * 12, list(range(9)))
    short_ac = L.ac_table([1, 1, 1, 1, 1, 1, 1, 1, 1] + [0] * 7)
    tree_dc = J.Table([1] * 15 + [2], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0xFF])
    tree_ac = L.ac_table([1] * 15 + [2])
    items = []
    for label, dct, act in (("no second level", short_dc, short_ac), ("16-bit tree", tree_dc, tree_ac), ("no second level, again", short_dc, short_ac)):
        fr = SC.frame(64, 64, "420", {0: dct}, {0: act})
        data, it = J.write(fr, SC.fill(fr, rng, p_eob=0.1))
        assert it.status == J.OK
        items.append((label, data, fr, it))
    scanned = G._scan(items)
    sizes = [pjd_amd.plan_luts(s.desc)[0].size for s in scanned]
    assert sizes[0] == sizes[2] == 2 * 2048 and sizes[1] > sizes[0], sizes
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([s.desc for s in scanned]) as b:
            b.upload()
            seen = []
            for rep in range(2):
                b.decode(); b.sync()
                outs, st = b.download()
                info = b.info()
                assert info["n_sequential"] == 0 and info["n_fallback"] == 0 and info["n_table_sets"] == 2
                assert info["huff_lds_bytes"] == sizes[1] + 2 * (2048 + 256) + 16
                for k, (label, data, fr, it) in enumerate(items):
                    assert st[k] == J.OK, (rep, label, st[k])
                    assert np.array_equal(b.coefficients(k), J.intent_buffer(fr, it)), (rep, label)
                    assert np.array_equal(outs[k], port.decode(data)["rgb"]), (rep, label)
                seen.append([o.tobytes() for o in outs])
            assert seen[0] == seen[1]
    finally:
        ctx.close()


def test_huff_lds_bytes_is_the_largest_real_blob():
    """Eight pictures of the default workload (tables fitted per picture): the dynamic LDS of the entropy decoder is the host builder's
    largest blob + 2 x (2,048 + 256) + 16, below what 256 bytes per long prefix would give; the runtime is asked with that size."""
    import pjd_amd
    import synth
    jpegs = synth.cfg3_imagenet_like(8, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    scanned = [pjd_amd.Scanned(j) for j in jpegs]
    luts = [pjd_amd.plan_luts(s.desc) for s in scanned]
    real, nominal = max(b.size for b, _, _ in luts), max(n for _, n, _ in luts)
    areas = 2 * (2048 + 256) + 16
    assert 0 < real < nominal
    assert pjd_amd.plan_info([s.desc for s in scanned])["huff_lds_bytes"] == real + areas
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([s.desc for s in scanned]) as b:
            info = b.info()
            assert info["huff_lds_bytes"] == real + areas < nominal + areas, (info["huff_lds_bytes"], real, nominal)
            wgs, lds = b.huff_occupancy()
            print(f"pjd_k_huff_lanes at {lds} B of LDS: {wgs} workgroups per CU")
            assert lds == info["huff_lds_bytes"] and wgs >= 1
    finally:
        ctx.close()
