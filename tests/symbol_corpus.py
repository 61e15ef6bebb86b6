"""Hand-built entropy streams (tests/jpeg_symbols.py): the fixed families behind tests/golden/sym_*.jpg and a seeded random corpus.

Every stream comes with its intent.  `fixtures()` -> {name: (jpeg, frame, intent)}; `corpus(n, seed)` -> [(label, jpeg, frame, intent)].
"""
import itertools

import numpy as np

from jpeg_symbols import (AC, AC_BITS, AC_LEN, AC_RUN, AC_SYM, CUT, DC, DC_BITS, DC_LEN, DC_SYM, END, EOB, RAW, Component, Frame,
                          Table, _token_bits, acv, dcv, write)

BASELINE_AC = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]           # the 162 symbols an encoder uses
SIZE0_RUNS = [r << 4 for r in range(1, 15)]                                                       # 0x10..0xE0


def kraft(counts):
    return sum(c / (1 << (ln + 1)) for ln, c in enumerate(counts))


def by_profile(symbols, first=2, complete=False):
    """Canonical table of `symbols` in this order: at most L - first + 1 codes of each length L from `first` on, the rest as long as
    they must be; incomplete (the all-ones codes stay free) unless `complete`."""
    counts, left = [0] * 16, len(symbols)
    for ln in range(first, 17):
        c = min(left, ln - first + 1) if ln < 16 else left
        counts[ln - 1] = c
        left -= c
    while kraft(counts) >= 1:                  # push codes down until they fit
        k = max(i for i in range(15) if counts[i])
        counts[k] -= 1
        counts[k + 1] += 1
    t = Table(counts, symbols)
    assert complete or kraft(counts) < 1
    return t


# ---- the table library --------------------------------------------------------------------------------------------------------------
def dc_general():
    """DC sizes 0..11, the out-of-range sizes 12..15 and the symbol 0xFF; incomplete."""
    return Table([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 5, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0xFF])


def ac_general():
    """EOB, ZRL, every size-0 run symbol, sizes 1..10 at runs 0..3, 1..4 at runs 4..15, the sizes 11..15 and 0xFF (110 symbols)."""
    syms = [0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0xF0, 0x04, 0x12, 0x31]
    rest = [(r << 4) | s for r in range(4) for s in range(1, 11)] + [(r << 4) | s for r in range(4, 16) for s in range(1, 5)]
    syms += [s for s in rest if s not in syms] + SIZE0_RUNS + [0x0B, 0x1C, 0x2D, 0x3E, 0x0F, 0xFF]
    return by_profile(syms)


def ac_162():
    """All 162 baseline symbols: the most a table may hold."""
    syms = [0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0x04, 0x12, 0x31, 0xF0] + [s for s in BASELINE_AC if s not in (0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0x04, 0x12, 0x31, 0xF0)]
    return by_profile(syms)


def ac_all16():
    """Every code 16 bits long: each symbol goes through the second-level table."""
    syms = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11) if s <= 6 or r < 2] + SIZE0_RUNS
    return Table([0] * 15 + [len(syms)], syms)


def ac_9_10():
    """Codes of exactly 9 and 10 bits around one short EOB: the edge between the first- and second-level tables."""
    syms = [0x00] + [0x01, 0x02, 0x03, 0x11, 0x12, 0x21, 0xF0, 0x0A, 0x31, 0x41, 0x05, 0x06, 0x07, 0x08, 0x09, 0x04, 0x13, 0x22, 0x51,
                     0x61, 0x71, 0x81, 0x91, 0xA1, 0xB1, 0xC1, 0xD1, 0xE1, 0xF1, 0x1A, 0x2A, 0x3A] + SIZE0_RUNS
    n9 = 20
    return Table([1, 0, 0, 0, 0, 0, 0, 0, n9, len(syms) - 1 - n9, 0, 0, 0, 0, 0, 0], syms)


def dc_single(sym=3):
    """One code: '0' for one DC size."""
    return Table([1] + [0] * 15, [sym])


def dc_ones():
    """DC sizes whose codes are long runs of 1-bits (streams of mostly 1-bits: dense FF00 stuffing)."""
    return Table([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])


def ac_ones():
    return Table([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0], [0x00, 0x11, 0x21, 0x12, 0x31, 0x0A, 0x08, 0x07, 0x06, 0x05, 0x04, 0x03,
                                                                     0x02, 0x01, 0xF0])


def dc_dup():
    """Duplicated symbols: two codes decode to size 2 (and two to 0)."""
    return Table([0, 1, 3, 3, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], [0, 2, 1, 3, 2, 4, 0, 5, 6, 7, 8, 9, 10, 11])


TABLES_DC = {"general": dc_general, "single": dc_single, "ones": dc_ones, "dup": dc_dup}
TABLES_AC = {"general": ac_general, "all162": ac_162, "all16": ac_all16, "edge9_10": ac_9_10, "ones": ac_ones}


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
SAMPLINGS = {"grey": [(1, 1)], "444": [(1, 1), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)],
             "440": [(1, 2), (1, 1), (1, 1)]}


def frame(w, h, sub, dc, ac, assign=None, ri=0, std=False, qt16=False):
    """assign: per component (DC id, AC id); the tables dc / ac are {id: Table}."""
    samp = SAMPLINGS[sub]
    if assign is None:
        assign = [(0, 0)] + [(1 if 1 in dc else 0, 1 if 1 in ac else 0)] * (len(samp) - 1)
    comps = [Component(hh, vv, min(j, 1), td, ta) for j, ((hh, vv), (td, ta)) in enumerate(zip(samp, assign))]
    qt = {t: [1 + ((k * 7 + t * 3) % 40) for k in range(64)] for t in {c.tq for c in comps}}
    return Frame(w, h, comps, dc, ac, qt=qt, qt16=set(qt) if qt16 else (), ri=ri, standard_restart=std)


def valid_symbols(table, ac):
    out = []
    for s in dict.fromkeys(table.symbols):
        if s == 0xFF:
            continue
        if ac and (s & 15) <= 10 and s != 0:
            out.append(s)
        if not ac and s <= 11:
            out.append(s)
    return out


def random_unit(rng, dct, act, p_eob=0.25, big=False):
    """One valid data unit drawn from what the tables hold."""
    dcs = valid_symbols(dct, False)
    size = int(rng.choice(dcs))
    toks = [DC(size, int(rng.integers(0, 1 << size)) if size else 0)]
    acs = valid_symbols(act, True)
    has_eob = 0x00 in act.symbols
    slot = 1
    while slot < 64:
        if has_eob and rng.random() < p_eob:
            toks.append(EOB)
            return toks
        fit = [s for s in acs if slot + (s >> 4) <= 63]
        if not fit:
            assert has_eob, "the AC table can neither end nor fill the unit"
            toks.append(EOB)
            return toks
        s = int(rng.choice(fit))
        run, sz = s >> 4, s & 15
        b = int(rng.integers(0, 1 << sz)) if sz else 0
        if big and sz:
            b = int(rng.choice([0, (1 << sz) - 1, b]))
        toks.append(AC(run, sz, b))
        slot += run + 1
    return toks


def tables_of(fr, u):
    per = fr.unit_comps()
    c = fr.comps[per[u % len(per)]]
    return fr.dc[c.td], fr.ac[c.ta]


def fill(fr, rng, **kw):
    return [random_unit(rng, *tables_of(fr, u), **kw) for u in range(fr.n_units())]


def first_unit_after_restart(fr):
    rst = sorted(fr.restarts_before())
    return rst[0] * len(fr.unit_comps()) if rst else None


def plant(fr, units, u, cls, rng, keep_n=None, pick=None):
    """Replace unit u (and drop what follows, for the truncation classes) by one that fails with `cls` in the reference's decoder."""
    dct, act = tables_of(fr, u)
    unit = list(units[u])
    body = unit[1:-1] if unit[-1] == EOB else unit[1:]
    keep = body[: int(rng.integers(0, len(body) + 1)) if keep_n is None else keep_n]
    while keep and 1 + sum(t[1] + 1 for t in keep) > 63:
        keep = keep[:-1]                                # the unit must still be open where the AC-class error goes
    slot = 1 + sum(t[1] + 1 for t in keep)
    ff_first = lambda: (pick // 7) % 2 == 0 if pick is not None else rng.random() < 0.5     # the table's own 0xFF, or a free code
    if cls == DC_SYM:
        new = [DC(0xFF)] if 0xFF in dct.symbols and ff_first() else [RAW("1" * 16)]
    elif cls == DC_LEN:
        bad = [s for s in dct.symbols if 11 < s < 0xFF]
        new = [DC(bad[pick % len(bad)] if pick is not None else int(rng.choice(bad)))]
    elif cls == DC_BITS:
        size = max(s for s in valid_symbols(dct, False))
        units[u] = [CUT(DC(size, int(rng.integers(0, 1 << size))), "bits")]
        return units[: u + 1]
    elif cls == AC_SYM:
        new = unit[:1] + keep + ([AC(15, 15)] if 0xFF in act.symbols and ff_first() else [RAW("1" * 16)])
    elif cls == AC_RUN:
        new = unit[:1] + keep
        while slot + 15 < 64:                          # ZRLs until a run of 15 overshoots slot 63
            new.append(AC(15, 0))
            slot += 16
        new.append(AC(15, 0))
    elif cls == AC_LEN:
        bad = [s for s in act.symbols if s != 0xFF and (s & 15) > 10 and slot + (s >> 4) < 64]
        b = bad[pick % len(bad)] if pick is not None else int(rng.choice(bad))
        new = unit[:1] + keep + [AC(b >> 4, b & 15)]
    elif cls == AC_BITS:
        s = max(valid_symbols(act, True), key=lambda x: (x & 15) if slot + (x >> 4) < 64 else -1)
        units[u] = unit[:1] + keep + [CUT(AC(s >> 4, s & 15, int(rng.integers(0, 1 << (s & 15)))), "bits")]
        return units[: u + 1]
    else:
        raise ValueError(cls)
    units[u] = new                                      # what follows the error is never read
    return units


def ac_oversub():
    """ac_general with two more 16-bit codes than fit (the reference's generate_codes keeps counting; those two never match): a table
    the planner refuses, so the picture goes to the literal kernel.  The 16-bit codes that fit decode to 0x01."""
    t = ac_general()
    code = 0
    for ln in range(1, 17):
        code = (code + t.counts[ln - 1]) << (1 if ln < 16 else 0)
    extra = (1 << 16) - code + 2
    return Table(t.counts[:15] + [t.counts[15] + extra], t.symbols + [0x01] * extra, oversubscribed=True)


GENERAL = ({0: dc_general(), 1: dc_general()}, {0: ac_general(), 1: ac_162()})


# ---- int16 edges -----------------------------------------------------------------------------------------------------------------
# The exact kernels keep an absolute DC in slot 0 of the dense scratch and mark an explicit zero at slot 52 with -32768: a DC of
# exactly -32768 (the int16 predictor reaches it) must stay a value.  These streams put absolute DCs at -32768, 32767 and -32767 in
# every component and sampling, at the last unit, after a restart and beside either kind of slot 52, and AC values whose dequantised
# product (int16)(c * q) is one of those three at natural positions 0, 1, 38 (from slot 48 and from slot 52), 58 (T.81 map) and 63.
ZERO52 = [acv(15, 3), acv(15, -3), acv(15, 9), AC(3, 0), EOB]           # slot 48 = 9, then an explicit 0 at slot 52
VALUE52 = [acv(15, 3), acv(15, -3), acv(15, -9), acv(3, 77), EOB]       # slot 48 = -9, then 77 at slot 52


def _split(d, n):
    """n DC differences (each within +-2047, zeros first) that add up to d."""
    full, rem = divmod(abs(d), 2047)
    s = 1 if d >= 0 else -1
    steps = [s * 2047] * full + ([s * rem] if rem else [])
    assert len(steps) <= n, (d, n)
    return [0] * (n - len(steps)) + steps


def dc_script(fr, anchors):
    """DC difference of every data unit (decode order) that takes component c's absolute DC to each anchor: anchors[c] lists
    (k, value, route) for the k-th unit of component c; route "wrap" goes there across the int16 wrap, anything else directly.
    The predictor restarts at 0 after every restart marker; units after an anchor keep its value until the next one."""
    per, rst = fr.unit_comps(), fr.restarts_before()
    seq, seg = {c: [] for c in range(len(fr.comps))}, 0
    for u in range(fr.n_units()):
        m, j = divmod(u, len(per))
        seg += j == 0 and m in rst
        seq[per[j]].append((u, seg))
    diffs = [0] * fr.n_units()
    for c, anc in anchors.items():
        units, pred, nxt, pseg = seq[c], 0, 0, 0
        for k, t, route in sorted(anc):
            if units[k][1] != pseg:                   # a restart since the last anchor: the predictor starts again at 0
                pred, pseg = 0, units[k][1]
                nxt = min(i for i in range(k + 1) if units[i][1] == pseg)
            d = t - pred
            if route == "wrap":
                d += 65536 if d < 0 else -65536
            for i, s in zip(range(nxt, k + 1), _split(d, k - nxt + 1)):
                diffs[units[i][0]] = s
            pred, nxt = t, k + 1
    return diffs


def _chain(k0, wrap_first):
    """Anchors over >= 21 units of a component from its k0-th: -32768 straight down (16 x -2047, then -16), -32767, -32768, 32767
    (down across the wrap), -32768 (up across the wrap); or first up to 32767 and across the wrap to -32768, -32767, -32768."""
    if wrap_first:
        return [(k0 + 16, 32767, "direct"), (k0 + 17, -32768, "wrap"), (k0 + 18, -32767, "direct"), (k0 + 19, -32768, "direct")]
    return [(k0 + 16, -32768, "direct"), (k0 + 17, -32767, "direct"), (k0 + 18, -32768, "direct"), (k0 + 19, 32767, "wrap"),
            (k0 + 20, -32768, "wrap")]


def edge_anchors(fr):
    """A _chain at the start of every restart segment that holds >= 21 units of a component (the two kinds in turn); every chain
    ends at -32768 and the value stays, so the last unit of each such segment -- the picture's last unit among them -- is -32768."""
    per, rst = fr.unit_comps(), fr.restarts_before()
    segs = {c: [] for c in range(len(fr.comps))}
    seg = 0
    for u in range(fr.n_units()):
        m, j = divmod(u, len(per))
        seg += j == 0 and m in rst
        segs[per[j]].append(seg)
    anchors = {}
    for c, ss in segs.items():
        starts = [k for k in range(len(ss)) if k == 0 or ss[k] != ss[k - 1]]
        anchors[c] = [a for n, k0 in enumerate(starts) if ss.count(ss[k0]) >= 21 for a in _chain(k0, (n + c) % 2 == 1)]
        assert anchors[c], "no restart segment holds 21 units of a component"
    return anchors


def edge_frame(w, h, sub, q_dc, qt16, ri=0, std=False, ac=None):
    """A frame of the general tables whose DC quantiser (zigzag entry 0 of every table) is q_dc."""
    dc, _ = GENERAL
    fr = frame(w, h, sub, dc, ac or {0: ac_general(), 1: ac_general()}, ri=ri, std=std, qt16=qt16)
    for t in fr.qt:
        fr.qt[t][0] = q_dc
    return fr


def dc_edge_units(fr, rng):
    """Units of `fr` that follow dc_script(edge_anchors(fr)); the anchored units alternate an explicit zero and a value at slot 52."""
    anchors = edge_anchors(fr)
    diffs = dc_script(fr, anchors)
    per = fr.unit_comps()
    comp_k = {c: [u for u in range(fr.n_units()) if per[u % len(per)] == c] for c in range(len(fr.comps))}
    marked = sorted(comp_k[c][k] for c, anc in anchors.items() for k, _, _ in anc)
    units = []
    for u in range(fr.n_units()):
        dct, act = tables_of(fr, u)
        body = random_unit(rng, dct, act)[1:]
        if u in marked:
            body = list(ZERO52 if marked.index(u) % 2 == 0 else VALUE52)
        units.append([dcv(diffs[u])] + body)
    return units


# name -> (width, height, sampling, DC quantiser, 16-bit DQT, restart interval, T.81 restart rule, AC table).  Every colour frame
# has >= 21 MCUs per restart segment, so that each chroma chain fits.
DC_EDGE_FRAMES = {
    "sym_edge_dc_grey_q1_ri24": (64, 48, "grey", 1, False, 24, False, None),
    "sym_edge_dc_444_q3_ri21": (56, 48, "444", 3, False, 21, False, None),
    "sym_edge_dc_420_q65535": (112, 48, "420", 65535, True, 0, False, None),
    "sym_edge_dc_422_q32768": (112, 24, "422", 32768, True, 0, False, None),
    "sym_edge_dc_440_q2": (56, 48, "440", 2, False, 0, False, None),
    # not committed (the planner routes them, or they differ only in a quantiser): the edge family of the GPU tests and the corpus
    "sym_edge_dc_444_q32767": (56, 24, "444", 32767, True, 0, False, None),
    "sym_edge_dc_grey_q2_ri21": (8, 8 * 42, "grey", 2, False, 21, False, None),
    "sym_edge_dc_420_q1_ri21_refrule": (112, 96, "420", 1, False, 21, False, None),      # subsampled luma + DRI: routed up front
    "sym_edge_dc_420_q3_ri21_std": (112, 96, "420", 3, False, 21, True, None),
    "sym_edge_dc_422_q1_ri21_refrule": (112, 48, "422", 1, False, 21, False, None),
    "sym_edge_dc_440_q65535_ri21_std": (56, 96, "440", 65535, True, 21, True, None),
    "sym_edge_dc_444_q3_oversub": (56, 24, "444", 3, False, 0, False, "oversub"),         # a table the planner refuses: literal kernel
}
COMMITTED_EDGE = ["sym_edge_dc_grey_q1_ri24", "sym_edge_dc_444_q3_ri21", "sym_edge_dc_420_q65535", "sym_edge_dc_422_q32768",
                  "sym_edge_dc_440_q2", "sym_edge_deq_444"]


def deq_edge_frame(standard_zigzag=False):
    """4:4:4, a 16-bit quantisation table per component: Y 32768 everywhere (an odd coefficient -> -32768) but 64 at natural 38 (zigzag
    entry 52 under either map: +-512 -> -32768); Cb 32767 (1 -> 32767, -1 -> -32767, a DC of -32768 -> -32768); Cr 32769 (1 -> -32767,
    -1 -> 32767).  Under T.81's map (standard_zigzag) slot 48 lands on natural 58 with Y's 32768."""
    dc, _ = GENERAL
    y = [32768] * 64
    y[52] = 64
    return Frame(40, 32, [Component(1, 1, t, 0, 0) for t in range(3)], {0: dc[0]}, {0: ac_162()},
                 qt={0: y, 1: [32767] * 64, 2: [32769] * 64}, qt16={0, 1, 2}, standard_zigzag=standard_zigzag)


def deq_edge_units(fr):
    """Per unit: DC, slot 1, slot 48, a slot 52 in every other MCU, slot 63 (no EOB).  The coefficients cycle through values whose
    products land on the edges under the unit's table; Cb's DC goes down to -32768 at its 19th unit."""
    per = fr.unit_comps()
    n_mcu = len(fr.mcus())
    anchors = {0: [(k, [1, -1, 3, -3][k % 4], "direct") for k in range(n_mcu)],
               1: [(0, 1, "direct"), (1, -1, "direct"), (18, -32768, "direct")],
               2: [(k, [1, -1][k % 2], "direct") for k in range(n_mcu)]}
    diffs = dc_script(fr, anchors)
    vals = {0: [1, -1, 3, 512, -512, 7], 1: [1, -1, 1, -1, 1, -1], 2: [1, -1, -1, 1, 1, -1]}
    units = []
    for u in range(fr.n_units()):
        c, m = per[u % len(per)], u // len(per)
        vv = vals[c]
        body = [acv(0, vv[m % 6]), AC(15, 0), AC(15, 0), acv(14, vv[(m + 3) % 6])]       # slots 1 and 48
        if m % 2:
            body += [acv(3, vv[(m + 4) % 6]), acv(10, vv[(m + 1) % 6])]                  # slots 52 and 63
        else:
            body += [acv(14, vv[(m + 1) % 6])]                                              # slot 63
        units.append([dcv(diffs[u])] + body)
    return units


def edge_family():
    """{name: (jpeg, frame, intent)}: every int16-edge stream (COMMITTED_EDGE among them)."""
    rng = np.random.default_rng(32768)
    F = {}
    for name, (w, h, sub, q, q16, ri, std, act) in DC_EDGE_FRAMES.items():
        ac = {0: ac_oversub(), 1: ac_general()} if act == "oversub" else None
        fr = edge_frame(w, h, sub, q, q16, ri=ri, std=std, ac=ac)
        F[name] = (*write(fr, dc_edge_units(fr, rng)), fr)
    for name, std in [("sym_edge_deq_444", False), ("sym_edge_deq_444_t81", True)]:
        fr = deq_edge_frame(std)
        F[name] = (*write(fr, deq_edge_units(fr)), fr)
    return {n: (d, fr, it) for n, (d, it, fr) in F.items()}


def edge_variants(rng, n):
    """Seeded variants of the DC family for the corpus: sampling, size, quantiser, table precision and restart layout drawn at random."""
    out = []
    for k in range(n):
        sub = str(rng.choice(list(SAMPLINGS)))
        mw, mh = 8 * SAMPLINGS[sub][0][0], 8 * SAMPLINGS[sub][0][1]
        q = int(rng.choice([1, 3, 255, 32767, 65535, 2, 32768]))
        ri = int(rng.choice([0, 21, 25]))
        per_row = int(rng.integers(1, 9))
        rows = -(-max(ri, 21) * int(rng.integers(1, 3)) // per_row) + int(rng.integers(0, 2))
        w, h = per_row * mw - int(rng.integers(0, mw // 2)), rows * mh - int(rng.integers(0, mh // 2))
        std = bool(ri and rng.random() < 0.5)
        fr = edge_frame(w, h, sub, q, q > 255 or bool(rng.random() < 0.3), ri=ri, std=std)
        try:
            units = dc_edge_units(fr, rng)
        except AssertionError:
            continue                              # a restart layout without a segment of 21 units of some component
        data, it = write(fr, units)
        out.append((f"edge{k}:{sub}:{w}x{h}:q{q}:ri{ri}{':std' if std else ''}", data, fr, it))
    return out


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def fixtures():
    F = {}
    rng = np.random.default_rng(9001)
    dc, ac = GENERAL

    def add(name, fr, units, eoi=True):
        data, it = write(fr, units, eoi)
        assert len(data) < 32768, name
        F[name] = (data, fr, it)

    # size-0 run symbols, runs that end on slot 63 or one past it, ZRL -> EOB, ZRL x3 + a coefficient, the slot-52 quirk
    fr = frame(64, 16, "444", dc, {0: ac_general(), 1: ac_general()})
    units = fill(fr, rng)
    special = [
        [dcv(5)] + [AC(r, 0) for r in range(1, 8)] + [AC(0, 1, 1), EOB],                  # 0x10..0x70: explicit zeros at 2, 5, 9, .. 35
        [dcv(-5)] + [AC(r, 0) for r in range(8, 13)] + [EOB],                             # 0x80..0xC0
        [dcv(1)] + [AC(13, 0), AC(14, 0), acv(0, -2), EOB],                                # 0xD0, 0xE0
        [dcv(-3), AC(15, 0), EOB],                                                        # ZRL -> EOB
        [dcv(0), AC(15, 0), AC(15, 0), AC(15, 0), acv(0, 7), EOB],                         # ZRL x3 (slots 16, 32, 48), +7 at slot 49
        [dcv(2), acv(15, 3), acv(15, -3), acv(15, 9), AC(3, 0), EOB],                      # slot 48 = 9, then an explicit 0 at slot 52
        [dcv(2), acv(15, 3), acv(15, -3), acv(15, -9), acv(3, 77), EOB],                   # slot 48 = -9, then 77 at slot 52
        [dcv(4), acv(15, 2), acv(15, 2), acv(15, 2), acv(14, -1)],                          # lands on slot 63, no EOB
        [dcv(4)] + [acv(0, (-1) ** k * (k % 50 + 1)) for k in range(63)],                  # every slot, no EOB
        [dcv(-4), acv(0, 1), AC(15, 0), AC(15, 0), AC(15, 0), acv(13, -1)],               # ZRLs, then a run of 13 onto slot 63
        [dcv(6), AC(14, 0), AC(14, 0), AC(14, 0), AC(14, 0), AC(2, 0)],                    # size-0 runs end on slot 63 (an explicit 0)
    ]
    units[: len(special)] = special
    add("sym_size0_runs_444", fr, units)

    # DC size 11 (value bits all 0, all 1), a predictor that wraps int16 both ways, across restarts; AC size 10 at +-1023, +-512
    fr = frame(64, 24, "grey", dc, ac, ri=5)
    units = []
    for k in range(fr.n_units()):
        seg = k % 5
        if k < 20:
            d = DC(11, (1 << 11) - 1) if (k // 5) % 2 == 0 else DC(11, 0)           # +2047 x5 / -2047 x5 per segment: no wrap (reset)
            units.append([d, acv(0, 1023), acv(0, -1023), acv(0, 512), acv(0, -512), EOB])
        else:
            units.append(random_unit(rng, dc[0], ac[0]))
    add("sym_dc11_ac10_rst5_grey", fr, units)
    fr = frame(8, 400, "grey", dc, ac, ri=23)
    units = [[DC(11, (1 << 11) - 1) if k < 23 else DC(11, 0), EOB] for k in range(fr.n_units())]     # +2047 x23 wraps up; after the
    #                                                                                                 restart -2047 x23 wraps down
    units[23] = [DC(11, 0), acv(0, 1023), EOB]
    add("sym_dc_wrap_both_ri23_8x400", fr, units)

    # tables: single-code DC, all 16-bit AC codes, 9/10-bit codes, 162 symbols, duplicates, four table pairs with ids 0..3
    fr = frame(17, 9, "420", {0: dc_single(3), 1: dc_single(2)}, {0: ac_all16(), 1: ac_9_10()})
    add("sym_tables_single_dc_all16_420_17x9", fr, fill(fr, rng))
    fr = frame(40, 40, "422", {0: dc_dup(), 1: dc_general()}, {0: ac_9_10(), 1: ac_162()})
    add("sym_tables_edge9_10_162_422_40x40", fr, fill(fr, rng, p_eob=0.1))
    four_dc = {0: dc_general(), 1: dc_dup(), 2: dc_ones(), 3: dc_single(4)}
    four_ac = {0: ac_general(), 1: ac_162(), 2: ac_9_10(), 3: ac_all16()}
    fr = frame(24, 24, "444", four_dc, four_ac, assign=[(3, 2), (1, 3), (2, 1)])
    add("sym_tables_ids_0_3_a_444", fr, fill(fr, rng))
    fr = frame(24, 24, "444", four_dc, four_ac, assign=[(0, 3), (0, 2), (3, 0)])        # Y and Cb share a DC table, not an AC table
    add("sym_tables_shared_dc_444", fr, fill(fr, rng))
    fr = frame(24, 24, "444", four_dc, four_ac, assign=[(2, 3), (1, 3), (0, 3)])        # all share the AC table, not a DC table
    add("sym_tables_shared_ac_444", fr, fill(fr, rng))
    fr = frame(48, 16, "444", {0: dc_ones()}, {0: ac_ones()}, assign=[(0, 0)] * 3)
    units = [[DC(11, (1 << 11) - 1), AC(0, 10, 1023), AC(0, 8, 255), AC(0, 7, 127), AC(1, 2, 3), EOB] for _ in range(fr.n_units())]
    add("sym_mostly_ones_444", fr, units)

    # frames
    for sub, (w, h), ri in [("grey", (1, 1), 0), ("444", (8, 8), 1), ("422", (17, 9), 0), ("420", (1, 300), 0), ("440", (300, 1), 0),
                            ("420", (300, 1), 0), ("444", (1, 300), 1), ("grey", (300, 1), 38), ("444", (40, 24), 5)]:
        fr = frame(w, h, sub, dc, ac, ri=ri, qt16=(sub == "440"))
        add(f"sym_frame_{sub}_{w}x{h}_ri{ri}", fr, fill(fr, rng))

    # errors: every class, planted in the first unit, the last unit or the first unit after a restart marker
    for cls, tag, where in [(DC_SYM, "dc_sym", "rst"), (DC_LEN, "dc_len", "first"), (DC_BITS, "cut_dc_bits", "last"),
                            (AC_SYM, "ac_sym", "last"), (AC_RUN, "ac_run", "rst"), (AC_LEN, "ac_len", "first"),
                            (AC_BITS, "cut_ac_bits", "rst")]:
        fr = frame(40, 16, "444", dc, {0: ac_general(), 1: ac_general()}, ri=(3 if where == "rst" else 0))
        units = fill(fr, rng)
        u = {"first": 0, "last": fr.n_units() - 1, "rst": first_unit_after_restart(fr)}[where]
        if cls in (DC_BITS, AC_BITS) and where == "rst":
            u = max(fr.restarts_before()) * len(fr.unit_comps())    # a cut in the last restart segment: every segment reaches the file
        add(f"sym_err_{tag}_{where}", fr, plant(fr, units, u, cls, rng))
    fr = frame(64, 8, "grey", dc, ac)
    units = fill(fr, rng)
    units[5] = [dcv(0), acv(15, 1), acv(15, 1), acv(15, 1), AC(15, 0)]                  # slot 49 + 15 = 64: one past the end
    add("sym_err_ac_run_to_64_grey", fr, units)
    fr = frame(40, 16, "420", dc, ac)
    units = fill(fr, rng)
    units[9] = [CUT(DC(11, 5), "code")]
    add("sym_err_cut_in_code_420", fr, units[:10])
    fr = frame(40, 16, "444", dc, ac)
    units = fill(fr, rng)[:17] + [[END]]
    add("sym_err_end_on_unit_boundary_444", fr, units)

    # int16 edges: absolute DCs of -32768 / 32767 / -32767 and dequantised products at those values (the rest of the family: corpus())
    edge = edge_family()
    for name in COMMITTED_EDGE:
        assert len(edge[name][0]) < 2048, name
        F[name] = edge[name]
    return F


# ---- the random corpus -------------------------------------------------------------------------------------------------------------
def corpus(n=300, seed=31337):
    rng = np.random.default_rng(seed)
    out = []
    dc_names, ac_names = list(TABLES_DC), list(TABLES_AC)
    k = n_planted = 0
    while len(out) < n:
        k += 1
        sub = str(rng.choice(list(SAMPLINGS)))
        w, h = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        if rng.random() < 0.1:
            w, h = (int(rng.integers(1, 4)), int(rng.integers(100, 300)))[:: 1 if rng.random() < 0.5 else -1]
        dcs = {i: TABLES_DC[str(rng.choice(dc_names))]() for i in range(4)}
        acs = {i: TABLES_AC[str(rng.choice(ac_names))]() for i in range(4)}
        ncomp = len(SAMPLINGS[sub])
        assign = [(int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(ncomp)]
        if ncomp == 3 and rng.random() < 0.5:
            assign[2] = assign[1]                  # Cb and Cr mostly share their tables
        mcux = (w + 8 * SAMPLINGS[sub][0][0] - 1) // (8 * SAMPLINGS[sub][0][0])
        ri = int(rng.choice([0, 0, 1, 2, 3, 7, mcux]))
        fr = frame(w, h, sub, dcs, acs, assign=assign, ri=ri, std=bool(ri and rng.random() < 0.7))
        units = fill(fr, rng, p_eob=float(rng.choice([0.05, 0.3, 0.7])), big=bool(rng.random() < 0.3))
        roll = rng.random()
        label = f"{k}:{sub}:{w}x{h}:ri{ri}"
        try:
            if roll < 0.45:
                cls = 1 + n_planted % 7                  # every class in turn, and in turn each bad size of DC_LEN / AC_LEN
                u = int(rng.integers(0, len(units)))
                units = plant(fr, units, u, cls, rng, pick=n_planted // 7)
                label += f":err{cls}@{u}"
            elif roll < 0.5:
                units = units[: int(rng.integers(0, len(units)))] + [[END]]
                label += ":end"
            data, it = write(fr, units)
        except (ValueError, IndexError, ZeroDivisionError, AssertionError):
            continue                           # the planted form does not exist with these tables / at this bit position
        n_planted += ":err" in label
        out.append((label, data, fr, it))
    out += [(name, *x) for name, x in edge_family().items() if name not in COMMITTED_EDGE]
    out += edge_variants(np.random.default_rng(seed + 1), 12)
    return out


# ---- routing, restated -------------------------------------------------------------------------------------------------------------
L1_BYTES, LUT_LDS_MAX = 4 << 9, 6 * (4 << 9) + 8192          # pjd_internal.h: PJD_L1_BYTES, PJD_LUT_LDS_MAX


def _second_level_bytes(t):
    """Second-level tables of one decode table: 256 bytes per 9-bit prefix that starts codes longer than 9 bits (pjd_plan.cpp)."""
    code, end9 = 0, 0
    for ln in range(1, 17):
        code += t.counts[ln - 1]
        if ln == 9:
            end9 = code
        if ln < 16:
            code <<= 1
    p0, p1 = min(end9, 512), min((code + 127) >> 7, 512)
    return max(p1 - p0, 0) * 256


def tables_fit(fr):
    """Does the parallel decoder take the frame's tables?  One slot per distinct AC table, one per distinct (DC table, AC slot)."""
    key = lambda t: (tuple(t.counts), tuple(t.symbols))
    if any(t.oversubscribed for c in fr.comps for t in (fr.dc[c.td], fr.ac[c.ta])):
        return False                           # not a prefix code: the planner gives it no decode table
    ac_slots, dc_slots = [], []
    for c in fr.comps:
        a = key(fr.ac[c.ta])
        if a not in ac_slots:
            ac_slots.append(a)
        d = (key(fr.dc[c.td]), ac_slots.index(a))
        if d not in dc_slots:
            dc_slots.append(d)
    used = {key(fr.ac[c.ta]): fr.ac[c.ta] for c in fr.comps}
    used_dc = {key(fr.dc[c.td]): fr.dc[c.td] for c in fr.comps}
    total = (len(ac_slots) + len(dc_slots)) * L1_BYTES
    total += sum(_second_level_bytes(used[a]) for a in ac_slots) + sum(_second_level_bytes(used_dc[d[0]]) for d in dc_slots)
    return total <= LUT_LDS_MAX


def expect_sequential(fr, it):
    """The planner's up-front routing to the exact kernel: tables it does not take, the reference's restart rule with subsampled luma,
    and restart segments that do not all reach the file (a stream cut short)."""
    if not tables_fit(fr):
        return True
    if fr.ri and not fr.standard_restart and (fr.hs, fr.vs) != (1, 1):
        return True
    if fr.ri:
        per = len(fr.unit_comps())
        return any(m * per >= len(it.unit_bit) for m in fr.restarts_before())
    return False


# ---- streams at the density bound ----------------------------------------------------------------------------------------------------
def unit_symbols(toks, dct, act):
    """(code bits, code + value bits, ends the unit) of each symbol of a valid unit."""
    out, slot = [], 0
    for t in toks:
        tb, nc = _token_bits(t, dct if slot == 0 else act)
        if t[0] == "DC":
            slot = 1
            out.append((nc, len(tb), False))
        elif t == EOB:
            out.append((nc, len(tb), True))
            slot = 64
        else:
            slot += t[1] + 1
            out.append((nc, len(tb), slot >= 64))
    return out


def unit_steps(syms):
    """Write-pass steps of one unit that takes every pair the format allows (pjd_internal.h): the first symbol whole within 8 bits and
    leaving the unit open, the second one's code within what is left of 9 bits."""
    k = steps = 0
    while k < len(syms):
        if k + 1 < len(syms) and syms[k][1] <= 8 and not syms[k][2] and syms[k][1] + syms[k + 1][0] <= 9:
            k += 2
        else:
            k += 1
        steps += 1
    return steps


def unit_shapes(dct, act, max_ac=3, n_dc=6, n_ac=10):
    """Valid units of a DC symbol and up to `max_ac` AC symbols ending in an EOB, or on slot 63 without one, from the cheapest symbols
    (value bits all 0).  Pairs never reach across units, so a stream's steps are the sum of its units'."""
    dcs = sorted(valid_symbols(dct, False), key=lambda s: len(dct.code_bits(s)) + s)[:n_dc]
    acs = sorted(valid_symbols(act, True), key=lambda s: len(act.code_bits(s)) + (s & 15))[:n_ac]
    for d in dcs:
        for n in range(max_ac + 1):
            for seq in itertools.product(acs, repeat=n):
                end = 1 + sum((s >> 4) + 1 for s in seq)
                if end < 64 and 0x00 in act.symbols:
                    yield [DC(d, 0)] + [AC(s >> 4, s & 15, 0) for s in seq] + [EOB]
                elif end == 64:
                    yield [DC(d, 0)] + [AC(s >> 4, s & 15, 0) for s in seq]


def cheapest_unit(dct, act, **kw):
    """The unit with the fewest bits per step."""
    return min(unit_shapes(dct, act, **kw), key=lambda u: bits_per_step(u, dct, act))


def bits_per_step(u, dct, act):
    s = unit_symbols(u, dct, act)
    return sum(x[1] for x in s) / unit_steps(s)


def dense_frame(fr, **kw):
    """`fr` filled with the cheapest unit of each component, over and over: a stream that runs at its tables' step bound."""
    per, units = {}, []
    for u in range(fr.n_units()):
        dct, act = tables_of(fr, u)
        key = (id(dct), id(act))
        if key not in per:
            per[key] = cheapest_unit(dct, act, **kw)
        units.append(per[key])
    return units
