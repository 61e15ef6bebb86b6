"""Hand-built progressive (SOF2) streams for the tests: named streams that each hold forms the others do not, a seeded random corpus,
broken streams derived from valid ones, and the one picture of 32768 blocks.  Everything is written by tests/jpeg_progressive.py from
target coefficients and a scan script; nothing here decodes.

    named()     {name: Written}            hand-made scripts (the `prog_*` ones in FIXTURES are committed under tests/golden/progressive/)
    corpus()    [(label, Written)]         named() + seeded random frames, scripts and coefficients
    broken()    [(label, data, frame, status, scan, block, tags)]   cuts and planted symbols, per procedure, scan and block position
    big()       Written                    2048x1024 grey: EOB10..EOB14, the flush at 32767 followed by another run
"""
import functools

import numpy as np

import jpeg_progressive as P
import jpeg_symbols as J
import symbol_corpus as SC
from jpeg_progressive import S

SIZES = [(1, 1), (8, 8), (17, 9), (1, 300), (300, 1), (40, 24), (33, 70)]
SUBS = ["grey", "444", "422", "420", "440"]


def frame_of(sub, w, h):
    """A frame decoded with T.81's zigzag map (PJD_F_STANDARD_ZIGZAG), as every progressive test decodes; its baseline tables serve only
    the baseline twin that gives the oracle port its metadata."""
    fr = SC.frame(w, h, sub, {0: SC.dc_general()}, {0: SC.ac_162()}, assign=[(0, 0)] * len(SC.SAMPLINGS[sub]))
    fr.standard_zigzag = True
    return fr


def twin(fr):
    """The same frame as a baseline file of zeros: what the oracle port reads its metadata from."""
    return J.write(fr, [[J.dcv(0), J.EOB]] * fr.n_units())[0]


def random_target(fr, rng, density=0.15, p_empty=0.3, amp=1023, dc_amp=1000):
    nu = fr.n_units()
    t = np.zeros((nu, 64), np.int64)
    t[:, 0] = rng.integers(-dc_amp, dc_amp + 1, nu)
    mag = np.minimum(amp, rng.geometric(0.08, (nu, 63)) * rng.choice([1, 1, 1, 2, 9, 40], (nu, 63)))
    ac = np.where(rng.random((nu, 63)) < density, mag * rng.choice([-1, 1], (nu, 63)), 0)
    ac[rng.random(nu) < p_empty] = 0
    t[:, 1:] = ac
    return t


def comps_of(fr):
    return list(range(len(fr.comps)))


def full_script(fr, dc_al=1, ac_al=2, bands=((1, 5), (6, 63)), ri=None, eob="max", shape="flat", tids=(0, 0, 0)):
    """DC first (interleaved) at dc_al, AC first per component and band at ac_al, then every refinement level down to 0."""
    cs = comps_of(fr)
    sc = [S(cs, al=dc_al, ri=ri, tid=[tids[c] for c in cs], shape=shape)]
    for c in cs:
        sc += [S(c, a, b, 0, ac_al, eob=eob, tid=tids[c], shape=shape) for a, b in bands]
    for al in range(ac_al - 1, -1, -1):
        for c in cs:
            sc += [S(c, a, b, al + 1, al, eob=eob, tid=tids[c], shape=shape) for a, b in bands]
    for al in range(dc_al - 1, -1, -1):
        sc.append(S(cs, ah=al + 1, al=al, tid=[tids[c] for c in cs]))
    return sc


def _refinement_forms_target(fr):
    """Grey blocks made for G.1.2.3 at the step Al 1 -> 0: |v| >= 2 has history, |v| == 1 is new."""
    t = np.zeros((fr.n_units(), 64), np.int64)
    t[:, 0] = [40 * k - 100 for k in range(fr.n_units())]
    t[0, [1, 2, 10, 25, 63]] = [3, -1, -5, 1, 1]       # new after a history one; a negative correction inside a ZRL's span; new at Se
    t[1, [1, 7]] = [2, -3]                              # EOB in a block that owes corrections ...
    t[2, [3]] = [-7]                                    # ... and more of them inside the same run
    t[3, [1, 20, 40, 62, 63]] = [-1, 1, -1, 5, -1]      # ZRLs without corrections; new at Se after a history one
    t[5, [30]] = [6]
    t[6, [63]] = [-2]
    return t


@functools.lru_cache(maxsize=1)
def named():
    out = {}
    rng = np.random.default_rng(20260)

    def add(name, fr, target, script, **kw):
        out[name] = P.build(fr, target, script, **kw)
        out[name].name = name

    fr = frame_of("grey", 8, 8)
    add("prog_dc_only_grey_8x8", fr, random_target(fr, rng), [S(0)])
    fr = frame_of("grey", 1, 1)
    add("prog_full_grey_1x1", fr, random_target(fr, rng, 0.4, 0), full_script(fr, eob="single"))
    fr = frame_of("grey", 64, 8)
    add("prog_refine_forms_grey_64x8", fr, _refinement_forms_target(fr),
        [S(0, al=0), S(0, 1, 63, 0, 1, shape="skew"), S(0, 1, 63, 1, 0, shape="skew")])
    fr = frame_of("420", 17, 9)
    add("prog_420_17x9_ri1_tables_0_3", fr, random_target(fr, rng, 0.2, 0.2), full_script(fr, ri=1, tids=(0, 3, 2), shape="skew"))
    fr = frame_of("422", 17, 9)
    add("prog_422_17x9_three_levels", fr, random_target(fr, rng, 0.2, 0.3), full_script(fr, dc_al=2, ac_al=3, eob=("random", 5)))
    fr = frame_of("440", 300, 1)
    add("prog_440_300x1_ri_prime", fr, random_target(fr, rng, 0.1, 0.5), full_script(fr, ri=7, bands=((1, 63),)))
    fr = frame_of("444", 1, 300)
    add("prog_444_1x300_ri_row", fr, random_target(fr, rng, 0.1, 0.5), full_script(fr, ri=1, bands=((1, 63),), eob="single"))
    fr = frame_of("420", 40, 24)
    cs = [0, 1, 2]
    # the restart interval changes between scans (MCUs of the scan: 3 interleaved MCUs a row, 5 luma blocks a row) and goes back to 0; a
    # table id redefined between scans; component 1 uses id 0 after component 0 left another table there
    add("prog_420_40x24_dri_changes", fr, random_target(fr, rng, 0.15, 0.3),
        [S(cs, al=1, ri=3), S(0, 1, 63, 0, 1, ri=5), S(1, 1, 63, 0, 1, ri=2), S(2, 1, 63, 0, 1, ri=0, tid=1), S(0, 1, 63, 1, 0, ri=7, shape="skew"),
         S(1, 1, 63, 1, 0, ri=0), S(2, 1, 63, 1, 0, ri=1, tid=0), S(cs, ah=1, al=0, ri=4)])
    fr = frame_of("444", 17, 9)
    add("prog_444_17x9_incomplete", fr, random_target(fr, rng, 0.3, 0.1),
        [S(cs, al=2), S(0, 1, 9, 0, 2), S(1, 4, 4, 0, 0), S(0, 1, 9, 2, 1), S(cs[:2], ah=2, al=1), S(2, 20, 63, 0, 3)])
    fr = frame_of("grey", 16, 16)
    add("prog_grey_16x16_one_slot_a_band", fr, random_target(fr, rng, 0.3, 0.1),
        [S(0, al=0)] + [S(0, z, z, 0, 1, tid=z % 4) for z in range(1, 64)] + [S(0, z, z, 1, 0, tid=z % 4) for z in range(63, 0, -1)])
    fr = frame_of("grey", 24, 16)
    add("prog_grey_24x16_band_split_48_52", fr, random_target(fr, rng, 0.5, 0),
        [S(0, al=0), S(0, 1, 39, 0, 1), S(0, 40, 50, 0, 1), S(0, 51, 63, 0, 1), S(0, 40, 50, 1, 0), S(0, 51, 63, 1, 0), S(0, 1, 39, 1, 0)])
    # illegal, but they pass the scanner: a refinement scan repeated at the same Ah/Al, where the (cur & p1) == 0 guard decides ...
    add("prog_grey_24x16_refinement_repeated", fr, random_target(fr, rng, 0.4, 0.1),
        [S(0, al=1), S(0, 1, 63, 0, 2), S(0, 1, 63, 2, 1), S(0, 1, 63, 2, 1, eob="single"), S(0, ah=1, al=0), S(0, ah=1, al=0), S(0, 1, 63, 1, 0)],
        legal=False)
    # ... and an AC first band over slots an earlier one reached, where the zeros stored over runs and ZRLs show
    add("prog_grey_24x16_overlapping_bands", fr, random_target(fr, rng, 0.4, 0.1),
        [S(0, al=0), S(0, 1, 30, 0, 0), S(0, 5, 50, 0, 3), S(0, 20, 63, 0, 1)], legal=False)
    # end-of-band runs that claim more blocks than their restart interval has left: the restart drops the rest of the run
    fr = frame_of("grey", 64, 16)
    t = np.zeros((fr.n_units(), 64), np.int64)
    t[:, 0] = rng.integers(-200, 200, fr.n_units())
    t[[0, 7, 12], 3] = [5, -1, 2]
    t[[4, 12], 9] = [1, -6]
    add("prog_grey_64x16_eob_run_cut_by_a_restart", fr, t,
        [S(0, al=0, ri=3), S(0, 1, 63, 0, 1, eob_overrun=5), S(0, 1, 63, 1, 0, ri=5, eob_overrun=2)])
    # every EOBn the frame has room for, extra bits all zero and all one, in first and refinement scans; the run of the last scan ends
    # exactly on the last block
    fr = frame_of("grey", 256, 256)
    t = np.zeros((fr.n_units(), 64), np.int64)
    t[:, 0] = rng.integers(-500, 500, fr.n_units())
    t[::97, 11] = 3
    t[5::131, 12] = -1
    zo = lambda lo, hi: [x for n in range(lo, hi) for x in (1 << n, (2 << n) - 1)]
    add("eobn_grey_256x256", fr, t,
        [S(0), S(0, 1, 2, 0, 1, eob=("lengths", zo(0, 8))), S(0, 3, 4, 0, 1, eob=("lengths", [256, 511])), S(0, 5, 6, 0, 1, eob=("lengths", [512, 511])),
         S(0, 7, 8, 0, 1, eob=("lengths", [1023])), S(0, 1, 2, 1, 0, eob=("lengths", zo(0, 8))), S(0, 3, 4, 1, 0, eob=("lengths", [256, 511])),
         S(0, 5, 6, 1, 0, eob=("lengths", [512, 511])), S(0, 7, 8, 1, 0, eob=("lengths", [1023])), S(0, 11, 12, 0, 1), S(0, 11, 12, 1, 0),
         S(0, 9, 10, 0, 0, eob=("lengths", [1024]))])
    return out


FIXTURES = ["prog_dc_only_grey_8x8", "prog_full_grey_1x1", "prog_refine_forms_grey_64x8", "prog_420_17x9_ri1_tables_0_3",
            "prog_422_17x9_three_levels", "prog_440_300x1_ri_prime", "prog_444_1x300_ri_row", "prog_420_40x24_dri_changes",
            "prog_444_17x9_incomplete", "prog_grey_16x16_one_slot_a_band", "prog_grey_24x16_band_split_48_52",
            "prog_grey_24x16_refinement_repeated", "prog_grey_24x16_overlapping_bands", "prog_grey_64x16_eob_run_cut_by_a_restart"]


def random_script(fr, rng):
    cs = comps_of(fr)
    cuts = sorted(set(rng.integers(1, 63, rng.integers(0, 4)).tolist()))
    bands = list(zip([1] + [c + 1 for c in cuts], cuts + [63]))
    eob = [("random", int(rng.integers(1 << 30))), "max", "single"][int(rng.integers(3))]
    mcus = len(fr.mcus())
    ri = [None, 1, max(1, fr.bw // fr.hs), 3, 5][int(rng.integers(5))]
    sc = full_script(fr, dc_al=int(rng.integers(0, 3)), ac_al=int(rng.integers(0, 4)), bands=bands, ri=ri, eob=eob,
                     shape=["flat", "skew", "long"][int(rng.integers(3))], tids=tuple(int(x) for x in rng.integers(0, 4, 3)))
    if rng.random() < 0.5 and mcus > 1:                   # the interval changes somewhere, and goes back to 0 later
        k = int(rng.integers(1, len(sc)))
        sc[k] = sc[k]._replace(ri=int(rng.integers(1, 9)))
        k2 = int(rng.integers(k, len(sc)))
        if k2 > k:
            sc[k2] = sc[k2]._replace(ri=0)
    if rng.random() < 0.3:                                # incomplete: the last scans are missing
        sc = sc[:int(rng.integers(1, len(sc) + 1))]
    return sc


@functools.lru_cache(maxsize=2)
def corpus(n=40, seed=4242):
    """[(label, Written)]: the named streams and `n` seeded random ones over every sampling and size."""
    rng = np.random.default_rng(seed)
    items = list(named().items())
    for k in range(n):
        sub = SUBS[k % len(SUBS)]
        w, h = SIZES[(k // len(SUBS) + k) % len(SIZES)]
        fr = frame_of(sub, w, h)
        t = random_target(fr, rng, density=float(rng.choice([0.03, 0.15, 0.5])), p_empty=float(rng.choice([0, 0.3, 0.8])),
                          amp=int(rng.choice([3, 60, 1023])))
        items.append((f"rand{k}_{sub}_{w}x{h}", P.build(fr, t, random_script(fr, rng))))
    return items


@functools.lru_cache(maxsize=1)
def big():
    """2048x1024 grey, 32768 blocks a scan: EOB10..EOB14 with extra bits all zero and all one, and the flush at 32767 followed by
    another run (the last block's).  The one picture of its size."""
    fr = frame_of("grey", 2048, 1024)
    nu = fr.n_units()
    t = np.zeros((nu, 64), np.int64)
    t[:, 0] = (np.arange(nu) % 2048) - 1024
    t[::5000, 5] = 2
    t[::7001, 5] = -3
    L = lambda n: [1 << n, (2 << n) - 1]
    w = P.build(fr, t, [S(0), S(0, 1, 1, 0, 0, eob=("lengths", L(10) + L(11) + L(12))), S(0, 2, 2, 0, 0, eob=("lengths", L(13))),
                        S(0, 3, 3, 0, 0, eob=("lengths", [1 << 14])), S(0, 4, 4, 0, 0, eob="max"), S(0, 5, 5, 0, 1, eob="max"),
                        S(0, 5, 5, 1, 0, eob=("lengths", [1 << 14, 5000]))])
    w.name = "big_grey_2048x1024"
    return w


# ---- broken streams --------------------------------------------------------------------------------------------------------------------

PROCEDURES = {(True, False): "dc_first", (True, True): "dc_refine", (False, False): "ac_first", (False, True): "ac_refine"}


def _bases():
    """Valid streams to break: between them every procedure is the first, a middle and the last scan wherever a legal file can have it
    there, with restart intervals that start a segment at the last block."""
    rng = np.random.default_rng(777)
    out = []
    fr = frame_of("444", 24, 16)
    t = random_target(fr, rng, 0.5, 0.0, amp=300)
    cs = [0, 1, 2]
    kw = dict(shape="long", eob="single")
    out.append(("a", fr, t, [S(cs, al=1, ri=5, shape="long"), S(0, 1, 5, 0, 1, **kw), S(1, 1, 63, 0, 1, **kw), S(2, 1, 63, 0, 1, **kw),
                             S(cs, ah=1, al=0), S(0, 6, 63, 0, 0, **kw), S(0, 1, 5, 1, 0, **kw), S(1, 1, 63, 1, 0, **kw), S(2, 1, 63, 1, 0, **kw)]))
    out.append(("b", fr, t, [S(0, al=1, ri=5, shape="long"), S(0, 1, 9, 0, 0, **kw), S([1, 2], al=1, shape="long"), S(0, 10, 63, 0, 1, **kw),
                             S(0, 10, 63, 1, 0, **kw), S(cs, ah=1, al=0)]))
    out.append(("c", fr, t, [S(cs, al=0, ri=1, shape="long"), S(1, 1, 3, 0, 1, **kw), S(1, 1, 3, 1, 0, **kw), S(2, 1, 9, 0, 0, ri=5, **kw)]))
    fr = frame_of("grey", 40, 16)
    t = random_target(fr, rng, 0.5, 0.3, amp=300)
    kw = dict(shape="long", eob="max")
    out.append(("d", fr, t, [S(0, al=1, ri=1, shape="long"), S(0, 1, 4, 0, 1, **kw), S(0, ah=1, al=0), S(0, 1, 4, 1, 0, **kw), S(0, 5, 63, 0, 0, **kw)]))
    out.append(("e", fr, t, [S(0, al=0, shape="long"), S(0, 1, 63, 0, 0, ri=9, shape="long", eob="single")]))
    out.append(("f", fr, t, [S(0, 0, 0, 0, 1, ri=9, shape="long"), S(0, 1, 63, 0, 1, **kw), S(0, 1, 63, 1, 0, **kw), S(0, ah=1, al=0, ri=1)]))
    fr = frame_of("grey", 128, 16)
    t = random_target(fr, rng, 0.3, 0.85, amp=3)
    out.append(("h", fr, t, [S(0, al=0), S(0, 1, 63, 0, 1, eob="max"), S(0, 1, 63, 1, 0, eob="max", shape="skew")]))
    fr = frame_of("444", 24, 16)
    t = random_target(fr, rng, 0.5, 0.0, amp=300)
    out.append(("g", fr, t, [S(0, al=0, shape="long"), S(0, 1, 63, 0, 0, shape="long", eob="single"), S([1, 2], al=0, ri=2, shape="long")]))
    return out


SYMBOLS = {"dc_first": [0xFF] + list(range(12, 16)),
           "ac_first": [0xFF] + list(range(0x0B, 0x10)) + [0xF1, 0xF0],       # 0xF1 / 0xF0: a run and a ZRL past Se in a narrow band
           "ac_refine": [0xFF, 0x02, 0x13]}


@functools.lru_cache(maxsize=1)
def broken():
    """[(label, data, frame, status, scan, block, tags)]: tags = (procedure, scan position, block position, kind)."""
    out = []
    for bname, fr, t, script in _bases():
        w = P.build(fr, t, script)
        for si, sc in enumerate(script):
            proc = PROCEDURES[(sc.ss == 0, sc.ah != 0)]
            spos = "first" if si == 0 else "last" if si == len(script) - 1 else "middle"
            nb = w.scans[si]["n_blocks"]
            ri, per = w.scans[si]["restart_interval"], w.scans[si]["blocks_per_mcu"]
            blocks = [("first", 0), ("last", nb - 1)]
            if ri and ri * per < nb:
                blocks.append(("after_restart", ri * per * ((nb - 1) // (ri * per))))
            blocks.append(("middle", None))
            for bpos, blk in blocks:
                if blk is None:                           # cuts a token of each kind holds wherever it may lie in the scan
                    for where in ("code", "bits"):
                        for kind in ("dc", "dcbit", "ac", "acr", "eobn", "zrl", "corr"):
                            r = P.cut(w, si, where, lambda b, k: k == kind)
                            if r is not None:
                                out.append((f"{bname}:s{si}:{proc}:any{r[2]}:cut_{where}_{kind}", r[0], fr, r[1], si, r[2], (proc, spos, "middle", f"cut_{where}_{kind}")))
                    continue
                if bpos == "last" and ri and blk % (ri * per) == 0:
                    bpos_tags = ("last", "after_restart")
                else:
                    bpos_tags = (bpos,)
                made = []
                for where in ("code", "bits"):
                    for kinds in (("dc",), ("dcbit",), ("ac", "acr"), ("eobn",), ("zrl",), ("corr",)):
                        r = P.cut(w, si, where, lambda b, k: b == blk and k in kinds)
                        if r is not None:
                            made.append((f"cut_{where}_{r[3]}", r[0], r[1], r[2]))
                if proc != "dc_refine":
                    band = sc.se - sc.ss
                    for sym in SYMBOLS[proc] + ["raw"]:
                        if proc == "ac_first" and sym in (0xF1, 0xF0) and band >= 15:
                            continue
                        dmg = P.Damage(si, blk, "raw", None) if sym == "raw" else P.Damage(si, blk, "sym", sym)
                        wd = P.build(fr, t, script, damage=dmg)
                        made.append(("raw" if sym == "raw" else f"sym_{sym:02x}", wd.data, wd.intent.status, blk))
                for kind, data, status, eblk in made:
                    for bp in bpos_tags:
                        out.append((f"{bname}:s{si}:{proc}:{bp}{eblk}:{kind}", data, fr, status, si, eblk, (proc, spos, bp, kind)))
    seen = set()
    return [x for x in out if not (x[0] in seen or seen.add(x[0]))]


def desynchronised():
    """Refinement streams with a run and a ZRL that pass Se: no error class of their own -- the coefficient is dropped and the decode
    goes on -- so only a decoder knows what follows.  [(label, data, frame)]"""
    out = []
    fr = frame_of("grey", 24, 16)
    t = random_target(fr, np.random.default_rng(99), 0.5, 0.0, amp=3)
    kw = dict(shape="long", eob="single")
    for bname, fr, t, script in [("z", fr, t, [S(0), S(0, 1, 5, 0, 1, **kw), S(0, 6, 63, 0, 1, **kw), S(0, 1, 5, 1, 0, **kw), S(0, 6, 63, 1, 0, **kw)])]:
        for si, sc in enumerate(script):
            if sc.ss and sc.ah and sc.se - sc.ss < 15:
                for sym in (0xF1, 0xF0):
                    data = _unchecked_damage(fr, t, script, si, sym)
                    out.append((f"{bname}:s{si}:refine_run_past_se_{sym:02x}", data, fr))
    return out


def _unchecked_damage(fr, t, script, si, sym):
    """Symbol `sym` planted at block 0 of refinement scan `si` (0xF1: a new coefficient after a run past Se; 0xF0: a ZRL past Se)."""
    w = P.build(fr, t, script)
    parts = [(pre, list(segs)) for pre, segs in w.parts]
    tab = w.scans[si]["tables"][0]
    # a scan of its own table: rebuild it with the planted symbol first
    syms = [sym] + [s for s in tab.symbols if s != sym]
    table = P._make_table(syms, "long")
    toks = [x for x in w.tokens if x[0] == si]
    old = "".join(parts[si][1])
    assert len(parts[si][1]) == 1
    bits, pos = table.code_bits(sym) + ("1" if sym & 15 else ""), 0
    for _, blk, kind, sg, p0, ncode, nextra in toks:
        code = old[p0:p0 + ncode]
        if ncode:
            code = table.code_bits(tab.matches(code))
        bits += code + old[p0 + ncode:p0 + ncode + nextra]
    bits += "1" * (-len(bits) % 8)
    pre = parts[si][0]
    k = pre.index(b"\xff\xc4")
    ln = (pre[k + 2] << 8) | pre[k + 3]
    parts[si] = (pre[:k] + J._seg(0xC4, table.segment(1, pre[k + 4] & 15)) + pre[k + 2 + ln:], [bits])
    return P.assemble(parts)
