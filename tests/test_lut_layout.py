"""The two-level decode tables of the entropy decoder (pjd_internal.h, PjdDevTset; built by pjd_lut_build.h on the device and, through
pjd_plan_luts, on the host), checked on the CPU against a naive canonical matcher.

A 9-bit prefix that starts codes longer than 9 bits has a second-level table of 2^k entries, 9 + k the longest code under it, instead
of 128 whatever the codes are.  For every table of every case below and every one of the 65,536 sixteen-bit windows the lookup -- the
first-level entry, or for a pointer entry (low five bits zero) the u16 at its byte offset (bits 31..16) indexed by the top k of the seven
bits behind the prefix (bits 9..5 hold 32 - k) -- must give the 16-bit entry of the symbol a scan over the codes finds, shortest match
first: bits used (code length + value bits), run + 1, EOB, size, which name the symbol and its code length; and the invalid marker (16
bits used, size 14) where no code matches.  First-level entries whose code fits nine bits are compared as whole 32-bit words, pair
fields included, with entries made from the same matcher: the layout of the second level must not have moved them.  Sizes: the blob is
the first levels + 2 * 2^k per long prefix (recomputed here), never more than the NOMINAL size (256 bytes per long prefix:
symbol_corpus._second_level_bytes), and a set has a blob exactly where the nominal size fits PJD_LUT_LDS_MAX -- routing is the old rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)

import symbol_corpus as sc
from jpeg_symbols import Table

BAD = 16 | (1 << 5) | (14 << 12)                      # PJD_LUT_ENTRY(16, 1, false, PJD_LUT_BADSYM)
W16 = np.arange(65536, dtype=np.int64)


# ---- the naive matcher: generate_codes restated, shortest match wins ---------------------------------------------------------------
_NAIVE = {}


def naive(t):
    """-> (length[65536], symbol[65536]) of the code each 16-bit window starts with; length 0: none.  (Kept per table: read-only.)"""
    key = (tuple(t.counts), tuple(t.symbols))
    if key not in _NAIVE:
        if len(_NAIVE) > 16:
            _NAIVE.clear()
        _NAIVE[key] = _naive(t)
    return _NAIVE[key]


def _naive(t):
    ln_of, sym_of = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    symbols = np.array(list(t.symbols) + [0], np.int64)
    code, q = 0, 0
    for ln in range(1, 17):
        cnt = t.counts[ln - 1]
        c = W16 >> (16 - ln)
        hit = (ln_of == 0) & (c >= code) & (c < code + cnt) & (c < (1 << ln))
        ln_of[hit] = ln
        sym_of[hit] = symbols[q + c[hit] - code]
        q += cnt
        code = (code + cnt) << 1
    return ln_of, sym_of


def entry(ln, sym, ac):
    """The 16-bit entry of symbol `sym` with a code of `ln` bits (arrays), as pjd_internal.h lays it out."""
    bad = np.where(sym == 0xFF, 14, 0)
    if ac:
        run, size, eob = sym >> 4, sym & 15, sym == 0
        bad = np.where((bad == 0) & ~eob & (size > 10), 15, bad)
    else:
        run, size, eob = np.zeros_like(sym), sym, np.zeros(sym.shape, bool)
        bad = np.where((bad == 0) & (sym > 11), 15, bad)
    used = ln + np.where(bad > 0, 0, size)
    return used | (np.where(eob, 32, run + 1) << 5) | (eob.astype(np.int64) << 11) | (np.where(bad > 0, bad, size) << 12)


def first_level(t, ac, partner):
    """The 512 first-level words whose code fits nine bits (else -1), pair fields included; `partner`: the AC table of the pair's second symbol."""
    idx = np.arange(512, dtype=np.int64)
    ln, sym = naive(t)
    ln9, sym9 = ln[idx << 7], sym[idx << 7]
    m = entry(ln9, sym9, ac)
    used, size = m & 31, (m >> 12) & 15
    can = (ln9 > 0) & (ln9 <= 9) & ((m & 0x800) == 0) & (size < 14) & (used < 9)
    rest = 9 - np.minimum(used, 9)
    ln2, sym2 = naive(partner)
    w2 = (((idx << np.minimum(used, 9)) & 0x1FF) << 7)
    l2, s2 = ln2[w2], sym2[w2]
    m2 = entry(l2, s2, True)
    can &= (l2 > 0) & (l2 <= rest) & (((m2 >> 12) & 15) < 14) & (used + (m2 & 31) <= 31)
    pair = np.where(can, (used + (m2 & 31)) | ((((m >> 5) & 127) + ((m2 >> 5) & 127)) << 5) | (((m2 >> 12) & 15) << 12), m & 0xFFF)
    return np.where((ln9 > 0) & (ln9 <= 9), (m & 0xFFFF) | (pair << 16), -1)


def prefix_range(t):
    """[p0, p1) of symbol_corpus._second_level_bytes."""
    code, end9 = 0, 0
    for ln in range(1, 17):
        code += t.counts[ln - 1]
        if ln == 9:
            end9 = code
        if ln < 16:
            code <<= 1
    p0, p1 = min(end9, 512), min((code + 127) >> 7, 512)
    return p0, max(p1, p0)


def second_level_real(t):
    """Sum over the long prefixes of 2 * 2^k, 9 + k the longest code under the prefix (k = 1 where none)."""
    ln, _ = naive(t)
    p0, p1 = prefix_range(t)
    longest = ln.reshape(512, 128).max(axis=1)
    return sum(2 << max(int(longest[p]) - 9, 1) for p in range(p0, p1))


def lookup(blob, slot):
    """lut_lookup_pair of pjd_k_huffman.hip for every 16-bit window, restated: the low half of what it returns."""
    l1 = blob[slot * 2048: slot * 2048 + 2048].view(np.uint32).astype(np.int64)
    b16 = blob.view(np.uint16).astype(np.int64)
    e = l1[W16 >> 7]
    ptr = (e & 31) == 0
    pk = W16 << 16                                     # the window at the top of a 32-bit word
    at = (e >> 16) + 2 * (((pk << 9) & 0xFFFFFFFF) >> ((e >> 5) & 31))
    assert not ptr.any() or (at[ptr].max() + 2 <= blob.size and (at[ptr] % 2 == 0).all()), "a pointer entry leads outside the blob"
    e2 = b16[np.where(ptr, at, 0) >> 1]
    return np.where(ptr, e2, e & 0xFFFF), ptr, l1


# ---- descriptors ---------------------------------------------------------------------------------------------------------------------
_BASE = {}


def base_desc(ncomp):
    import pjd_amd
    import synth
    if ncomp not in _BASE:
        s = pjd_amd.Scanned(synth.make(32, 16, 7, 85, synth.SUB_GREY if ncomp == 1 else synth.SUB_444, 0))
        assert s.valid
        _BASE[ncomp] = s
    d = pjd_amd.ImageDesc()
    C.memmove(C.byref(d), C.byref(_BASE[ncomp].desc), C.sizeof(pjd_amd.ImageDesc))
    return d


def put(h, t):
    off = 0
    h.offsets[0] = 0
    for ln in range(1, 17):
        off += t.counts[ln - 1]
        h.offsets[ln] = off
    for k in range(162):
        h.symbols[k] = t.symbols[k] if k < len(t.symbols) else 0
    h.set = 1


def desc_of(dc, ac, assign):
    """dc, ac: {id: Table}; assign: per component (DC id, AC id)."""
    d = base_desc(len(assign))
    for i, t in dc.items():
        put(d.dc[i], t)
    for i, t in ac.items():
        put(d.ac[i], t)
    for c, (td, ta) in enumerate(assign):
        d.comp_dc[c], d.comp_ac[c] = td, ta
    return d


def tables_of_desc(d):
    def tab(h):
        return Table([h.offsets[ln] - h.offsets[ln - 1] for ln in range(1, 17)], list(h.symbols[: h.offsets[16]]), oversubscribed=True)
    return [(tab(d.dc[d.comp_dc[c]]), tab(d.ac[d.comp_ac[c]])) for c in range(d.num_components)]


def check_set(label, d):
    """Everything the docstring promises for the table set of descriptor d.  -> (real size, nominal size)."""
    import pjd_amd
    blob, nominal, slots = pjd_amd.plan_luts(d)
    comps = tables_of_desc(d)
    by_slot = {}
    for c, (dct, act) in enumerate(comps):
        by_slot.setdefault(slots[c][1], (act, True, act))
        by_slot.setdefault(slots[c][0], (dct, False, act))
    assert sorted(by_slot) == list(range(len(by_slot))), (label, slots)
    oversub = any(t.oversubscribed for t, _, _ in by_slot.values())
    want_nominal = len(by_slot) * sc.L1_BYTES + sum(sc._second_level_bytes(t) for t, _, _ in by_slot.values())
    if oversub:                                        # not a prefix code: no decode tables (symbol_corpus.tables_fit says so before it counts)
        assert blob.size == 0, label
        return 0, nominal
    assert nominal == want_nominal, (label, nominal, want_nominal)
    assert (blob.size > 0) == (nominal <= sc.LUT_LDS_MAX), (label, blob.size, nominal)      # routing: the nominal size against the old limit
    if blob.size == 0:
        return 0, nominal
    want_real = len(by_slot) * sc.L1_BYTES + sum(second_level_real(t) for t, _, _ in by_slot.values())
    assert blob.size == (want_real + 15) // 16 * 16, (label, blob.size, want_real)
    assert blob.size <= nominal, (label, blob.size, nominal)
    for slot, (t, ac, partner) in by_slot.items():
        ln, sym = naive(t)
        want = np.where(ln > 0, entry(ln, sym, ac), BAD)
        got, ptr, l1 = lookup(blob, slot)
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (label, slot, f"window {diff[0]:016b}: entry {got[diff[0]]:#06x}, the matcher says {want[diff[0]]:#06x} ({diff.size} windows differ)")
        p0, p1 = prefix_range(t)
        assert (ptr == (((W16 >> 7) >= p0) & ((W16 >> 7) < p1))).all(), (label, slot, "pointer entries exactly at the long prefixes")
        assert (ln[ptr] != 0).any() == (p1 > p0) and (ln[ptr] <= 9).sum() == (ln[ptr] == 0).sum(), (label, slot)
        w32 = first_level(t, ac, partner)
        short = w32 >= 0
        assert (l1[short] == w32[short]).all(), (label, slot, "a first-level entry of a short code moved")
        rest = np.ones(512, bool)
        rest[short] = False
        rest[p0:p1] = False
        assert (l1[rest] == (BAD | ((BAD & 0xFFF) << 16))).all(), (label, slot, "a prefix no code starts with")
    return blob.size, nominal


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
AC_SYMS = [s for s in sc.BASELINE_AC if s] + sc.SIZE0_RUNS          # 175 distinct valid symbols besides the EOB


def ac_table(counts):
    n = sum(counts)
    return Table(counts, ([0x00] + AC_SYMS)[:n])


def shaped():
    """name -> AC table of a given code-length profile (the DC table beside it is symbol_corpus.dc_general)."""
    T = {}
    T["no code over 9 bits"] = ac_table([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0])
    T["a single 16-bit code"] = ac_table([1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1])
    # 2 ten-bit codes fill a prefix, 4 eleven-bit ones the next, ...: one prefix per length 10..15, then a 16-bit code in a seventh
    T["every length 10 to 16, distinct prefixes"] = ac_table([1, 1, 1, 1, 1, 1, 0, 0, 0, 2, 4, 8, 16, 32, 64, 1])
    T["a prefix with two lengths (11 and 13)"] = ac_table([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 0, 0])
    T["a complete 16-bit tree"] = ac_table([1] * 15 + [2])
    T["the code space ends in a hole"] = ac_table([0, 2, 2, 2, 2, 2, 2, 2, 1, 3, 3, 3, 3, 3, 3, 3])     # 3 / 65536 of the code space stay free
    T["every code 16 bits long"] = sc.ac_all16()
    return T


@pytest.mark.parametrize("name", list(shaped()))
def test_table_shapes(name):
    act = shaped()[name]
    dct = sc.dc_general()
    real, nominal = check_set(name, desc_of({0: dct}, {0: act}, [(0, 0)]))
    assert real > 0
    if name == "no code over 9 bits":
        assert second_level_real(act) == 0 and real == 2 * 2048 + second_level_real(dct)
    if name == "every length 10 to 16, distinct prefixes":
        assert second_level_real(act) == 2 * (2 + 4 + 8 + 16 + 32 + 64 + 128)
    if name == "a prefix with two lengths (11 and 13)":
        assert second_level_real(act) == 2 * 16
    # the same profile as a DC table (sizes 0..15 and 0xFF as its symbols, over and over), paired with the Annex-K-like general AC table
    n = sum(act.counts)
    as_dc = Table(act.counts, ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 0xFF] * 11)[:n])
    check_set(name + " (as a DC table)", desc_of({0: as_dc}, {0: sc.ac_general()}, [(0, 0)]))


def test_annex_k_tables():
    """The four tables of T.81 Annex K (what the workload generator writes without optimisation): the figures of DESIGN.md."""
    import pjd_amd
    import synth
    s = pjd_amd.Scanned(synth.make(64, 48, 7, 85, synth.SUB_420, 0))
    real, nominal = check_set("annex K", s.desc)
    acs = [a for _, a in tables_of_desc(s.desc)]
    assert sorted({sum(t.counts) for t in acs}) == [162] and acs[0].counts[15] == 125           # luma AC: 125 sixteen-bit codes
    assert real < nominal
    print(f"annex K: {real} B of {nominal} B nominal")


def test_edge_family_shapes():
    """The table sets of symbol_corpus.edge_family(): the general tables in every sampling, the 162-symbol table, the over-subscribed one."""
    seen = set()
    frames = [sc.edge_frame(w, h, sub, q, q16, ri=ri, std=std, ac=({0: sc.ac_oversub(), 1: sc.ac_general()} if act == "oversub" else None))
              for (w, h, sub, q, q16, ri, std, act) in sc.DC_EDGE_FRAMES.values()] + [sc.deq_edge_frame()]
    n_oversub = 0
    for fr in frames:
        assign = [(c.td, c.ta) for c in fr.comps]
        key = (tuple(assign), tuple((i, tuple(t.counts), tuple(t.symbols)) for i, t in sorted(fr.dc.items())),
               tuple((i, tuple(t.counts), tuple(t.symbols)) for i, t in sorted(fr.ac.items())))
        if key in seen:
            continue
        seen.add(key)
        d = desc_of(fr.dc, fr.ac, assign)
        real, nominal = check_set(f"edge family {len(seen)}", d)
        assert (real > 0) == sc.tables_fit(fr)
        n_oversub += real == 0
    assert len(seen) >= 3 and n_oversub == 1


def random_counts(rng):
    """A count vector that satisfies Kraft: 2..162 code lengths drawn towards the long end, lengthened one by one until they fit."""
    n = int(rng.integers(2, 163))
    lens = np.sort(rng.integers(int(rng.integers(1, 10)), 17, n))
    counts = [int((lens == ln).sum()) for ln in range(1, 17)]
    while sc.kraft(counts) > 1:
        k = min(i for i in range(15) if counts[i])      # the shortest code weighs most
        counts[k] -= 1
        counts[k + 1] += 1
    if sc.kraft(counts) > 1:                            # 162 sixteen-bit codes fit any tree: not reached
        raise AssertionError(counts)
    return counts


def test_random_count_vectors():
    rng = np.random.default_rng(20480)
    n_blob = n_routed = n_second = 0
    for k in range(200):
        ca, cd = random_counts(rng), random_counts(rng)
        pool = np.array([0x00] + AC_SYMS + [0xFF, 0x0B, 0x1C, 0x2F])
        act = Table(ca, [int(x) for x in rng.choice(pool, sum(ca), replace=False)])
        dct = Table(cd, [int(x) for x in rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 0xFF], sum(cd))])
        three = k % 2 == 1                              # every other case: three components, chroma with tables of its own
        if three:
            act2 = Table(ca, list(reversed(act.symbols)))
            d = desc_of({0: dct, 1: dct}, {0: act, 1: act2}, [(0, 0), (1, 1), (0, 1)])
        else:
            d = desc_of({0: dct}, {0: act}, [(0, 0)])
        real, nominal = check_set(f"random {k}", d)
        n_blob += real > 0
        n_routed += real == 0
        n_second += real > 0 and real < nominal
    assert n_blob >= 50 and n_routed >= 5 and n_second >= 50, (n_blob, n_routed, n_second)      # both sides of the routing rule, and sized tables, are in the draw


def test_default_workload_blob():
    """The flagship workload (bench.py: seeded cfg3_imagenet_like, tables fitted per picture): the largest blob of its first 64 pictures
    sizes the dynamic LDS of the entropy decoder; 8,768 B where it was 11,520 B.  The cap is that figure rounded up to the next 256 B."""
    import pjd_amd
    import synth
    jpegs = synth.cfg3_imagenet_like(64, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    sizes, nominals = [], []
    for j in jpegs:
        s = pjd_amd.Scanned(j)
        blob, nominal, _ = pjd_amd.plan_luts(s.desc)
        sizes.append(blob.size)
        nominals.append(nominal)
    print(f"first 64 pictures of the default workload: largest blob {max(sizes)} B (mean {np.mean(sizes):.0f}), nominal {max(nominals)} B (mean {np.mean(nominals):.0f})")
    assert min(sizes) > 0 and max(sizes) <= 8960
    assert all(r <= n for r, n in zip(sizes, nominals))
    s = pjd_amd.Scanned(jpegs[0])
    check_set("default workload, picture 0", s.desc)
