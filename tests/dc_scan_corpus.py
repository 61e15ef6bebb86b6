"""Streams for the DC prediction across entropy-decoder lanes (pjd_k_lane_dc_local / _carry and pjd_k_group_dc, pjd_k_backend.hip).

The entropy decoder leaves DC DIFFERENCES and per-lane sums; the predictor at every lane start is a segmented prefix sum over lanes, in
blocks (or, per picture, chunks) of DC_BLOCK = 256 lanes with a carry between them, modulo 2^16.  Here every stream is hand-built
(tests/jpeg_symbols.py) so that at PJD_SUB_BYTES=128 -- a lane is 128 bytes of the destuffed stream, the planner's per-picture
adjustment is off -- its lanes, and the lanes that start a restart segment ("heads": the sum restarts at 0 there), lie where the scan's
carries change hands.  DC differences are drawn over the whole +-2047 range, each component from another distribution, so that the lane
sums, the block aggregates and the running predictor leave 16 bits again and again.  AC symbols only size the units.

`corpus()` -> [(label, jpeg, frame, intent)] (the shape tests/test_gpu_symbol_streams.py takes); `MEMBERS` says per label what the member
is there for and which segment lane counts it was built to; `layout()` is the lane layout restated in plain Python from a descriptor.
The batch compositions of tests/test_gpu_dc_scan.py (`offsets_order`, `carry_batch`, `group_batch`) are here too, so that
tests/test_dc_scan_cpu.py can hold them against the model without a GPU.

Build time of the whole corpus (about 2.2 MB of stream, 90,000 units): see BUILD_SECONDS."""
import functools
import math

import numpy as np

import jpeg_symbols as J
import symbol_corpus as SC

S = 128                      # PJD_SUB_BYTES of every test that uses the lane model
DC_BLOCK = 256               # PJD_DC_BLOCK (pjd_internal.h)
PICTURE_MAX_LANES = 2048     # PJD_DC_PICTURE_MAX_LANES: the single chain takes the per-picture form up to this many lanes per picture
GROUP_MAX_LANES = 8192       # pjd_plan.cpp: no picture groups with a picture of more lanes
GROUP_MIN_PICTURES = 64
BUILD_SECONDS = 10           # measured: the whole corpus on one core of the build machine (the three ~2048-lane members: 1 s each)

LADDER = [1, 2, 64, 65, 255, 256, 257, 512, 513, 2047, 2048, 2049]
FULL, UP, DOWN, MIXED = "full", "up", "down", "mixed"        # distributions of a component's DC differences


def _diff(rng, dist):
    if dist == FULL:
        return int(rng.integers(-2047, 2048))
    if dist == UP:
        return int(rng.integers(0, 2048))
    if dist == DOWN:
        return int(rng.integers(-2047, 1))
    return int(rng.integers(-2047, 2048)) if rng.random() < 0.3 else int(rng.integers(1024, 2048))      # MIXED: mostly large steps up


# ---- the lane layout, restated --------------------------------------------------------------------------------------------------------
class Layout:
    """Lanes of one picture at S bytes: `lanes` [(first byte, end byte)] of the destuffed stream in lane order, `heads` the
    picture-local indices of the lanes that start a restart segment (lane 0 among them), `seg_lanes` the lanes of each segment."""

    def __init__(self, seg_offsets, ecs_len, s=S):
        bounds = list(seg_offsets) + [ecs_len]
        self.lanes, self.heads, self.seg_lanes = [], [], []
        for b0, b1 in zip(bounds, bounds[1:]):
            n = max(1, -(-(b1 - b0) // s))
            self.heads.append(len(self.lanes))
            self.seg_lanes.append(n)
            self.lanes += [(b0 + j * s, min(b0 + (j + 1) * s, b1)) for j in range(n)]
        self.n = len(self.lanes)

    def without_unit_start(self, unit_bit):
        """Lanes in which no data unit starts (unit_bit: where each unit starts in the destuffed, marker-free scan)."""
        starts = np.asarray(unit_bit, np.int64)
        return [k for k, (b0, b1) in enumerate(self.lanes)
                if np.searchsorted(starts, 8 * b0, "left") == np.searchsorted(starts, 8 * b1, "left")]


def layout(scanned, s=S):
    """The layout of a pjd_amd.Scanned: from its descriptor's seg_offsets / ecs_len alone."""
    d = scanned.desc
    offs = [int(x) for x in scanned.seg_offsets()] if int(d.restart_interval) else [0]
    return Layout(offs, int(d.ecs_len), s)


# ---- building a stream to a lane layout ---------------------------------------------------------------------------------------------
def _frame(mcus_w, mcus_h, sub, ac, ri=0, std=False, crop=(3, 5)):
    """Luma on `ac`, chroma on the 162-symbol table: with one table for all components a lane's decoder cannot tell which unit of
    the MCU it is in (class PHASE of tests/nosync_corpus.py: such pictures go to the exact kernel, which is not what this is about)."""
    comps = {"2c": [(1, 1), (1, 1)]}.get(sub) or SC.SAMPLINGS[sub]
    hs, vs = comps[0]
    w, h = max(1, 8 * hs * mcus_w - crop[0]), max(1, 8 * vs * mcus_h - crop[1])
    cs = [J.Component(hh, vv, min(j, 1), min(j, 1), min(j, 1)) for j, (hh, vv) in enumerate(comps)]
    qt = {t: [1 + ((k * 3 + t) % 4) for k in range(64)] for t in {c.tq for c in cs}}               # small quantisers
    dc = {t: SC.dc_general() for t in {c.td for c in cs}}
    acs = {0: ac, 1: SC.ac_162()} if len(cs) > 1 else {0: ac}
    return J.Frame(w, h, cs, dc, acs, qt=qt, ri=ri, standard_restart=std)


def _dims(n_mcu):
    w = max(1, math.isqrt(n_mcu))
    return w, -(-n_mcu // w)


class _Ac:
    """What the builder needs of one AC table: code lengths, the symbols it draws from (runs up to 2, sizes 1..10) and, to fill a
    unit slot by slot, those without a run."""

    def __init__(self, act):
        self.len = {s: len(act.code_bits(s)) for s in set(act.symbols) if s in act.code_of}
        self.eob = self.len[0x00]
        self.syms = [s for s in SC.valid_symbols(act, True) if (s >> 4) <= 2 and (s & 15) >= 1]
        self.fill = [s for s in self.syms if (s >> 4) == 0]


class _Builder:
    """Units of one frame, restart segment by restart segment, each grown or cut to its number of lanes."""

    def __init__(self, fr, rng, dists):
        self.fr, self.rng, self.dists = fr, rng, dists
        self.per = fr.unit_comps()
        self.acs = [_Ac(fr.ac[c.ta]) for c in fr.comps]
        self.units, self.bits, self.diffs = [], [], []

    def ac(self, u):
        return self.acs[self.per[u % len(self.per)]]

    def _dc(self, u):
        c = self.per[u % len(self.per)]
        d = _diff(self.rng, self.dists[c % len(self.dists)])
        t = J.dcv(d)
        dct = self.fr.dc[self.fr.comps[c].td]
        return d, t, len(dct.code_bits(t[1])) + t[1]

    def _ac(self, a, s):
        sz = s & 15
        return J.AC(s >> 4, sz, int(self.rng.integers(0, 1 << sz))), a.len[s] + sz

    def unit(self, u, want_bits):
        d, t, bits = self._dc(u)
        toks, slot = [t], 1
        a = self.ac(u)
        while slot < 64 and bits < want_bits:
            s = a.syms[int(self.rng.integers(len(a.syms)))]
            if slot + (s >> 4) > 63:
                break
            tok, nb = self._ac(a, s)
            toks.append(tok)
            bits += nb
            slot += (s >> 4) + 1
        if slot < 64:
            toks.append(J.EOB)
            bits += a.eob
        self.units.append(toks)
        self.bits.append(bits)
        self.diffs.append(d)

    @staticmethod
    def _slot(toks):
        return 1 + sum(t[1] + 1 for t in toks[1:] if t != J.EOB)

    def segment(self, first, count, lanes):
        """Units first .. first + count - 1 with a mean of bits that lands inside the `lanes`-th lane, then AC symbols appended to (or
        taken from) the last units until the padded segment is more than (lanes - 1) * S bytes and at most lanes * S."""
        lo, hi = 8 * S * (lanes - 1) + 1, 8 * S * lanes - 7          # bits; the segment is padded to a byte
        mean = 0.97 * 8 * S * (lanes - 0.5) / count
        for u in range(first, first + count):
            self.unit(u, mean * self.rng.uniform(0.6, 1.4))
        total = sum(self.bits[first:first + count])
        for u in range(first + count - 1, first - 1, -1):
            if lo <= total <= hi:
                break
            toks, a = self.units[u], self.ac(u)
            if toks[-1] == J.EOB:
                toks.pop()
                self.bits[u] -= a.eob
                total -= a.eob
            slot = self._slot(toks)
            while total + (a.eob if slot < 64 else 0) < lo and slot < 64:
                tok, nb = self._ac(a, a.fill[int(self.rng.integers(len(a.fill)))])
                toks.append(tok)
                self.bits[u] += nb
                total += nb
                slot += 1
            while total + (a.eob if slot < 64 else 0) > hi and len(toks) > 1:
                t = toks.pop()
                nb = a.len[(t[1] << 4) | t[2]] + t[2]
                self.bits[u] -= nb
                total -= nb
                slot -= t[1] + 1
            if slot < 64:
                toks.append(J.EOB)
                self.bits[u] += a.eob
                total += a.eob
        assert lo <= total <= hi, ("the segment does not reach its lanes", lanes, count, total)


def _segments(fr):
    """(first unit, units) of every restart segment."""
    per = len(fr.unit_comps())
    cuts = [0] + sorted(m * per for m in fr.restarts_before()) + [fr.n_units()]
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


def build(fr, seg_lanes, seed, dists=(FULL, UP, DOWN)):
    """-> (jpeg, intent, diffs): `fr` with its k-th restart segment seg_lanes[k] lanes long at S bytes."""
    b = _Builder(fr, np.random.default_rng(seed), dists)
    segs = _segments(fr)
    assert len(segs) == len(seg_lanes), (len(segs), len(seg_lanes))
    for (first, count), lanes in zip(segs, seg_lanes):
        b.segment(first, count, lanes)
    data, it = J.write(fr, b.units)
    return data, it, b.diffs


def _sized(sub, seg_lanes, unit_bytes=25, std=False):
    """A frame whose restart segments (equal numbers of MCUs) hold about unit_bytes per unit at their mean number of lanes."""
    per = sum(h * v for h, v in ({"2c": [(1, 1), (1, 1)]}.get(sub) or SC.SAMPLINGS[sub]))
    nseg = len(seg_lanes)
    if nseg == 1:
        mw, mh = _dims(max(1, round(S * (seg_lanes[0] - 0.5) / unit_bytes / per)))
        return _frame(mw, mh, sub, SC.ac_general())
    ri = max(1, round(S * max(seg_lanes[:-1]) / unit_bytes / per))
    tail = max(1, round(S * seg_lanes[-1] / unit_bytes / per))            # the last segment is as short as its lanes ask
    mw, mh = _dims(ri * (nseg - 1) + min(tail, ri))
    if mw * mh - ri * (nseg - 1) > ri:
        ri = -(-(mw * mh) // nseg)
    assert -(-(mw * mh) // ri) == nseg, (sub, seg_lanes)
    return _frame(mw, mh, sub, SC.ac_general(), ri=ri, std=std)


# ---- wraps, asserted on the intent ---------------------------------------------------------------------------------------------------
def predictor_wraps(fr, it, diffs):
    """How often the running predictor left int16: units whose absolute DC is not their predecessor's plus their difference."""
    per = fr.unit_comps()
    rst = {m * len(per) for m in fr.restarts_before()}
    pred, n = [0] * len(fr.comps), 0
    for u in range(it.n_decoded):
        if u in rst:
            pred = [0] * len(fr.comps)
        c = per[u % len(per)]
        dc = int(it.slots[u, 0])
        n += dc != pred[c] + diffs[u]
        assert dc == J.wrap16(pred[c] + diffs[u])
        pred[c] = dc
    return n


def block_sums(fr, it, diffs, lay):
    """Per block of DC_BLOCK picture-local lanes and component: the sum of the differences of the units that start in the block's
    lanes behind its last head (what the block's aggregate holds before it is cut to 16 bits)."""
    per = fr.unit_comps()
    starts = np.asarray(it.unit_bit, np.int64)
    out = []
    for b0 in range(0, lay.n, DC_BLOCK):
        b1 = min(b0 + DC_BLOCK, lay.n)
        h = max([x for x in lay.heads if b0 <= x < b1], default=b0)
        u0, u1 = np.searchsorted(starts, 8 * lay.lanes[h][0]), np.searchsorted(starts, 8 * lay.lanes[b1 - 1][1])
        s = [0] * len(fr.comps)
        for u in range(u0, min(u1, it.n_decoded)):
            s[per[u % len(per)]] += diffs[u]
        out.append(s)
    return out


# ---- the members ---------------------------------------------------------------------------------------------------------------------
MEMBERS = {}         # label -> dict(seg_lanes=[...] or None, why=...)
_DIFFS = {}          # label -> the DC difference of every unit


def _add(out, label, fr, data, it, diffs, seg_lanes, why):
    out.append((label, data, fr, it))
    MEMBERS[label] = dict(seg_lanes=seg_lanes, why=why)
    _DIFFS[label] = diffs


def _ladder(out):
    why = {1: "one lane: a head and nothing to add", 2: "the smallest carry inside a chunk", 64: "one full wave", 65: "a wave and a lane",
           255: "one lane short of a block", 256: "exactly one block / chunk", 257: "one lane into the second block: the first carry",
           512: "two full chunks", 513: "the carry of a carry", 2047: "a lane short of the per-picture limit",
           2048: "the largest picture of the per-picture form", 2049: "the smallest picture that takes the three-launch scan"}
    for n in LADDER:
        fr = _sized("444", [n])
        data, it, diffs = build(fr, [n], 1000 + n)
        _add(out, f"ladder{n}", fr, data, it, diffs, [n], why[n])


def _heads(out):
    for label, sub, seg_lanes, why in [
            ("heads_255_511", "444", [255, 256, 40], "heads on the last lane of the first and of the second block"),
            ("heads_256_512", "grey", [256, 256, 40], "heads on the first lane of the second and of the third block"),
            ("heads_257", "grey", [257, 30], "a head one lane into the second block: the carry must stop at it"),
            ("heads_single_1024", "444", [1024, 1024], "one head on the first lane of a block, between two stretches of 1023 headless lanes: "
                                                       "whole blocks without a head on either side (the carry passes through them)")]:
        fr = _sized(sub, seg_lanes)
        data, it, diffs = build(fr, seg_lanes, 2000 + len(out), dists=(UP, DOWN, FULL))
        _add(out, label, fr, data, it, diffs, seg_lanes, why)
    # every lane a head: one MCU per restart segment, each at most S bytes
    fr = _frame(24, 24, "444", SC.ac_general(), ri=1)
    seg_lanes = [1] * 576
    data, it, diffs = build(fr, seg_lanes, 2100, dists=(MIXED, FULL, DOWN))
    _add(out, "heads_every_lane", fr, data, it, diffs, seg_lanes, "every lane a head, over three blocks: nothing may be carried anywhere")


def _fat(out):
    """Ordinary units up to lane 249, fifteen units of 63 AC symbols with 16-bit codes and mostly 10-bit values (180-205 bytes each: lanes
    in which no unit starts, across the edge of the first block), ordinary units behind.  Grey: the run needs 16-bit codes in
    consecutive units, and colour components on one AC table are not for the parallel path (_frame)."""
    fr = _frame(40, 40, "grey", SC.ac_all16(), crop=(1, 7))
    b = _Builder(fr, np.random.default_rng(3000), (MIXED,))
    a = b.acs[0]
    big = [s for s in a.fill if (s & 15) == 10]
    mid = [s for s in a.fill if 5 <= (s & 15) <= 9]
    u, fat_units = 0, []
    while u < fr.n_units():
        if not fat_units and sum(b.bits) >= 8 * S * 249:
            for _ in range(15):
                d, t, bits = b._dc(u)
                toks = [t]
                for k in range(63):
                    tok, nb = b._ac(a, big[int(b.rng.integers(len(big)))] if b.rng.random() < 0.7 else mid[int(b.rng.integers(len(mid)))])
                    toks.append(tok)
                    bits += nb
                b.units.append(toks); b.bits.append(bits); b.diffs.append(d)
                fat_units.append(u)
                u += 1
            continue
        b.unit(u, 200 * b.rng.uniform(0.6, 1.4))
        u += 1
    assert len(fat_units) == 15 and all(180 * 8 <= b.bits[k] <= 205 * 8 for k in fat_units), [b.bits[k] / 8 for k in fat_units]
    data, it = J.write(fr, b.units)
    _add(out, "fat_units", fr, data, it, b.diffs, None, "lanes in which no data unit starts (their sums are zero), across lane 256")
    MEMBERS["fat_units"]["fat_units"] = fat_units


def _samplings(out):
    for label, sub, ri_std, dists in [("samp_420", "420", False, (FULL, UP, DOWN)), ("samp_422", "422", False, (UP, DOWN, MIXED)),
                                      ("samp_440", "440", False, (DOWN, FULL, UP)), ("samp_420_dri_std", "420", True, (MIXED, DOWN, UP)),
                                      ("samp_grey", "grey", False, (UP,)), ("samp_2c", "2c", False, (DOWN, MIXED))]:
        seg_lanes = [130, 200, 140, 170] if ri_std else [640]
        fr = _sized(sub, seg_lanes, std=ri_std)
        data, it, diffs = build(fr, seg_lanes, 4000 + len(out), dists=dists)
        _add(out, label, fr, data, it, diffs, seg_lanes, f"{sub}: units of several components per MCU, each component another sum")


def _damaged(out):
    fr = _sized("444", [620])
    b = _Builder(fr, np.random.default_rng(5000), (FULL, UP, DOWN))
    b.segment(0, fr.n_units(), 620)
    u = fr.n_units() // 2 + 1
    units = SC.plant(fr, [list(x) for x in b.units], u, J.DC_SYM, b.rng, pick=7)          # pick 7: a code the table does not assign
    data, it = J.write(fr, units)
    assert it.status == J.DC_SYM and it.err_unit == u and "raw_dc" in it.forms
    _add(out, "damaged_620", fr, data, it, b.diffs, [620], "an unassigned code in the middle: the status, and the picture up to the error")


@functools.lru_cache(maxsize=1)
def corpus():
    out = []
    _ladder(out)
    _heads(out)
    _fat(out)
    _samplings(out)
    _damaged(out)
    return tuple(out)


def member(label):
    return next(x for x in corpus() if x[0] == label)


def clean():
    return [x for x in corpus() if x[3].status == J.OK]


def diffs_of(label):
    corpus()
    return _DIFFS[label]


def ladder(upto=LADDER[-1]):
    return [member(f"ladder{n}") for n in LADDER if n <= upto]


def heads_members():
    return [x for x in corpus() if x[0].startswith("heads_")]


def backend_members():
    """The members the back-end forms run: heads, fat units, samplings."""
    return [x for x in corpus() if x[0].startswith(("heads_", "fat_", "samp_"))]


def intended_lanes(label):
    """Lanes the member was built to (None: whatever its units make, fat_units)."""
    sl = MEMBERS[label]["seg_lanes"]
    return None if sl is None else sum(sl)


def many_lanes(mcus_w, mcus_h):
    """A grey picture of one-MCU restart segments of a byte or two: mcus_w * mcus_h lanes in a few kilobytes (for the planner's limit
    of GROUP_MAX_LANES lanes per picture; no decode test uses it)."""
    fr = _frame(mcus_w, mcus_h, "grey", SC.ac_general(), ri=1, crop=(0, 0))
    rng = np.random.default_rng(mcus_w * mcus_h)
    data, it = J.write(fr, [[J.dcv(int(rng.integers(-7, 8))), J.EOB] for _ in range(fr.n_units())])
    return ("many_lanes_%d" % (mcus_w * mcus_h), data, fr, it)


# ---- batch compositions --------------------------------------------------------------------------------------------------------------
def offsets_order(lanes):
    """An order of the clean corpus (labels) in which the lanes before ladder2049 are = 255, before ladder257 = 0 and before
    heads_single_1024 = 1 (mod DC_BLOCK): in the three-launch scan a block then ends on the 2049-lane picture's head, the 257-lane
    picture starts a block, and the single head sits one lane into one.  lanes: label -> lanes of the member at S bytes."""
    targets = [("ladder2049", 255), ("ladder257", 0), ("heads_single_1024", 1)]
    free = [l for l in lanes if l not in dict(targets)]
    order, total = [], 0
    for label, want in targets:
        need = (want - total) % DC_BLOCK
        # the fewest free members whose lanes add up to `need` modulo the block: breadth-first over residues
        reach = {0: []}
        frontier = [0]
        while need not in reach and frontier:
            nxt = []
            for r in frontier:
                for l in free:
                    if l in reach[r]:
                        continue
                    q = (r + lanes[l]) % DC_BLOCK
                    if q not in reach:
                        reach[q] = reach[r] + [l]
                        nxt.append(q)
            frontier = nxt
        assert need in reach, ("no members add up to", need)
        for l in reach[need]:
            free.remove(l)
            order.append(l)
            total += lanes[l]
        order.append(label)
        total += lanes[label]
    return order + free


CARRY_BATCHES = {
    # name -> (one-lane pictures in front, copies of ladder2049, last picture or None, the global lanes it is about)
    "headless_65536": (300, 32, None, "global lanes 65535..65537 inside the last copy's headless stretch, blocks 255 and 256 without a head: block 255 "
                                      "hands its carry to block 256, the first block of the carry kernel's second chunk"),
    "head_on_65536": (993, 31, "heads_single_1024", "the single head on global lane 65536: the first lane of block 256"),
    "head_on_65535": (992, 31, "heads_single_1024", "the single head on global lane 65535: the last lane of block 255"),
}


def carry_batch(name):
    """-> labels of the batch: k one-lane pictures, copies of the 2049-lane member, and the single-head member where the batch ends in it."""
    k, copies, last, _ = CARRY_BATCHES[name]
    return ["ladder1"] * k + ["ladder2049"] * copies + ([last] if last else [])


def group_batch():
    """-> labels: the ladder up to 2048 lanes, the heads members and the damaged member, four times over (68 pictures: the planner makes
    picture groups from 64 on)."""
    once = [x[0] for x in ladder(PICTURE_MAX_LANES)] + [x[0] for x in heads_members()] + ["damaged_620"]
    return once * 4
