"""Baseline streams on which a decoder started at a wrong state never falls into step with the true decode (test helper, seeded,
built on tests/jpeg_symbols.py; nothing is committed as a file).

The parallel entropy decoder starts one speculative decoder per lane (every S bytes of a restart segment) at "DC expected, unit 0 of
the MCU" and relies on it meeting the true decode soon.  On these streams it does not:

  class 1  LOCKSTEP   every symbol is 8 bits (a 4-bit code and 4 value bits), every unit 63 bytes for 64 slots and no EOB: a decoder
                      started at any byte reads one symbol per byte whatever table it believes in, so its bit position always agrees
                      and its zigzag slot never does (only a lane that starts on a unit boundary holds the truth)
  class 2  CHAINS     class 1 with SYNCHRONISER units (DC, three coefficients, an 8-bit EOB that the DC table reads as size 0) in
                      chosen lanes: every decoder that is in a unit's AC part lands on "DC expected" there, so the runs of lanes in
                      between are chains of a chosen length; a 62-byte unit keeps unit boundaries off the lane starts of a chain
  class 3  PHASE      ordinary random units with EOBs, all components on ONE DC and ONE AC table: position and slot agree after a few
                      hundred bytes, the unit's place in the MCU cannot (the decode does not depend on it) until the segment ends
  class 4  HEADS      classes 1 and 3 with restart intervals of 1, 2 and about 100 lanes at 128 bytes: a segment's first lane holds
                      the truth, chains end there
  class 5  ERRORS     a class-2 picture with an error before / behind the wave its longest chain flags, and one cut short

`streams()` -> {name: Stream}; `members(S)` -> the streams decoded with lanes of S bytes; `Model` is a plain model of the state-only
pass (bit position, unit phase, zigzag slot) written from the reference's rules (src/jpeg_scanner.cpp:467-520), for the CPU tests.
"""
import functools

import numpy as np

import jpeg_symbols as J
import symbol_corpus as SC
from jpeg_symbols import AC, CUT, DC, EOB, Table

WAVE = 64                    # lanes per wave of the entropy decoder (pjd_internal.h PJD_HUFF_LANES)
UNIT_BYTES = 63


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def lock_ac(sync=False):
    """15 codes of 4 bits: 0000 -> 0x04 (run 0, size 4), 0001 -> 0x14, .. 1110 -> 0xE4; 1111 stays free (no 0xFF byte, no stuffing).
    sync: the 8-bit code 11110000 is the EOB."""
    return Table([0, 0, 0, 15, 0, 0, 0, int(sync)] + [0] * 8, [(r << 4) | 4 for r in range(15)] + ([0x00] if sync else []))


def lock_dc(sync=False):
    """15 codes of 4 bits, all of them size 4.  sync: 11110000 is size 0, so that DC and AC decoders both take that byte whole."""
    return Table([0, 0, 0, 15, 0, 0, 0, int(sync)] + [0] * 8, [4] * 15 + ([0] if sync else []))


# ---- units ----------------------------------------------------------------------------------------------------------------------------
class _Values:
    """Value nibbles: the AC ones at random; the DC difference (magnitude 8..15) always towards 0, so the predictor stays small."""

    def __init__(self, rng, ncomp):
        self.rng, self.pred, self.nib = rng, [0] * ncomp, iter(())

    def _nibble(self):
        for b in self.nib:
            return b
        self.nib = iter(self.rng.integers(0, 16, 8192).tolist())      # drawn in bulk: one call per nibble costs seconds over the corpus
        return next(self.nib)

    def dc(self, c):
        mag = 8 + self._nibble() % 8
        b = 15 - mag if self.pred[c] > 0 else mag
        self.pred[c] += J.extend(4, b)
        return DC(4, b)

    def ac(self, run=0):
        return AC(run, 4, self._nibble())


def full_unit(v, c):
    """DC, AC(1, 4), 61 x AC(0, 4): 64 slots in 63 bytes, no EOB."""
    return [v.dc(c), v.ac(1)] + [v.ac() for _ in range(61)]


def short_unit(v, c):
    """DC, 2 x AC(1, 4), 59 x AC(0, 4): 64 slots in 62 bytes, no EOB (moves the unit grid by one byte, synchronises nothing)."""
    return [v.dc(c), v.ac(1), v.ac(1)] + [v.ac() for _ in range(59)]


def sync_unit(v, c, n_ac=3):
    """DC, n_ac x AC(0, 4), EOB: n_ac + 2 bytes."""
    return [v.dc(c)] + [v.ac() for _ in range(n_ac)] + [EOB]


def _grid(n):
    """(columns, rows) with columns * rows == n, as square as n allows."""
    w = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return n // w, w


def lock_frame(sub, n_mcu, sync=False, ri=0, std=False):
    hs, vs = SC.SAMPLINGS[sub][0]
    mw, mh = _grid(n_mcu)
    return SC.frame(8 * hs * mw, 8 * vs * mh, sub, {0: lock_dc(sync)}, {0: lock_ac(sync)}, assign=[(0, 0)] * len(SC.SAMPLINGS[sub]),
                    ri=ri, std=std)


class Stream:
    """One file with its frame and intent, and what its design claims: cls (1..5), `chain` -- the longest run of lanes (at design_S
    bytes per lane) over which the truth has to travel lane by lane -- and `cross`, the most wave boundaries one such run crosses."""

    def __init__(self, name, cls, data, fr, it, design_S=None, chain=None, cross=None, note=""):
        self.name, self.cls, self.data, self.fr, self.it = name, cls, data, fr, it
        self.design_S, self.chain, self.cross, self.note = design_S, chain, cross, note
        self.sub = fr.sampling()

    def segments(self):
        """[(first byte, end byte)] of every restart segment in the destuffed, marker-free scan."""
        per = len(self.fr.unit_comps())
        nbytes = scan_bytes(self)
        starts = [0] + [self.it.unit_bit[m * per] // 8 for m in sorted(self.fr.restarts_before()) if m * per < len(self.it.unit_bit)]
        return list(zip(starts, starts[1:] + [nbytes]))

    def lane_starts(self, S):
        """[(first byte, starts a restart segment)] of every lane: every S bytes of each segment (pjd_plan.cpp)."""
        out = []
        for b0, b1 in self.segments():
            out += [(b, b == b0) for b in range(b0, max(b1, b0 + 1), S)]
        return out

    def n_lanes(self, S):
        return len(self.lane_starts(S))


@functools.lru_cache(maxsize=None)
def _scan_of(data):
    """The entropy-coded bytes as the decoder sees them: stuffing and restart markers removed."""
    sos = data.rindex(b"\xff\xda")                         # the entropy-coded bytes hold no marker but RSTn
    p = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    out = bytearray()
    while p < len(data):
        b = data[p]
        if b != 0xFF:
            out.append(b)
            p += 1
        elif p + 1 < len(data) and data[p + 1] == 0x00:
            out.append(0xFF)
            p += 2
        elif p + 1 < len(data) and 0xD0 <= data[p + 1] <= 0xD7:
            p += 2
        else:
            break
    return bytes(out)


def scan_bytes(stream):
    return len(_scan_of(stream.data))


# ---- class 1 ----------------------------------------------------------------------------------------------------------------------------
def lockstep(name, sub, n_mcu, seed, ri=0, std=False, cls=1):
    fr = lock_frame(sub, n_mcu, ri=ri, std=std)
    v = _Values(np.random.default_rng(seed), len(fr.comps))
    per = fr.unit_comps()
    units = [full_unit(v, per[u % len(per)]) for u in range(fr.n_units())]
    data, it = J.write(fr, units)
    assert it.status == J.OK and b"\xff\x00" not in data[data.rindex(b"\xff\xda"):]
    return Stream(name, cls, data, fr, it)


# ---- class 2 ----------------------------------------------------------------------------------------------------------------------------
def chain_units(S, n_lanes, sync_lanes, seed):
    """Grey units for n_lanes lanes of S bytes with one synchroniser in each of `sync_lanes`; no other lane start of the stream lies
    on a unit boundary.  -> (units, longest chain, most wave boundaries a chain crosses)."""
    v = _Values(np.random.default_rng(seed), 1)
    units, pos, todo = [], 0, sorted(sync_lanes)
    while pos <= (n_lanes - 1) * S:
        lane, off = divmod(pos, S)
        if todo and lane == todo[0] and off >= 1:
            u = sync_unit(v, 0)
            todo.pop(0)
        else:
            assert not todo or lane <= todo[0], "no unit starts inside a synchroniser's lane"
            u = short_unit(v, 0) if (pos + UNIT_BYTES) % S == 0 else full_unit(v, 0)
        units.append(u)
        pos += len(u)
    assert not todo
    true_lanes = [0] + sorted(sync_lanes) + [n_lanes]          # lanes whose exit is true without help, and the end
    runs = [(a + 1, b - 1) for a, b in zip(true_lanes, true_lanes[1:]) if b - 1 >= a + 1]
    chain = max(e - s + 1 for s, e in runs)
    cross = max(e // WAVE - (s - 1) // WAVE for s, e in runs)
    return units, chain, cross


def chains(name, S, n_lanes, sync_lanes, seed, edit=None, cls=2):
    units, chain, cross = chain_units(S, n_lanes, sync_lanes, seed)
    fr = lock_frame("grey", len(units), sync=True)
    if edit is not None:
        units = edit(fr, units)
    data, it = J.write(fr, units)
    assert b"\xff\x00" not in data[data.rindex(b"\xff\xda"):] or it.status != J.OK
    return Stream(name, cls, data, fr, it, design_S=S, chain=chain, cross=cross)


# ---- class 3 ----------------------------------------------------------------------------------------------------------------------------
def phase_only(name, sub, w, h, seed, ri=0, std=False, cls=3):
    n = len(SC.SAMPLINGS[sub])
    fr = SC.frame(w, h, sub, {0: SC.dc_general()}, {0: SC.ac_general()}, assign=[(0, 0)] * n, ri=ri, std=std)
    data, it = J.write(fr, SC.fill(fr, np.random.default_rng(seed)))
    assert it.status == J.OK
    return Stream(name, cls, data, fr, it)


# ---- class 5 ----------------------------------------------------------------------------------------------------------------------------
X5 = (128, 328, (40, 325))          # the class-2 picture whose chain crosses five wave boundaries (lanes 41..324)


def _full_from(units, u):
    while len(units[u]) != 63:
        u += 1
    return u


def _err_first_wave(fr, units):
    """An invalid AC code in a unit of the first wave (lane 10); the unit keeps its 63 bytes, so the design behind it stands."""
    u = _full_from(units, 10 * 128 // UNIT_BYTES)
    return SC.plant(fr, units, u, J.AC_SYM, np.random.default_rng(5), keep_n=60)


def _err_behind_flag(fr, units):
    """A run past slot 63 in lane 326 (wave 5 begins at lane 320): 1 + 2 + 47 slots, then run 14; padded to 63 bytes."""
    u = _full_from(units, 326 * 128 // UNIT_BYTES)
    units[u] = units[u][:49] + [AC(14, 4, 9)] + units[u][49:62]
    return units


def _cut_middle(fr, units):
    """The data ends inside a unit of lane 200 (of 328), in the middle of the chain."""
    u = _full_from(units, 200 * 128 // UNIT_BYTES)
    units[u] = units[u][:30] + [CUT(AC(0, 4, 5), "code")]
    return units[: u + 1]


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def streams():
    L = []
    # class 1, grey: 2, 63, 64, 65, 128, 129 lanes and 5..9 waves at 128 bytes; 2, 63, 64, 65 lanes at 1024
    for n in (3, 128, 129, 131, 260, 261, 650, 780, 910, 1040, 1170, 17, 1024, 1041):
        L.append(lockstep(f"lock_grey_{n}", "grey", n, 1000 + n))
    # class 1, 4:2:0 (378 bytes per MCU): 65 lanes, 6 and 9 waves at 128 bytes; 9, 48 and 65 lanes at 1024
    for n in (22, 130, 176):
        L.append(lockstep(f"lock_420_{n}", "420", n, 2000 + n))
    # class 2: chains of 2, 5 and 17 lanes inside a wave and 17 across a boundary; 63 and 70 lanes; across 3, 4 and 5 boundaries
    L.append(chains("chain_short", 128, 73, (3, 9, 27, 30, 48, 52, 70), 31))
    L.append(chains("chain_63", 128, 87, (20, 84), 32))
    L.append(chains("chain_70", 128, 94, (20, 91), 33))
    L.append(chains("chain_x3", 128, 204, (40, 201), 34))
    L.append(chains("chain_x4", 128, 264, (40, 261), 35))
    L.append(chains("chain_x5", *X5, 36))
    L.append(chains("chain_1024_66", 1024, 72, (3, 70), 37))
    # class 3
    L.append(phase_only("phase_420", "420", 256, 192, 41))
    L.append(phase_only("phase_422", "422", 256, 96, 42))
    L.append(phase_only("phase_444", "444", 120, 96, 43))
    L.append(phase_only("phase_420_big", "420", 544, 512, 44))
    # class 4: 1, 2 and about 100 lanes of 128 bytes per restart segment
    L.append(lockstep("heads_grey_ri2", "grey", 400, 51, ri=2, cls=4))
    L.append(lockstep("heads_grey_ri4", "grey", 400, 52, ri=4, cls=4))
    L.append(lockstep("heads_grey_ri200", "grey", 400, 53, ri=200, cls=4))
    L.append(lockstep("heads_444_ri1", "444", 134, 54, ri=1, cls=4))
    L.append(lockstep("heads_444_ri67", "444", 134, 55, ri=67, cls=4))
    L.append(lockstep("heads_420_ri1_std", "420", 68, 56, ri=1, std=True, cls=4))
    L.append(lockstep("heads_420_ri34_std", "420", 68, 57, ri=34, std=True, cls=4))
    L.append(phase_only("heads_phase_444_ri6", "444", 320, 240, 58, ri=6, cls=4))
    L.append(phase_only("heads_phase_444_ri500", "444", 320, 240, 59, ri=500, cls=4))
    L.append(phase_only("heads_phase_420_ri250_std", "420", 512, 384, 60, ri=250, std=True, cls=4))
    # class 5
    L.append(chains("err_first_wave", *X5, 36, edit=_err_first_wave, cls=5))
    L.append(chains("err_behind_flag", *X5, 36, edit=_err_behind_flag, cls=5))
    L.append(chains("cut_middle", *X5, 36, edit=_cut_middle, cls=5))
    out = {s.name: s for s in L}
    assert len(out) == len(L)
    return out


AT_1024 = ("lock_grey_17", "lock_grey_1024", "lock_grey_1040", "lock_grey_1041", "lock_grey_1170", "lock_420_22", "lock_420_130",
           "lock_420_176", "chain_1024_66", "chain_x5", "phase_420_big", "phase_444", "heads_grey_ri200", "heads_420_ri34_std",
           "heads_phase_444_ri500", "err_behind_flag", "cut_middle")


def members(S):
    """The streams decoded with lanes of S bytes: all of them at 128 (the streams for 1024 alone left out), a selection at 1024."""
    ss = streams()
    if S == 128:
        return [s for n, s in ss.items() if n not in ("lock_grey_17", "lock_grey_1024", "lock_grey_1041", "chain_1024_66")]
    assert S == 1024
    return [ss[n] for n in AT_1024]


# ---- a model of the state-only pass ---------------------------------------------------------------------------------------------------
class Model:
    """The state a decoder carries between symbols -- p (bit position), c (the unit's place in the MCU), z (0: a DC symbol is
    expected, else the next zigzag slot) -- advanced by the reference's rules: a DC symbol takes its code and `size` value bits and
    opens the unit at slot 1; an AC symbol takes its code and value bits and moves run + 1 slots; an EOB, or reaching slot 64, ends the
    unit.  What the reference calls an error cannot stop a decoder that is only guessing: a run past slot 63 ends the unit, a size out
    of range has no value bits, bits that are no code are skipped as 16 bits and one slot (the conventions of tools/sync_sim.c).
    All components of these streams share their tables, so c only counts."""

    def __init__(self, stream):
        fr = stream.fr
        assert len({(c.td, c.ta) for c in fr.comps}) == 1
        self.ecs = _scan_of(stream.data)
        self.nbits = 8 * len(self.ecs)
        self.dus = len(fr.unit_comps())
        self.dc, self.ac = self._lut(fr.dc[fr.comps[0].td]), self._lut(fr.ac[fr.comps[0].ta])
        self.stream = stream
        self._dist_at = None

    @staticmethod
    def _lut(t):
        """{(length, code): symbol} and the lengths in use."""
        return t.codes, sorted({ln for ln, _ in t.codes})

    def _peek16(self, p):
        b = p >> 3
        v = int.from_bytes(self.ecs[b:b + 3].ljust(3, b"\0"), "big")
        return (v >> (8 - (p & 7))) & 0xFFFF

    def step(self, p, c, z):
        codes, lens = self.dc if z == 0 else self.ac
        w = self._peek16(p)
        for ln in lens:
            sym = codes.get((ln, w >> (16 - ln)))
            if sym is not None:
                break
        else:
            z += 1
            return (p + 16, (c + 1) % self.dus, 0) if z > 63 else (p + 16, c, z)
        if z == 0:
            return p + ln + (sym if sym <= 11 else 0), c, 1
        if sym == 0:
            return p + ln, (c + 1) % self.dus, 0
        size = sym & 15
        p += ln + (size if size <= 10 else 0)
        z += (sym >> 4) + 1
        return (p, (c + 1) % self.dus, 0) if z > 63 else (p, c, z)

    def truth(self, b0, b1):
        """{bit position: (c, z)} of the true decode of the segment [b0, b1) bytes."""
        out, (p, c, z) = {}, (8 * b0, 0, 0)
        while p < 8 * b1:
            out[p] = (c, z)
            p, c, z = self.step(p, c, z)
        return out

    def run(self, p, c, z, end_bit):
        """The state after the first symbol that ends at or behind end_bit."""
        while p < end_bit:
            p, c, z = self.step(p, c, z)
        return p, c, z

    def sync_distance(self, p0, truth, end_bit, phase=True):
        """Bits from p0 until a decoder started there at "DC expected, unit 0" is in the true state (the slot alone with
        phase=False); None if it never is before end_bit."""
        p, c, z = p0, 0, 0
        while p < end_bit:
            t = truth.get(p)
            if t is not None and t[1] == z and (t[0] == c or not phase):
                return p - p0
            p, c, z = self.step(p, c, z)
        return None

    def lockstep_distances(self, S):
        """For streams whose symbols are all 8 bits: sync_distance in BYTES for every lane start at once, by one backward pass over
        the bytes (dist[state] at byte q = 0 for the true state, else 1 + dist[next state] at q + 1).  -> [(start, head, distance or
        None)] per lane."""
        assert S % 128 == 0
        dist_at = self._dist_at or self._all_lockstep_distances()
        return [(q, head, dist_at[q]) for q, head in self.stream.lane_starts(S)]

    def _all_lockstep_distances(self):
        """{byte: distance or None} for every 128th byte of every restart segment."""
        dus = self.dus
        nst = dus * 64
        st = np.arange(nst)
        c, z = st // 64, st % 64
        nxt = {}
        for b in set(self.ecs):                                  # the transition of every byte value on every state
            t = np.empty(nst, np.int64)
            assert self._byte_step(b, 0)[0] == 8 and self._byte_step(b, 1)[0] == 8, "not a lockstep stream"
            sym_ac = self._byte_step(b, 1)[1]
            zn = np.where(z == 0, 1, 64 if sym_ac is None else z + sym_ac)
            done = zn > 63
            t[:] = np.where(done, ((c + 1) % dus) * 64, c * 64 + zn)
            nxt[b] = t
        INF = np.int64(1) << 40
        dist_at = {}
        for b0, b1 in reversed(self.stream.segments()):
            tr = self.truth(b0, b1)
            dist = np.full(nst, INF)
            for q in range(b1 - 1, b0 - 1, -1):
                dist = np.minimum(dist[nxt[self.ecs[q]]] + 1, INF)
                tc, tz = tr[8 * q]
                dist[tc * 64 + tz] = 0
                if (q - b0) % 128 == 0:
                    dist_at[q] = int(dist[0])                    # "DC expected, unit 0"
        self._dist_at = {q: (None if d >= INF else d) for q, d in dist_at.items()}
        return self._dist_at

    def _byte_step(self, b, z):
        """(bits taken, slots an AC symbol moves or None for an EOB) of byte b read as one symbol in state z (0 or 1)."""
        codes, lens = self.dc if z == 0 else self.ac
        w = b << 8
        for ln in lens:
            sym = codes.get((ln, w >> (16 - ln)))
            if sym is not None:
                break
        else:
            raise AssertionError("a byte that is no symbol")
        if z == 0:
            return ln + sym, None
        if sym == 0:
            return ln, None
        return ln + (sym & 15), (sym >> 4) + 1


def rounds_needed(lanes, nbytes_end):
    """From [(start, head, sync distance or None)] per lane (all in bytes, or all in bits): R[j] = how many lanes back the nearest lane lies whose own
    speculative decode is true by the END of lane j (0: lane j's own, or a segment head) -- the rounds lane j's exit needs, one lane
    per round."""
    R = []
    for j in range(len(lanes)):
        end = lanes[j + 1][0] if j + 1 < len(lanes) else nbytes_end      # a segment's last lane ends where the next segment starts
        r, i = None, j
        while True:
            qi, hi, di = lanes[i]
            if hi or (di is not None and qi + di <= end):
                r = j - i
                break
            i -= 1
        R.append(r)
    return R


def chain_and_cross(R):
    """(longest chain, most wave boundaries a chain crosses) of the rounds per lane."""
    chain, cross = max(R), 0
    for j, r in enumerate(R):
        if r:
            cross = max(cross, j // WAVE - (j - r) // WAVE)
    return chain, cross


@functools.lru_cache(maxsize=1)
def fallback_variants():
    """Five more pictures like chain_x5 (a chain across five or six wave boundaries, other lanes and seeds), for batches that need
    several pictures the parallel decoder gives up on.  No synchroniser lies in a wave's last lane: the speculative exit of that
    lane, the first thing the next wave bridges from, would be true, and the chain one generation shorter."""
    return [chains(f"chain_x5_v{k}", 128, n, sync, 70 + k) for k, (n, sync) in
            enumerate([(330, (30, 327)), (392, (10, 389)), (340, (60, 330)), (400, (64, 396)), (336, (1, 334))])]
