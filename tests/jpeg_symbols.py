"""A symbol-level baseline JPEG writer (test helper; pure Python + numpy, no encoder library).

Encoders only write the symbols an encoder needs.  The reference's data-unit decoder (src/jpeg_scanner.cpp:467-520) accepts more,
and so must the GPU decoder: size-0 run symbols, runs that end on or past slot 63, units without an EOB, DC differences of 11 bits,
a DC predictor that wraps int16, tables of any shape (16-bit codes, 0xFF or out-of-range sizes as symbols, incomplete codes), and
every one of its error classes.  Here a stream is written from TOKENS, one list per data unit in decode order:

    DC(size, bits)          a DC symbol `size` and its `size` value bits (size 12..15 or 0xFF: the symbol's code alone)
    AC(run, size, bits)     the AC symbol (run << 4) | size and its value bits (size 11..15: the code alone)
    EOB                     symbol 0x00
    RAW(bitstring)          literal bits where a symbol is expected: a code no table assigns (checked when the stream is built)
    END                     the stream ends here (at a unit boundary); what is left of the byte is padded with 1-bits
    CUT(token, where)       `token` cut at a byte boundary inside its code (where="code") or its value bits ("bits"); the stream ends

write() returns the file and its INTENT: what a decoder that follows the reference must make of it -- the status class and first
erring unit (PJD_ST_* values of include/pjd.h), and per data unit its zigzag-slot values, the slots it visited and its absolute DC
after the reference's int16 predictor (reset at every restart).  The intent comes from the tokens alone, not from decoding the bits.
"""
import numpy as np

OK, DC_SYM, DC_LEN, DC_BITS, AC_SYM, AC_RUN, AC_LEN, AC_BITS = range(8)
STATUS_NAMES = ["OK", "DC_SYM", "DC_LEN", "DC_BITS", "AC_SYM", "AC_RUN", "AC_LEN", "AC_BITS"]

EOB = ("EOB",)
END = ("END",)


def DC(size, bits=0):
    return ("DC", size, bits)


def AC(run, size, bits=0):
    return ("AC", run, size, bits)


def RAW(bitstring):
    return ("RAW", bitstring)


def CUT(token, where):
    return ("CUT", token, where)


def value_bits(v):
    """(size, bits) of a coefficient value, as T.81 F.1.2.1 codes it."""
    if v == 0:
        return 0, 0
    size = int(abs(v)).bit_length()
    return size, (v if v > 0 else v + (1 << size) - 1)


def dcv(diff):
    return DC(*value_bits(diff))


def acv(run, v):
    return AC(run, *value_bits(v))


def extend(size, bits):
    """The reference's sign extension (jpeg_scanner.cpp:480,510); size 0 stores a literal 0."""
    if size == 0:
        return 0
    return bits - ((1 << size) - 1) if bits < (1 << (size - 1)) else bits


def wrap16(x):
    return ((int(x) + 32768) & 0xFFFF) - 32768


class Table:
    """A DHT table as written: 16 counts and the symbols in code order (duplicates, 0xFF, anything -- up to 162).

    `oversubscribed=True` admits counts whose codes run out of their length, as the reference's generate_codes does (it keeps
    counting): a code that no longer fits its length never matches (get_next_symbol compares whole codes), so its symbol cannot be
    written, and the table is no prefix code the planner accepts."""

    def __init__(self, counts, symbols, oversubscribed=False):
        counts, symbols = list(counts), list(symbols)
        assert len(counts) == 16 and sum(counts) == len(symbols) <= 162
        self.counts, self.symbols = counts, symbols
        self.oversubscribed = False
        self.code_of = {}                  # symbol -> (length, code) of its FIRST occurrence
        self.codes = {}                    # (length, code) -> symbol
        code, q = 0, 0
        for ln in range(1, 17):
            for _ in range(counts[ln - 1]):
                if code >= (1 << ln):
                    assert oversubscribed, "over-subscribed table"
                    self.oversubscribed = True
                    code += 1
                    q += 1
                    continue                   # a code that does not fit its length: the symbol cannot be written
                self.codes.setdefault((ln, code), symbols[q])
                self.code_of.setdefault(symbols[q], (ln, code))
                code += 1
                q += 1
            code <<= 1

    def code_bits(self, sym):
        assert sym in self.code_of, f"symbol {sym:#x} is not in the table"
        ln, code = self.code_of[sym]
        return format(code, f"0{ln}b")

    def matches(self, bits):
        """Symbol of the code that `bits` (a str) starts with, or None (the reference's 16-bit search)."""
        for ln in range(1, min(16, len(bits)) + 1):
            s = self.codes.get((ln, int(bits[:ln], 2)))
            if s is not None:
                return s
        return None

    def segment(self, tc, th):
        return bytes([(tc << 4) | th]) + bytes(self.counts) + bytes(self.symbols)


def table_from_lengths(symbols_by_length):
    """{length: [symbols]} -> Table."""
    counts = [len(symbols_by_length.get(ln, [])) for ln in range(1, 17)]
    return Table(counts, [s for ln in range(1, 17) for s in symbols_by_length.get(ln, [])])


class Component:
    def __init__(self, h=1, v=1, tq=0, td=0, ta=0):
        self.h, self.v, self.tq, self.td, self.ta = h, v, tq, td, ta


class Frame:
    """width x height, components (luma first; only luma may be sampled 2x, as the reference requires), tables by id."""

    def __init__(self, width, height, comps, dc, ac, qt=None, qt16=(), ri=0, standard_restart=False, standard_zigzag=False):
        self.width, self.height, self.comps = width, height, comps
        self.dc, self.ac = dc, ac                                # {id: Table}
        self.qt = qt if qt is not None else {c.tq: list(range(1, 65)) for c in comps}     # {id: 64 values in zigzag order}
        self.qt16 = set(qt16)
        self.ri, self.standard_restart = ri, standard_restart
        self.standard_zigzag = standard_zigzag                   # decoded with ITU T.81's map (PJD_F_STANDARD_ZIGZAG): not in the file
        self.hs, self.vs = comps[0].h, comps[0].v
        self.bw, self.bh = (width + 7) // 8, (height + 7) // 8                             # 8x8 blocks (the reference's mcu_w / mcu_h)
        self.bw_real = self.bw + (self.hs == 2 and self.bw % 2 == 1)
        self.bh_real = self.bh + (self.vs == 2 and self.bh % 2 == 1)

    def mcus(self):
        """(y, x) of every MCU in decode order, in 8x8-block units (jpeg_scanner.cpp:725-727)."""
        return [(y, x) for y in range(0, self.bh, self.vs) for x in range(0, self.bw, self.hs)]

    def unit_comps(self):
        """Component of each data unit of one MCU, in decode order."""
        return [j for j, c in enumerate(self.comps) for _ in range(c.v * c.h)]

    def n_units(self):
        return len(self.mcus()) * len(self.unit_comps())

    def sampling(self):
        return {(1, 1, 1): "grey", (1, 1, 3): "444", (2, 1, 3): "422", (2, 2, 3): "420", (1, 2, 3): "440"}[(self.hs, self.vs, len(self.comps))]

    def zigzag(self):
        """Zigzag slot -> natural index of the map the frame is decoded with."""
        return K_ZZ_T81 if self.standard_zigzag else K_ZZ

    def quantiser(self, tq):
        """Quantiser of each natural position, as the reference fills it from the DQT entries through the zigzag map (the later
        entry wins at natural 38; natural 58 keeps 0 under the reference's map)."""
        q = [0] * 64
        for k, v in enumerate(self.qt[tq]):
            q[self.zigzag()[k]] = v
        return q

    def restarts_before(self):
        """MCU indices (in decode order) before which a restart happens: the reference's (y * Wr + x) % RI == 0 rule
        (jpeg_scanner.cpp:729), or ITU T.81's every-RI-th MCU."""
        if not self.ri:
            return set()
        if self.standard_restart:
            return {m for m in range(len(self.mcus())) if m % self.ri == 0 and m}
        return {m for m, (y, x) in enumerate(self.mcus()) if (y * self.bw_real + x) % self.ri == 0 and m}


class Intent:
    def __init__(self, n_units):
        self.status, self.err_unit = OK, -1
        self.slots = np.zeros((n_units, 64), np.int32)           # value per zigzag slot (slot 0: the absolute DC)
        self.visited = np.zeros((n_units, 64), bool)             # slots the unit wrote (an explicit 0 included)
        self.n_decoded = 0                                        # units decoded completely
        self.unit_bit = []                                        # where each written unit starts in the destuffed, marker-free scan
        self.forms = set()                                        # which forms the stream holds (coverage bookkeeping)


class _Bits:
    def __init__(self):
        self.s = []
        self.n = 0

    def put(self, bits):
        self.s.append(bits)
        self.n += len(bits)

    def pad(self):
        if self.n % 8:
            self.put("1" * (8 - self.n % 8))

    def take(self):
        out = "".join(self.s)
        self.s, self.n = [], 0
        return out


def _stuffed(bits):
    assert len(bits) % 8 == 0
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return raw.replace(b"\xff", b"\xff\x00")


def _seg(marker, body):
    return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body


def write(frame, units, eoi=True):
    """-> (JPEG bytes, Intent).  `units`: one token list per data unit in decode order (fewer than the frame has only with END / CUT)."""
    f = frame
    out = bytearray(b"\xff\xd8")
    for tq in sorted(f.qt):
        p16 = tq in f.qt16
        body = bytes([(0x10 if p16 else 0) | tq]) + b"".join(v.to_bytes(2 if p16 else 1, "big") for v in f.qt[tq])
        out += _seg(0xDB, body)
    body = bytes([8, f.height >> 8, f.height & 255, f.width >> 8, f.width & 255, len(f.comps)])
    for j, c in enumerate(f.comps):
        body += bytes([j + 1, (c.h << 4) | c.v, c.tq])
    out += _seg(0xC0, body)
    dht = b"".join(t.segment(0, i) for i, t in sorted(f.dc.items())) + b"".join(t.segment(1, i) for i, t in sorted(f.ac.items()))
    out += _seg(0xC4, dht)
    if f.ri:
        out += _seg(0xDD, bytes([f.ri >> 8, f.ri & 255]))
    body = bytes([len(f.comps)]) + b"".join(bytes([j + 1, (c.td << 4) | c.ta]) for j, c in enumerate(f.comps)) + bytes([0, 63, 0])
    out += _seg(0xDA, body)

    ucomp = f.unit_comps()
    per_mcu = len(ucomp)
    n_units = f.n_units()
    rst = f.restarts_before()
    it = Intent(n_units)
    bits = _Bits()
    segs = []                            # bit strings of the finished restart segments (padded to bytes)
    checks = []                          # (bit position in the destuffed scan, table) where a RAW / END / cut code must decode to nothing
    pred = [0] * len(f.comps)
    ended = False

    def fail(cls, u):
        if it.status == OK:
            it.status, it.err_unit = cls, u

    def here():
        return sum(len(s) for s in segs) + bits.n

    for u, toks in enumerate(units):
        assert u < n_units, "more units than the frame has"
        m, j = divmod(u, per_mcu)
        c = ucomp[j]
        dct, act = f.dc[f.comps[c].td], f.ac[f.comps[c].ta]
        if j == 0 and m in rst:
            bits.pad()
            segs.append(bits.take())
            if it.status == OK:
                pred = [0] * len(f.comps)
        it.unit_bit.append(here())
        live = it.status == OK                        # tokens after the first error are written, and decode to nothing
        slot = 0
        for t in toks:
            kind = t[0]
            want_dc = slot == 0
            assert slot < 64, f"unit {u}: a token after slot 63"
            table = dct if want_dc else act
            if kind == "END":
                assert want_dc, "END goes between units"
                if live:
                    checks.append((here(), dct))
                    fail(DC_SYM, u)                   # the data runs out where the unit's DC symbol should start
                    it.forms.add("end_at_unit_boundary")
                ended = True
                break
            if kind == "RAW":
                if live:
                    checks.append((here(), table))
                    fail(DC_SYM if want_dc else AC_SYM, u)
                    it.forms.add("raw_dc" if want_dc else "raw_ac")
                    live = False
                bits.put(t[1])
                continue
            if kind == "CUT":
                inner, where = t[1], t[2]
                tb, ncode = _token_bits(inner, table)
                pos = here()
                # the cut falls on a byte boundary (no padding to misread) inside the code, or inside / just before the value bits
                if where == "code":
                    b = (pos + ncode - 1) // 8 * 8
                    if b < pos:
                        raise ValueError("no byte boundary inside the code")
                else:
                    b = (pos + ncode + 7) // 8 * 8
                    if b >= pos + len(tb):
                        raise ValueError("no byte boundary inside the value bits")
                bits.put(tb[:b - pos])
                if live:
                    if where == "code":
                        checks.append((pos, table))
                        fail(DC_SYM if want_dc else AC_SYM, u)
                        it.forms.add("cut_in_code")
                    elif want_dc:
                        assert 0 < inner[1] <= 11
                        fail(DC_BITS, u)
                        it.forms.add("cut_in_dc_bits")
                    else:
                        assert slot + inner[1] < 64 and 0 < inner[2] <= 10
                        fail(AC_BITS, u)
                        it.forms.add("cut_in_ac_bits")
                ended = True
                break
            if kind == "DC":
                assert want_dc, f"unit {u}: a DC token after the unit's DC"
                size, b = t[1], t[2]
                bits.put(_token_bits(t, dct)[0])
                slot = 1
                if not live:
                    continue
                if size == 0xFF:
                    fail(DC_SYM, u); live = False; it.forms.add("dc_sym_ff"); continue
                if size > 11:
                    fail(DC_LEN, u); live = False; it.forms.add(f"dc_size_{size}"); continue
                it.forms.add(f"dc_size_{size}")
                if size == 11:
                    it.forms.add("dc11_bits_zero" if b == 0 else "dc11_bits_ones" if b == (1 << 11) - 1 else "dc11")
                raw = extend(size, b) + pred[c]
                dc_wrapped = raw > 32767 or raw < -32768
                if raw > 32767:
                    it.forms.add("dc_wrap_up")
                if raw < -32768:
                    it.forms.add("dc_wrap_down")
                pred[c] = wrap16(raw)
                it.slots[u, 0] = pred[c]
                it.visited[u, 0] = True
                continue
            assert not want_dc, f"unit {u}: the unit starts with {kind}, not DC"
            if kind == "EOB":
                bits.put(act.code_bits(0x00))
                slot = 64
                if live:
                    it.forms.add("eob")
                continue
            run, size, b = t[1], t[2], t[3]
            sym = (run << 4) | size
            assert sym != 0, "AC(0, 0) is the EOB"
            bits.put(_token_bits(t, act)[0])
            if not live:
                slot = min(64, slot + run + 1)
                continue
            if sym == 0xFF:
                fail(AC_SYM, u); live = False; it.forms.add("ac_sym_ff"); continue
            if slot + run >= 64:
                fail(AC_RUN, u); live = False
                it.forms.add("ac_run_to_64" if slot + run == 64 else "ac_run_past_64")
                continue
            slot += run
            if size > 10:
                fail(AC_LEN, u); live = False; it.forms.add(f"ac_size_{size}"); continue
            v = extend(size, b)
            after48 = bool(it.visited[u, 48] and it.slots[u, 48])
            it.slots[u, slot] = v
            it.visited[u, slot] = True
            if size == 0:
                it.forms.add(f"ac_size0_run_{run}")
                if slot == 52:
                    it.forms.add("explicit_zero_slot52_after_48" if after48 else "explicit_zero_slot52")
            elif size == 10:
                it.forms.add(f"ac10_{v}" if abs(v) in (512, 1023) else "ac10")
            if slot == 52 and size and after48:
                it.forms.add("nonzero_slot52_after_48")
            if slot == 63:
                it.forms.add("lands_on_63")
            slot += 1
        if ended:
            break
        if live:
            assert slot == 64, f"unit {u}: the tokens end at slot {slot} without an EOB"
            if toks[-1] != EOB:
                it.forms.add("no_eob")
            it.n_decoded += 1
            it.forms |= _edge_forms(f, it, u, c, m, dc_wrapped, rst)
    if not ended:
        assert len(units) == n_units, "fewer units than the frame has: end the stream with END or CUT"
    bits.pad()
    segs.append(bits.take())

    scan = "".join(segs)                      # what the reference's bit reader sees: restart markers stripped, padding kept
    for pos, table in checks:                 # the bits there run into no code before the data ends (the reference reads <= 16 bits)
        assert table.matches(scan[pos:pos + 16]) is None, "the bits at a RAW / END / cut decode to a symbol"

    for k, sb in enumerate(segs):
        if k:
            out += bytes([0xFF, 0xD0 + (k - 1) % 8])
        out += _stuffed(sb)
    if eoi:
        out += b"\xff\xd9"
    if len(segs) > 1:
        it.forms.add("restart")
    if eoi and scan.count("1") > 0.8 * len(scan) and len(scan) >= 64:
        it.forms.add("mostly_ones")
    return bytes(out), it


INT16_EDGES = {-32768: "min", 32767: "max", -32767: "minp1"}
COMP_NAMES = ["y", "cb", "cr"]


def _edge_forms(f, it, u, c, m, dc_wrapped, rst):
    """Forms of a decoded unit at the int16 edges: its absolute DC at -32768 / 32767 / -32767 (for -32768 also where and how it got
    there), and natural positions whose dequantised value (int16)(coef * q) is one of those three."""
    out = set()
    dc = int(it.slots[u, 0])
    if dc in INT16_EDGES:
        out.add({"min": "dc_abs_min", "max": "dc_abs_max", "minp1": "dc_abs_min_plus1"}[INT16_EDGES[dc]])
    if dc == -32768:
        q = f.qt[f.comps[c].tq][0]
        out |= {f"dc_abs_min_{COMP_NAMES[c]}", f"dc_abs_min_{f.sampling()}", "dc_abs_min_by_wrap" if dc_wrapped else "dc_abs_min_by_descent",
                f"dc_abs_min_q{q}_{16 if f.comps[c].tq in f.qt16 else 8}bit", f"dc_abs_min_q_{'odd' if q % 2 else 'even'}"}
        if u == f.n_units() - 1:
            out.add("dc_abs_min_last_unit")
        if any(r <= m for r in rst):
            out.add("dc_abs_min_after_restart")
        if it.visited[u, 52]:
            out.add("dc_abs_min_value52" if it.slots[u, 52] else "dc_abs_min_zero52")
    zz, q = f.zigzag(), f.quantiser(f.comps[c].tq)
    src = {}
    for k in np.flatnonzero(it.visited[u]):          # slot order: the later slot wins a shared natural position
        src[zz[k]] = k
    for n, k in src.items():
        v = int(it.slots[u, k])
        p = wrap16(v * q[n])
        if v and p in INT16_EDGES:
            out.add(f"deq_{INT16_EDGES[p]}_nat{n}" + (f"_slot{k}" if n == 38 else ""))
    return out


def _token_bits(t, table):
    """-> (bit string, code length) of a DC / AC / EOB token (no value bits for an out-of-range size or symbol 0xFF)."""
    if t[0] == "EOB":
        c = table.code_bits(0)
        return c, len(c)
    if t[0] == "DC":
        size, b = t[1], t[2]
        c = table.code_bits(size)
        vb = format(b, f"0{size}b") if 0 < size <= 11 else ""
        return c + vb, len(c)
    run, size, b = t[1], t[2], t[3]
    c = table.code_bits((run << 4) | size)
    vb = format(b, f"0{size}b") if 0 < size <= 10 and ((run << 4) | size) != 0xFF else ""
    return c + vb, len(c)


# ---- the reference's layout ------------------------------------------------------------------------------------------------------
# zigzag slot -> natural index, with the reference's entry 48 = 38 (src/headers/common.h:9-18)
K_ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 38, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
K_ZZ_T81 = K_ZZ[:48] + [58] + K_ZZ[49:]          # ITU T.81 (PJD_F_STANDARD_ZIGZAG): slot 48 -> natural 58


def unit_offsets(frame):
    """Offset in the reference's MCU_buffer (n_dpus x 19200 int16) of every data unit, in decode order (jpeg_scanner.cpp:725-737)."""
    f = frame
    W = f.bw_real
    offs = []
    for (y, x) in f.mcus():
        for j, c in enumerate(f.comps):
            for v in range(c.v):
                for h in range(c.h):
                    m = (y + v) * W + (x + h)
                    blk = (m // (W * 2)) * ((W + 1) // 2) + (m % W) // 2
                    pos = ((m // W) % 2) * 2 + (m % W) % 2
                    offs.append((blk // 25) * 19200 + (blk % 25) * 768 + j * 256 + pos * 64)
    return offs


def n_dpus(frame):
    pw, ph = (frame.bw_real + 1) // 2 * 2, (frame.bh_real + 1) // 2 * 2
    return (pw * ph + 99) // 100


def intent_buffer(frame, intent):
    """The intent in the reference's MCU_buffer layout: each unit's visited slots written in slot order (so an explicit 0 at slot 52
    overwrites natural 38 after slot 48 did), through the frame's zigzag map."""
    buf = np.zeros(n_dpus(frame) * 19200, np.int16)
    zz = frame.zigzag()
    for u, off in enumerate(unit_offsets(frame)):
        for k in np.flatnonzero(intent.visited[u]):
            buf[off + zz[k]] = intent.slots[u, k]
    return buf.reshape(-1, 19200)
