"""Progressive (SOF2) files for tests (pure Python + numpy), beside the baseline writer of tests/jpeg_symbols.py: a small writer kept for
the int16-edge test (write, edge_streams), the full writer (build: all four procedures from target coefficients and a scan script, see
below) and a bit-level model of ITU T.81 G.1.2 (decode, at the end).

The small writer puts one DHT before each scan and SOS with Ss / Se / Ah / Al, from given values:

    DCFirst(comps, al, values)       DC first scan over `comps` (interleaved when several), values[c][b] = the DC of block b before the
                                     point transform (coded as differences of 11 bits at most)
    DCRefine(comps, al, bits)        DC refinement scan: bits[c][b] in {0, 1}
    ACFirst(comp, ss, se, al, vals)  AC first scan over one component: vals[b] = {slot: value (|value| <= 1023)}; one EOB per block
                                     unless its last value sits on se

Only 4:4:4 and grey frames whose sizes are multiples of 8, without restart intervals: every grid is then the MCU grid, and block b of
component c is data unit b * ncomp + c.  The model is ITU T.81 G.1.2 as pjd_k_progressive stores it: coefficients accumulate in
zigzag-slot order, each store truncated to int16 -- (int16)(dc << Al), (int16)(dc | 1 << Al), (int16)(v << Al).
"""
from collections import namedtuple

import numpy as np

from jpeg_symbols import (AC_BITS, AC_LEN, AC_RUN, AC_SYM, DC_BITS, DC_LEN, DC_SYM, K_ZZ, OK, Intent, Table, _Bits, _seg, _stuffed, extend, value_bits,
                          wrap16)

DCFirst = namedtuple("DCFirst", "comps al values")
DCRefine = namedtuple("DCRefine", "comps al bits")
ACFirst = namedtuple("ACFirst", "comp ss se al vals")


def write(frame, scans, dc_table, ac_table):
    """-> (JPEG bytes, Intent with every slot of every unit visited: the model's coefficients)."""
    f = frame
    assert f.width % 8 == 0 and f.height % 8 == 0 and not f.ri and (f.hs, f.vs) == (1, 1)
    nc, nb = len(f.comps), (f.width // 8) * (f.height // 8)
    out = bytearray(b"\xff\xd8")
    for tq in sorted(f.qt):
        p16 = tq in f.qt16
        out += _seg(0xDB, bytes([(0x10 if p16 else 0) | tq]) + b"".join(v.to_bytes(2 if p16 else 1, "big") for v in f.qt[tq]))
    body = bytes([8, f.height >> 8, f.height & 255, f.width >> 8, f.width & 255, nc])
    for j, c in enumerate(f.comps):
        body += bytes([j + 1, 0x11, c.tq])
    out += _seg(0xC2, body)
    it = Intent(nb * nc)
    it.visited[:] = True
    slots = it.slots                                     # unit b * nc + c
    for sc in scans:
        bits = _Bits()
        if isinstance(sc, ACFirst):
            out += _seg(0xC4, ac_table.segment(1, 0))
            out += _seg(0xDA, bytes([1, sc.comp + 1, 0x00, sc.ss, sc.se, sc.al]))
            for b in range(nb):
                last = sc.ss - 1
                for z in sorted(sc.vals[b]):
                    v = sc.vals[b][z]
                    assert sc.ss <= z <= sc.se and v and abs(v) <= 1023
                    run = z - last - 1
                    while run > 15:
                        bits.put(ac_table.code_bits(0xF0))
                        run -= 16
                    size, vb = value_bits(v)
                    bits.put(ac_table.code_bits((run << 4) | size) + format(vb, f"0{size}b"))
                    slots[b * nc + sc.comp, z] = wrap16(v << sc.al)
                    last = z
                if last < sc.se:
                    bits.put(ac_table.code_bits(0x00))
        else:
            refine = isinstance(sc, DCRefine)
            if not refine:
                out += _seg(0xC4, dc_table.segment(0, 0))
            out += _seg(0xDA, bytes([len(sc.comps)]) + b"".join(bytes([c + 1, 0x00]) for c in sc.comps)
                        + bytes([0, 0, ((sc.al + 1) << 4 if refine else 0) | sc.al]))
            pred = {c: 0 for c in sc.comps}
            for b in range(nb):
                for c in sc.comps:
                    u = b * nc + c
                    if refine:
                        bits.put(str(sc.bits[c][b]))
                        slots[u, 0] = wrap16(int(slots[u, 0]) | (sc.bits[c][b] << sc.al))
                        continue
                    v = sc.values[c][b]
                    size, vb = value_bits(v - pred[c])
                    assert size <= 11
                    bits.put(dc_table.code_bits(size) + (format(vb, f"0{size}b") if size else ""))
                    pred[c] = v
                    slots[u, 0] = wrap16(v << sc.al)
        bits.pad()
        out += _stuffed(bits.take())
    return bytes(out + b"\xff\xd9"), it


def ramp(targets, n):
    """n DC values (before the point transform) that reach each (block, value) of `targets` in steps of 2047 at most."""
    vals, prev, pb = [0] * n, 0, -1
    for b, t in sorted(targets):
        steps = b - pb
        for k in range(1, steps + 1):
            vals[pb + k] = prev + (t - prev) * k // steps
            assert abs(vals[pb + k] - (vals[pb + k - 1] if pb + k else 0)) <= 2047
        prev, pb = t, b
    for k in range(pb + 1, n):
        vals[k] = prev
    return vals


def edge_streams(frame_of):
    """[(label, frame, scans)] of progressive frames whose stores truncate to -32768: `pred << Al` at Al = 3 (+-4096) in a DC first
    scan, then a DC refinement scan over it; AC first scans at Al = 13 with v = +-4 at slot 52 and at other slots (1, 5, 48, 60, 63);
    a grey frame and an interleaved 4:4:4 one.  frame_of(sub, w, h) -> a Frame."""
    out = []
    for sub, (w, h) in [("grey", (32, 16)), ("444", (32, 16))]:
        fr = frame_of(sub, w, h)
        nc, nb = len(fr.comps), (w // 8) * (h // 8)
        comps = list(range(nc))
        edge = lambda c: 4096 if c % 2 else -4096                # << 3: 32768 and -32768, both stored as -32768
        dc = {c: ramp([(2, edge(c)), (3, edge(c)), (nb - 1, 100 + c)], nb) for c in comps}
        scans = [DCFirst(comps, 3, dc), DCRefine(comps, 2, {c: [(b + c + 1) % 2 for b in range(nb)] for c in comps})]
        for c in comps:
            band1 = [{1: [4, -4, 3][b % 3], 5: -4} if b % 2 else {2: 1, 5: 4} for b in range(nb)]
            band2 = [{48: 4, 52: [4, -4][b % 2], 63: -4} if b % 3 else {52: 1, 60: -4} for b in range(nb)]
            scans += [ACFirst(c, 1, 5, 13, band1), ACFirst(c, 6, 63, 13, band2)]
        out.append((f"prog_edge_{sub}_{w}x{h}", fr, scans))
    return out


# ---- the full writer: target coefficients + a scan script -> a SOF2 file with all four procedures -----------------------------------
#
#   S(comps, ss, se, ah, al, ...)   one scan: DC first / DC refinement over `comps` (interleaved when several), AC first / AC refinement
#                                   over one component and the band ss..se
#   build(frame, target, script)    -> Written: the file, what each scan holds, a log of every token, and the INTENT
#
# `target` is (n_units, 64): the final coefficients per data unit (interleaved order, as the baseline writer counts units) and zigzag
# slot.  The intent needs no decode logic: after the scans written, slot z of a unit holds wrap16((dc >> Al) << Al) (DC) or
# sign(v) * ((|v| >> Al) << Al) (AC) at the lowest Al a scan has reached for that slot, and 0 where no scan has been.  A
# non-interleaved scan runs over the component's own block grid (T.81 A.2.3): luma units that only the MCU padding creates are
# reached by interleaved scans alone.  The scanner and the reference take at most 162 symbols per Huffman table; so does build().

_ScanT = namedtuple("Scan", "comps ss se ah al ri eob tid shape eob_overrun")
Damage = namedtuple("Damage", "scan block kind arg")      # kind "raw": 16 one-bits where the block's first symbol is expected;
#                                                           "sym": the symbol `arg` (its code alone) there


def S(comps, ss=0, se=0, ah=0, al=0, ri=None, eob="max", tid=0, shape="flat", eob_overrun=0):
    """ri: restart interval in MCUs of this scan (None: what the previous scan had; a DRI is written when it changes).
    eob: "single" (one EOB per block) | "max" (runs as long as they get, flushed at 32767) | ("random", seed) | ("lengths", [n, ...]:
    a run is flushed when it reaches the next length of the cycle).  tid: table id, or one per component of the scan.
    shape: "flat" | "skew" | "long" (every code 12 bits) -- the shape of the DHT built from the symbols the scan uses.
    eob_overrun: a run still open at a restart is written as that many blocks longer than it is -- no encoder does that; a decoder drops
    what is left of a run at the restart (T.81 G.1.2.2: EOBRUN belongs to the restart interval), so the coefficients are the same."""
    comps = (comps,) if isinstance(comps, int) else tuple(comps)
    tid = (tid,) * len(comps) if isinstance(tid, int) else tuple(tid)
    return _ScanT(comps, ss, se, ah, al, ri, eob, tid, shape, eob_overrun)


class Written:
    pass


def unit_grid(f):
    """-> (comp, bx, by, padding_only) per data unit, in interleaved order."""
    mcux, mcuy = -(-f.bw // f.hs), -(-f.bh // f.vs)
    out = []
    for my in range(mcuy):
        for mx in range(mcux):
            for c, cc in enumerate(f.comps):
                for v in range(cc.v):
                    for h in range(cc.h):
                        bx, by = mx * cc.h + h, my * cc.v + v
                        out.append((c, bx, by, c == 0 and (bx >= f.bw or by >= f.bh)))
    return out


def _scan_order(f, comps):
    """-> list of MCUs of the scan, each a list of (component, unit index)."""
    grid = unit_grid(f)
    per = len(f.unit_comps())
    mcux, mcuy = -(-f.bw // f.hs), -(-f.bh // f.vs)
    if len(comps) > 1:
        return [[(grid[u][0], u) for u in range(m * per, (m + 1) * per) if grid[u][0] in comps] for m in range(mcux * mcuy)]
    c = comps[0]
    at = {(bx, by): u for u, (cc, bx, by, pad) in enumerate(grid) if cc == c and not pad}
    w, h = (f.bw, f.bh) if c == 0 else (mcux, mcuy)
    return [[(c, at[(x, y)])] for y in range(h) for x in range(w)]


def _make_table(symbols, shape):
    """A DHT from the symbols a scan uses, most frequent first.  The all-ones word of the longest length stays unused."""
    n = len(symbols)
    assert 1 <= n <= 162, "the scanner, like the reference, takes at most 162 symbols per table"
    counts = [0] * 16
    flat = lambda k: max(1, int(k).bit_length())           # 2 ** L >= k + 1
    if shape == "long":
        counts[11] = n
    elif shape == "skew" and n > 2:
        m = min(n - 1, 5)
        for ln in range(1, m + 1):
            counts[ln - 1] = 1
        counts[m + flat(n - m) - 1] = n - m
    else:
        counts[flat(n) - 1] = n
    return Table(counts, symbols)


def _sign_mag(v, al):
    a = abs(int(v)) >> al
    return a if v >= 0 else -a


def build(frame, target, script, damage=None, legal=True):
    """-> Written.  `damage`: a Damage applied while the tokens are written.  legal=False admits a refinement scan repeated at the same
    Ah/Al and an AC first band over slots an earlier scan reached (the intent then has no coefficients: only a decoder knows them)."""
    f = frame
    grid = unit_grid(f)
    nu = len(grid)
    target = np.asarray(target, np.int64)
    assert target.shape == (nu, 64) and np.abs(target).max() <= 32767
    head = bytearray(b"\xff\xd8")
    for tq in sorted(f.qt):
        p16 = tq in f.qt16
        head += _seg(0xDB, bytes([(0x10 if p16 else 0) | tq]) + b"".join(v.to_bytes(2 if p16 else 1, "big") for v in f.qt[tq]))
    body = bytes([8, f.height >> 8, f.height & 255, f.width >> 8, f.width & 255, len(f.comps)])
    for j, c in enumerate(f.comps):
        body += bytes([j + 1, (c.h << 4) | c.v, c.tq])
    head += _seg(0xC2, body)

    reached = np.full((nu, 64), -1, np.int64)              # lowest Al a scan has reached
    w = Written()
    w.frame, w.parts, w.scans, w.tokens, w.forms = f, [], [], [], set()
    cur_ri = 0
    formula = True
    for si, sc in enumerate(script):
        dc_scan, refine = sc.ss == 0, sc.ah != 0
        assert (sc.se == 0 if dc_scan else len(sc.comps) == 1 and 1 <= sc.ss <= sc.se <= 63) and sc.al <= 13
        assert not refine or sc.al == sc.ah - 1
        order = _scan_order(f, sc.comps)
        ri = cur_ri if sc.ri is None else sc.ri
        toks = []                                          # (block, kind, table key, symbol or None, extra bit string, restart segment)
        eobrun, be, seg = 0, [], 0                         # be: correction bits owed by the blocks of the run [(block, bit)]
        pred = {c: 0 for c in sc.comps}
        flush_at = iter(())
        if isinstance(sc.eob, tuple) and sc.eob[0] == "lengths":
            import itertools
            flush_at = itertools.cycle(sc.eob[1])
        rng = np.random.default_rng(sc.eob[1]) if isinstance(sc.eob, tuple) and sc.eob[0] == "random" else None
        want_run = next(flush_at, None)

        def emit_eobrun(at_restart=False):
            nonlocal eobrun, be
            if eobrun:
                if at_restart and sc.eob_overrun:
                    eobrun = min(0x7FFF, eobrun + sc.eob_overrun)
                    w.forms.add("eob_run_cut_by_a_restart_" + ("refine" if refine else "first"))
                nb = eobrun.bit_length() - 1
                toks.append((eob_block, "eobn", tkey, nb << 4, format(eobrun - (1 << nb), f"0{nb}b") if nb else "", seg))
                w.forms.add(f"eob{nb}_" + ("refine" if refine else "first"))
                if nb and eobrun == (1 << nb):
                    w.forms.add(f"eob{nb}_extra_zeros")
                if nb and eobrun == (2 << nb) - 1:
                    w.forms.add(f"eob{nb}_extra_ones")
                if eobrun > 1 and be:
                    w.forms.add("corrections_inside_an_eob_run")
                eobrun = 0
            for blk, bit in be:
                toks.append((blk, "corr", tkey, None, str(bit), seg))
            be = []

        b = -1
        eob_block = 0
        for m, mcu in enumerate(order):
            if ri and m and m % ri == 0:
                emit_eobrun(at_restart=True)
                seg += 1
                pred = {c: 0 for c in sc.comps}
                w.forms.add("restart_" + ("dc" if dc_scan else "ac") + ("_refine" if refine else "_first"))
            for c, u in mcu:
                b += 1
                tkey = sc.tid[sc.comps.index(c)]
                hit = damage is not None and damage.scan == si and damage.block == b
                if hit:
                    emit_eobrun()
                    toks.append((b, "damage", tkey, damage.arg if damage.kind == "sym" else None, "1" * 16 if damage.kind == "raw" else "", seg))
                if dc_scan and not refine:
                    assert reached[u, 0] == -1 or not legal
                    v = int(target[u, 0]) >> sc.al
                    size, vb = value_bits(v - pred[c])
                    assert size <= 11
                    pred[c] = v
                    toks.append((b, "dc", tkey, size, format(vb, f"0{size}b") if size else "", seg))
                    reached[u, 0] = sc.al
                elif dc_scan:
                    assert reached[u, 0] == sc.al + 1 or (not legal and reached[u, 0] == sc.al)
                    toks.append((b, "dcbit", tkey, None, str((int(target[u, 0]) >> sc.al) & 1), seg))
                    reached[u, 0] = sc.al
                elif not refine:                           # AC first (T.81 G.1.2.2)
                    band = range(sc.ss, sc.se + 1)
                    if legal:
                        assert (reached[u, sc.ss:sc.se + 1] == -1).all(), "an AC first scan over slots an earlier scan reached"
                    elif (reached[u, sc.ss:sc.se + 1] != -1).any():
                        formula = False
                        w.forms.add("overlapping_ac_first_band")
                    r = 0
                    for z in band:
                        t = _sign_mag(target[u, z], sc.al)
                        if t == 0:
                            r += 1
                            continue
                        emit_eobrun()
                        while r > 15:
                            toks.append((b, "zrl", tkey, 0xF0, "", seg))
                            w.forms.add("zrl_first")
                            r -= 16
                        size, vb = value_bits(t)
                        assert size <= 10
                        toks.append((b, "ac", tkey, (r << 4) | size, format(vb, f"0{size}b"), seg))
                        if z == sc.se:
                            w.forms.add("first_coefficient_at_se")
                        r = 0
                    reached[u, sc.ss:sc.se + 1] = sc.al
                    if r > 0:
                        if eobrun == 0:
                            eob_block = b
                        eobrun += 1
                else:                                      # AC refinement (T.81 G.1.2.3): correction bits go after the next code word
                    rz = reached[u, sc.ss:sc.se + 1]
                    assert ((rz == sc.al + 1) | ((rz == sc.al) & (not legal))).all(), "a refinement scan needs the level above it"
                    if (rz == sc.al).any():
                        w.forms.add("refinement_repeated")
                    hist = [abs(int(target[u, z])) >> int(reached[u, z]) != 0 for z in range(sc.ss, sc.se + 1)]
                    mag = [abs(int(target[u, z])) >> sc.al for z in range(sc.ss, sc.se + 1)]
                    new = [k for k in range(len(mag)) if not hist[k] and mag[k] == 1]
                    last_new = new[-1] if new else -1
                    r, br = 0, []
                    for k, z in enumerate(range(sc.ss, sc.se + 1)):
                        if not hist[k] and mag[k] == 0:
                            r += 1
                            continue
                        while r > 15 and k <= last_new:
                            emit_eobrun()
                            toks.append((b, "zrl", tkey, 0xF0, "", seg))
                            w.forms.add("zrl_refine_with_corrections" if br else "zrl_refine")
                            r -= 16
                            toks.extend((blk, "corr", tkey, None, str(bit), seg) for blk, bit in br)
                            br = []
                        if hist[k]:
                            br.append((b, mag[k] & 1))
                            if target[u, z] < 0 and mag[k] & 1:
                                w.forms.add("correction_of_a_negative_coefficient")
                            continue
                        assert mag[k] == 1, "a coefficient the level above should have reached"
                        emit_eobrun()
                        toks.append((b, "acr", tkey, (r << 4) | 1, "1" if target[u, z] >= 0 else "0", seg))
                        if k and hist[k - 1]:
                            w.forms.add("new_coefficient_after_a_nonzero_history_one")
                        if z == sc.se:
                            w.forms.add("new_coefficient_at_se")
                        toks.extend((blk, "corr", tkey, None, str(bit), seg) for blk, bit in br)
                        r, br = 0, []
                    reached[u, sc.ss:sc.se + 1] = sc.al
                    if r > 0 or br:
                        if eobrun == 0:
                            eob_block = b
                        eobrun += 1
                        if br:
                            w.forms.add("eob_in_a_block_that_owes_corrections")
                        be += br
                if not dc_scan and eobrun:
                    if (eobrun == 0x7FFF or sc.eob == "single" or (want_run is not None and eobrun >= want_run)
                            or (rng is not None and rng.random() < 0.3)):
                        if eobrun == 0x7FFF:
                            w.forms.add("eobrun_flushed_at_32767")
                        emit_eobrun()
                        want_run = next(flush_at, None)
        if eobrun and b == eob_block + eobrun - 1:
            w.forms.add("eob_run_ends_on_the_last_block")
        emit_eobrun()

        # the tables: one DHT per scan from the symbols it uses, most frequent first
        used = {}
        for blk, kind, tkey, sym, extra, sg in toks:
            if sym is not None:
                used.setdefault(tkey, {}).setdefault(sym, 0)
                used[tkey][sym] += 1
        tables = {k: _make_table(sorted(d, key=lambda s: (-d[s], s)), sc.shape) for k, d in used.items()}
        pre = bytearray(head if si == 0 else b"")
        for k in sorted(tables):
            pre += _seg(0xC4, tables[k].segment(0 if dc_scan else 1, k))
        if ri != cur_ri:
            pre += _seg(0xDD, bytes([ri >> 8, ri & 255]))
            w.forms.add("dri_back_to_0" if ri == 0 else "dri_changed_between_scans" if si else "dri")
            cur_ri = ri
        pre += _seg(0xDA, bytes([len(sc.comps)]) + b"".join(bytes([c + 1, (t << 4) | t]) for c, t in zip(sc.comps, sc.tid))
                    + bytes([sc.ss, sc.se, (sc.ah << 4) | sc.al]))
        segs = [[] for _ in range(seg + 1)]
        pos = [0] * (seg + 1)
        for blk, kind, tkey, sym, extra, sg in toks:
            code = tables[tkey].code_bits(sym) if sym is not None else ""
            w.tokens.append((si, blk, kind, sg, pos[sg], len(code), len(extra)))
            segs[sg].append(code + extra)
            pos[sg] += len(code) + len(extra)
        segs = ["".join(x) for x in segs]
        segs = [x + "1" * (-len(x) % 8) for x in segs]
        w.parts.append((bytes(pre), segs))
        w.scans.append(dict(n_comp=len(sc.comps), comp=list(sc.comps), ss=sc.ss, se=sc.se, ah=sc.ah, al=sc.al, restart_interval=ri,
                            tables=[(tables[t] if t in tables else None) for t in sc.tid], tid=list(sc.tid), n_blocks=b + 1,
                            blocks_per_mcu=len(order[0]), ecs=_bytes_of("".join(segs))))
        w.forms.add(("dc" if dc_scan else "ac") + ("_refine" if refine else "_first"))
        if len(sc.comps) > 1:
            w.forms.add("interleaved_dc" + ("_refine" if refine else "_first"))
        elif (f.hs, f.vs) != (1, 1):
            w.forms.add(f"noninterleaved_{'luma' if sc.comps[0] == 0 else 'chroma'}_{'dc' if dc_scan else 'ac'}_in_a_subsampled_frame")
        if not dc_scan and sc.ss == sc.se:
            w.forms.add("ss_equals_se")
        if not dc_scan and sc.ss <= 48 and sc.se >= 52:
            w.forms.add("band_holds_slots_48_and_52")
        if not dc_scan and 48 <= sc.ss <= 52 and sc.se > 52 or not dc_scan and sc.ss < 48 and 48 <= sc.se < 52:
            w.forms.add("band_split_between_slots_48_and_52")
        if sc.al >= 2 and refine:
            w.forms.add("three_or_more_levels")
        w.forms.add(f"table_id_{max(sc.tid)}")
    w.data = assemble(w.parts)
    it = Intent(nu)
    it.visited[:] = True
    if formula:
        t, r = target, np.maximum(reached, 0)
        it.slots[:] = np.where(reached < 0, 0, np.sign(t) * ((np.abs(t) >> r) << r))
        dc = np.where(reached[:, 0] < 0, 0, (t[:, 0] >> r[:, 0]) << r[:, 0])
        it.slots[:, 0] = ((dc + 32768) & 0xFFFF) - 32768
    else:
        it.slots = None
    it.err_scan = it.err_block = -1
    if damage is not None:
        sc = script[damage.scan]
        dc_first, ac_first = sc.ss == 0 and sc.ah == 0, sc.ss != 0 and sc.ah == 0
        assert not (sc.ss == 0 and sc.ah), "a DC refinement scan has no symbols to damage"
        sym = damage.arg if damage.kind == "sym" else 0xFF
        if dc_first:
            it.status = DC_SYM if sym == 0xFF else DC_LEN
            assert sym == 0xFF or sym > 11
        elif ac_first:
            assert sym == 0xFF or sym & 15 > 10 or (sym >> 4) > sc.se - sc.ss or sym == 0xF0 and sc.se - sc.ss < 15
            it.status = AC_SYM if sym == 0xFF else AC_RUN if (sym >> 4) > sc.se - sc.ss or sym == 0xF0 else AC_LEN
        else:
            assert sym == 0xFF or sym & 15 > 1
            it.status = AC_SYM
        it.err_scan, it.err_block, it.slots = damage.scan, damage.block, None
        w.forms.add(f"damage_{damage.kind}")
    w.intent, w.reached = it, reached
    return w


def _bytes_of(bits):
    assert len(bits) % 8 == 0
    return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def assemble(parts, eoi=True):
    out = bytearray()
    for pre, segs in parts:
        out += pre
        for k, sb in enumerate(segs):
            if k:
                out += bytes([0xFF, 0xD0 + (k - 1) % 8])
            out += _stuffed(sb)
    return bytes(out + (b"\xff\xd9" if eoi else b""))


def cut(w, scan, where, pick):
    """A broken stream derived from the valid one `w`: scan `scan` ends at a byte boundary inside a token.  where: "code" (inside a
    code word) | "bits" (inside, or right before, the value / extra / refinement / correction bits).  pick(block, kind) chooses among the
    tokens that hold such a boundary.  -> (data, status, erring block, kind of the token) or None when no token fits."""
    for si, blk, kind, sg, pos, ncode, nextra in w.tokens:
        if si != scan or not pick(blk, kind):
            continue
        if where == "code":
            b = (pos + ncode - 1) // 8 * 8
            if not (ncode and pos < b):
                continue
        else:
            b = (pos + ncode + 7) // 8 * 8
            if not (nextra and b < pos + ncode + nextra):
                continue
        parts = [(pre, list(segs)) for pre, segs in w.parts]
        pre, segs = parts[scan]
        parts[scan] = (pre, segs[:sg] + [segs[sg][:b]])
        dc = kind in ("dc", "dcbit")
        status = (DC_SYM if dc else AC_SYM) if where == "code" else (DC_BITS if dc else AC_BITS)
        return assemble(parts), status, blk, kind
    return None


# ---- the model: a plain bit-level decoder of SOF2 files (ITU T.81 G.2, figures G.3-G.7, A.2.3) -----------------------------------------
# It shares nothing with the writer above but the bit-string helpers of jpeg_symbols.py, and follows the rules this library documents:
# scan bytes destuffed with RSTn removed and an align() at each restart (damage in one interval is not resynchronised, as in the
# reference), a read past the end of a scan fails, the first error ends the picture's decode (later scans are parsed, not run), every
# store truncates to int16, and an AC first scan stores zeros over the slots of a run and of a ZRL, as the reference does
# (src/jpeg_scanner.cpp:570-572,591-593) -- visible only where bands overlap.

class _Fail(Exception):
    pass


class Decoded:
    def as_intent(self):
        """The coefficients as an Intent (every slot visited), for jpeg_symbols.intent_buffer and intent_rgb."""
        it = Intent(self.coef.shape[0])
        it.visited[:] = True
        it.slots[:] = self.coef
        it.status = self.status
        return it


def decode(data, zigzag="t81"):
    """-> Decoded: status (PJD_ST_* class), err_scan, err_block (in the scan's block order), coef (n_units x 64: per zigzag slot for
    zigzag="t81", which keeps history per slot as pjd_k_progressive does; per natural position for zigzag="reference", where stores and
    the refinement history go through the reference's map, in which slots 48 and 52 share position 38), scans (what each scan says and
    holds, its tables and block order)."""
    index = list(range(64)) if zigzag == "t81" else K_ZZ
    assert zigzag in ("t81", "reference") and data[:2] == b"\xff\xd8"
    p, n = 2, len(data)
    huff, ri, comps, X, Y = {}, 0, None, 0, 0
    d = Decoded()
    d.status, d.err_scan, d.err_block, d.scans, d.coef = OK, -1, -1, [], None
    while True:
        assert data[p] == 0xFF, "a marker is expected"
        while data[p + 1] == 0xFF:
            p += 1
        m = data[p + 1]
        p += 2
        if m == 0xD9:
            break
        ln = (data[p] << 8) | data[p + 1]
        seg = data[p + 2:p + ln]
        p += ln
        if m == 0xC2:
            Y, X = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            comps = [(seg[6 + 3 * k] - 1, seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15) for k in range(seg[5])]
            assert [c for c, _, _ in comps] == list(range(len(comps)))
            hmax, vmax = max(h for _, h, _ in comps), max(v for _, _, v in comps)
            mcux, mcuy = -(-X // (8 * hmax)), -(-Y // (8 * vmax))
            first, per = [], 0
            for _, h, v in comps:
                first.append(per)
                per += h * v
            d.coef = np.zeros((mcux * mcuy * per, 64), np.int32)
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                huff[(seg[q] >> 4, seg[q] & 15)] = (counts, list(seg[q + 17:q + 17 + total]))
                q += 17 + total
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            sel = [(seg[1 + 2 * k] - 1, seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            ecs = bytearray()
            while True:                                    # destuff, drop RSTn, stop at any other marker
                if data[p] != 0xFF:
                    ecs.append(data[p]); p += 1
                elif data[p + 1] == 0:
                    ecs.append(0xFF); p += 2
                elif 0xD0 <= data[p + 1] <= 0xD7:
                    p += 2
                elif data[p + 1] == 0xFF:
                    p += 1
                else:
                    break
            # the blocks of the scan in T.81 A.2.3's order: [(component, unit, a restart happens before it)]
            unit = lambda c, bx, by: ((by // comps[c][2]) * mcux + bx // comps[c][1]) * per + first[c] + (by % comps[c][2]) * comps[c][1] + bx % comps[c][1]
            order = []
            if ns > 1:
                for mi in range(mcux * mcuy):
                    k0 = len(order)
                    for c, _, _ in sel:
                        for v in range(comps[c][2]):
                            for h in range(comps[c][1]):
                                order.append([c, unit(c, (mi % mcux) * comps[c][1] + h, (mi // mcux) * comps[c][2] + v), 0])
                    order[k0][2] = int(ri != 0 and mi != 0 and mi % ri == 0)
            else:
                c = sel[0][0]
                wc, hc = -(-(-(-X * comps[c][1] // hmax)) // 8), -(-(-(-Y * comps[c][2] // vmax)) // 8)
                for mi in range(wc * hc):
                    order.append([c, unit(c, mi % wc, mi // wc), int(ri != 0 and mi != 0 and mi % ri == 0)])
            tabs = {c: huff.get((0 if ss == 0 else 1, td if ss == 0 else ta)) for c, td, ta in sel}
            rec = dict(n_comp=ns, comp=[c for c, _, _ in sel], ss=ss, se=se, ah=ah, al=al, restart_interval=ri, tables=tabs,
                       ecs=bytes(ecs), order=order)
            d.scans.append(rec)
            if d.status == OK:
                try:
                    _run_scan(d, rec, index)
                except _Fail as e:
                    d.status, d.err_scan = e.args[0], len(d.scans) - 1
    return d


def _codes(table):
    """{(length, code): symbol} of a DHT (T.81 C.2: codes of one length count up, then a zero is appended)."""
    out, code, q = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(table[0][ln - 1]):
            out.setdefault((ln, code), table[1][q])
            code += 1
            q += 1
        code <<= 1
    return out


def _run_scan(d, rec, index):
    bits = "".join(format(x, "08b") for x in rec["ecs"])
    nbits = len(bits)
    pos = 0
    ss, se, ah, al = rec["ss"], rec["se"], rec["ah"], rec["al"]
    p1, m1 = 1 << al, -(1 << al)
    codes = {c: (_codes(t) if t else {}) for c, t in rec["tables"].items()}
    coef = d.coef

    def take(k, cls):
        nonlocal pos
        if k == 0:
            return 0
        if nbits - pos < k:
            raise _Fail(cls)
        v = int(bits[pos:pos + k], 2)
        pos += k
        return v

    def symbol(c, cls):
        nonlocal pos
        tab = codes[c]
        for ln in range(1, 17):
            if pos + ln > nbits:
                raise _Fail(cls)
            s = tab.get((ln, int(bits[pos:pos + ln], 2)))
            if s is not None:
                pos += ln
                if s == 0xFF:
                    raise _Fail(cls)                       # the reference's "no symbol" value
                return s
        raise _Fail(cls)

    def correct(row, z):
        cur = int(row[index[z]])
        if cur != 0 and take(1, AC_BITS) and (cur & p1) == 0:
            row[index[z]] = wrap16(cur + (p1 if cur >= 0 else m1))
        return cur

    pred, eobrun = {}, 0
    for blk, (c, u, restart) in enumerate(rec["order"]):
        d.err_block = blk
        if restart:
            pred, eobrun = {}, 0
            if pos // 8 < nbits // 8 and pos % 8:
                pos += 8 - pos % 8
        row = coef[u]
        if ss == 0 and ah == 0:                            # G.1.2.1, first scan: the DC difference, point-transformed
            s = symbol(c, DC_SYM)
            if s > 11:
                raise _Fail(DC_LEN)
            pred[c] = pred.get(c, 0) + extend(s, take(s, DC_BITS))
            row[0] = wrap16(pred[c] << al)
        elif ss == 0:                                      # G.1.2.1, refinement: one bit
            if take(1, DC_BITS):
                row[0] = wrap16(int(row[0]) | p1)
        elif ah == 0:                                      # G.1.2.2 (figures G.3-G.6 read backwards)
            if eobrun:
                eobrun -= 1
                continue
            z = ss
            while z <= se:
                s = symbol(c, AC_SYM)
                run, size = s >> 4, s & 15
                if size:
                    if z + run > se:
                        raise _Fail(AC_RUN)
                    for _ in range(run):
                        row[index[z]] = 0
                        z += 1
                    if size > 10:
                        raise _Fail(AC_LEN)
                    row[index[z]] = wrap16(extend(size, take(size, AC_BITS)) << al)
                    z += 1
                elif run == 15:
                    if z + 15 > se:
                        raise _Fail(AC_RUN)
                    for _ in range(15):
                        row[index[z]] = 0
                        z += 1
                    z += 1
                else:
                    eobrun = (1 << run) - 1 + take(run, AC_BITS)
                    break
        else:                                              # G.1.2.3 (figure G.7 read backwards)
            z = ss
            if eobrun == 0:
                while z <= se:
                    s = symbol(c, AC_SYM)
                    run, size = s >> 4, s & 15
                    new = 0
                    if size:
                        if size != 1:
                            raise _Fail(AC_SYM)
                        new = p1 if take(1, AC_BITS) else m1
                    elif run != 15:
                        eobrun = (1 << run) + take(run, AC_BITS)
                        break
                    while z <= se:                         # zero-history slots are counted, the others corrected on the way
                        if correct(row, z) == 0:
                            if run == 0:
                                break
                            run -= 1
                        z += 1
                    if new and z <= se:
                        row[index[z]] = wrap16(new)
                    z += 1
            if eobrun:
                while z <= se:
                    correct(row, z)
                    z += 1
                eobrun -= 1
    d.err_block = -1
