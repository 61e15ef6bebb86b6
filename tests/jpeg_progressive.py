"""A small progressive (SOF2) writer for tests (pure Python + numpy), beside the baseline one of tests/jpeg_symbols.py.

It writes one DHT before each scan and SOS with Ss / Se / Ah / Al, from given values:

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

from jpeg_symbols import Intent, _Bits, _seg, _stuffed, value_bits, wrap16

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
