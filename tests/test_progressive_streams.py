"""Hand-built progressive (SOF2) scans against three pins (CPU only): the writer's intent, a bit-level model of ITU T.81 G.1.2, and the
reference's own decode_MCU_component.

The streams (tests/progressive_corpus.py) are written by tests/jpeg_progressive.py from target coefficients and a scan script; the
coefficients a decoder must end with follow from the script alone.  The model (jpeg_progressive.decode) shares nothing with the writer
but bit-string helpers.  With zigzag="t81" it must equal the intent; with zigzag="reference" it must equal the reference's procedures,
run one scan at a time through oracle/ref_driver.cpp (ref_progressive_scan) where oracle/_ref is built, and the committed record of
what they answered (tests/golden/progressive/ref_record.json) everywhere.

What that pins: the four procedures (DC first, DC refinement, AC first, AC refinement with end-of-band runs), the bit reader's
end-of-data rule and the error each broken stream raises are the reference's.  What it does not: the ORDER of the blocks of a scan --
the reference only knows the interleaved order; the model takes the order from T.81 A.2.3, and test_model_on_libjpeg_files ties that to
libjpeg's files where Pillow is installed."""
import ctypes as C
import functools
import hashlib
import io
import json
import os

import numpy as np
import pytest

import jpeg_progressive as P
import jpeg_symbols as J
import pjd_amd
import progressive_corpus as PC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "progressive")

# the reference's message in its progressive branches -> the status classes it stands for (include/pjd.h, beside PJD_ST_*)
MESSAGE_CLASSES = {
    "": {J.OK},
    ": Error - Invalid DC value\n": {J.DC_SYM, J.DC_BITS},
    ": Error - DC coefficient length greater than 11\n": {J.DC_LEN},
    ": Error - Invalid AC value\n": {J.AC_SYM, J.AC_BITS},
    ": Error - Zero run-length exceeded spectral selection\n": {J.AC_RUN},
    ": Error - AC coefficient length greater than 10\n": {J.AC_LEN},
}


def all_streams(big=True):
    """[(label, data)] of everything the reference is asked about: fixtures, corpus, broken and desynchronised streams, the big picture."""
    out = [(label, w.data) for label, w in PC.corpus()]
    out += [(x[0], x[1]) for x in PC.broken()] + [(x[0], x[1]) for x in PC.desynchronised()]
    if big:
        out.append((PC.big().name, PC.big().data))
    return out


def reference_answer(ref, d):
    """Run the scans of the model's parse `d` through the reference's decode_MCU_component, in the model's block order.
    -> (coefficients n_units x 64 in the reference's natural order, erring scan or -1, good blocks of the last scan run, message)."""
    coef = np.zeros(d.coef.shape, np.int16)
    for si, sc in enumerate(d.scans):
        tables = {c: (np.cumsum([0] + t[0]).astype(np.uint8), t[1]) for c, t in sc["tables"].items() if t is not None}
        order = sc["order"]
        good, msg = ref.progressive_scan(sc["ss"], sc["se"], sc["ah"], sc["al"], tables, sc["ecs"], [u * 64 for _, u, _ in order],
                                         [c for c, _, _ in order], [r for _, _, r in order], coef.reshape(-1))
        if good != len(order):
            return coef, si, good, msg
        assert msg == ""
    return coef, -1, len(d.scans[-1]["order"]), ""


def digest(coef):
    return hashlib.sha256(np.ascontiguousarray(coef, np.int16).tobytes()).hexdigest()


@functools.lru_cache(maxsize=1)
def record():
    with open(os.path.join(GOLDEN, "ref_record.json")) as f:
        return json.load(f)


# ---- writer intent == model ---------------------------------------------------------------------------------------------------------

def test_intent_equals_model_on_every_valid_stream():
    n_formula = 0
    for label, w in PC.corpus() + [(PC.big().name, PC.big())]:
        d = P.decode(w.data)
        assert (d.status, d.err_scan, d.err_block) == (J.OK, -1, -1), label
        assert len(d.scans) == len(w.scans), label
        if w.intent.slots is not None:
            bad = np.argwhere(d.coef != w.intent.slots)
            assert bad.size == 0, (label, "the model differs from the intent at (unit, slot)", bad[:4].tolist())
            n_formula += 1
    assert n_formula >= len(PC.corpus()) - 1           # all but the overlapping-band stream, which only a decoder can know


def test_intent_equals_model_on_every_broken_stream():
    items = PC.broken()
    assert len(items) > 800
    for label, data, fr, status, scan, block, tags in items:
        d = P.decode(data)
        assert (d.status, d.err_scan, d.err_block) == (status, scan, block), (label, J.STATUS_NAMES[d.status], d.err_scan, d.err_block)


@pytest.mark.parametrize("name", PC.FIXTURES)
def test_fixture_is_committed(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        assert f.read() == PC.named()[name].data, "tests/golden/make_progressive_record.py writes what progressive_corpus.named() builds"


# ---- model == the reference's procedures --------------------------------------------------------------------------------------------

def _check_against(answer, label, d):
    coef, err_scan, good, msg = answer
    assert d.status in MESSAGE_CLASSES[msg], (label, msg, J.STATUS_NAMES[d.status])
    assert err_scan == d.err_scan, (label, err_scan, d.err_scan)
    if d.status:
        assert good == d.err_block, (label, good, d.err_block)
    return coef


def test_model_equals_the_live_reference(live_ref):
    """Every stream, scan by scan through decode_MCU_component: coefficients (partial ones at an error), where the error is, and the
    message's class."""
    if live_ref is None:
        pytest.skip("oracle/_ref not built (test_model_equals_the_reference_record pins the model to what it answered)")
    if not live_ref.has_progressive_scan():
        pytest.skip("oracle/_ref is a prebuilt copy older than oracle/ref_driver.cpp and the reference tree is not here to rebuild it "
                    "(where it is, oracle/Makefile rebuilds it; test_model_equals_the_reference_record runs either way)")
    for label, data in all_streams():
        d = P.decode(data, zigzag="reference")
        coef = _check_against(reference_answer(live_ref, d), label, d)
        bad = np.argwhere(coef != d.coef)
        assert bad.size == 0, (label, "the model differs from the reference at (unit, natural position)", bad[:4].tolist())


def test_model_equals_the_reference_record():
    """The same against the committed record of what oracle/_ref answered: [sha256 of the coefficients, erring scan, good blocks,
    message] per stream.  Never skips."""
    rec = record()
    streams = all_streams()
    assert sorted(rec) == sorted(label for label, _ in streams), "tests/golden/make_progressive_record.py records every stream"
    for label, data in streams:
        d = P.decode(data, zigzag="reference")
        sha, err_scan, good, msg = rec[label]
        _check_against((None, err_scan, good, msg), label, d)
        assert digest(d.coef) == sha, label


def test_the_two_maps_differ_only_where_slots_48_and_52_meet():
    """zigzag="reference" sends slots 48 and 52 to natural position 38, for stores and for the refinement history.  A stream with nothing
    in either slot decodes to the same coefficients under both maps; the band-split fixture has values in both, and there the two models
    must differ (else the reference pin would not see the shared position)."""
    for name, differ in [("prog_refine_forms_grey_64x8", False), ("prog_grey_24x16_band_split_48_52", True)]:
        w = PC.named()[name]
        a, b = P.decode(w.data, "t81").coef, P.decode(w.data, "reference").coef
        via = np.zeros_like(a)
        for z in range(64):
            if z != 48:
                via[:, J.K_ZZ[z]] = a[:, z]
        assert (((a[:, 48] != 0) & (a[:, 52] != 0)).any(), not np.array_equal(via, b)) == (differ, differ), name


# ---- the host scanner ------------------------------------------------------------------------------------------------------------------

def _scan_fields(sc):
    return dict(n_comp=int(sc.n_comp), comp=[int(sc.comp[q]) for q in range(sc.n_comp)], ss=int(sc.ss), se=int(sc.se), ah=int(sc.ah),
                al=int(sc.al), restart_interval=int(sc.restart_interval))


def test_scanner_gives_each_scan_its_parameters_tables_and_bytes():
    """pjd_amd.Scanned(..., SCAN_PROGRESSIVE): per scan what the writer put there and what the model parsed -- also after a DHT that
    redefines an id and a DRI that changes the interval or sets it back to 0."""
    seen = set()
    for label, w in PC.corpus():
        s = pjd_amd.Scanned(w.data, options=pjd_amd.SCAN_PROGRESSIVE)
        assert s.valid and s.log == "" and int(s.desc.n_scans) == len(w.scans), (label, s.log)
        d = P.decode(w.data)
        for k, ws in enumerate(w.scans):
            sc = s.desc.scans[k]
            got = _scan_fields(sc)
            assert got == {f: ws[f] for f in got}, (label, k, got)
            assert got == {f: d.scans[k][f] for f in got}, (label, k)
            ecs = bytes(np.ctypeslib.as_array(C.cast(sc.ecs, C.POINTER(C.c_uint8)), (int(sc.ecs_len),))) if sc.ecs_len else b""
            assert ecs == ws["ecs"] == d.scans[k]["ecs"], (label, k)
            if ws["ss"] == 0 and ws["ah"]:
                continue                                   # a DC refinement scan reads no symbols
            for q, t in enumerate(ws["tables"]):
                offs = np.cumsum([0] + t.counts).tolist()
                assert sc.table[q].set and list(sc.table[q].offsets) == offs and list(sc.table[q].symbols)[:len(t.symbols)] == t.symbols, (label, k, q)
        seen |= w.forms & {"dri_changed_between_scans", "dri_back_to_0", "table_id_3"}
    assert seen == {"dri_changed_between_scans", "dri_back_to_0", "table_id_3"}


def _many_scans(n):
    """A grey 8x8 progressive file of n scans: DC first, then DC refinement scans (illegal beyond the first few; the scanner counts)."""
    fr = PC.frame_of("grey", 8, 8)
    w = P.build(fr, np.zeros((1, 64), np.int64), [P.S(0, al=1), P.S(0, ah=1, al=0)])
    pre, segs = w.parts[1]
    return P.assemble([w.parts[0]] + [(pre, segs)] * (n - 1))


def test_scan_count_limit_is_one_number():
    """PJD_MAX_SCANS = 1024: a file of 1024 scans is taken, one of 1025 is rejected whether EOI or another SOS follows, and the planner
    refuses a descriptor that claims more."""
    s = pjd_amd.Scanned(_many_scans(1024), options=pjd_amd.SCAN_PROGRESSIVE)
    assert s.valid and int(s.desc.n_scans) == 1024
    assert pjd_amd.plan_info([s.desc])["n_sequential"] == 1
    for n in (1025, 1026):
        bad = pjd_amd.Scanned(_many_scans(n), options=pjd_amd.SCAN_PROGRESSIVE)
        assert not bad.valid and bad.log == "x.jpg: Error - Too many scans\nx.jpg: Error - Invalid JPEG\n", (n, bad.log)
    s.desc.n_scans = 1025                                  # (the scan array holds 1024; the planner must refuse before reading it)
    with pytest.raises(pjd_amd.PjdError):
        pjd_amd.plan_info([s.desc])
    s.desc.n_scans = 1024


SOS_REJECTS = [
    ((5, 3, 0, 0), "Invalid spectral selection (start greater than end)"),
    ((1, 64, 0, 0), "Invalid spectral selection (end greater than 63)"),
    ((0, 5, 0, 0), "Invalid spectral selection (contains DC and AC)"),
    ((1, 5, 3, 1), "Invalid succesive approximation"),
    ((1, 5, 0, 14), "Invalid successive approximation"),
]


@pytest.mark.parametrize("params,message", SOS_REJECTS)
def test_illegal_sos_parameters_are_rejected(params, message):
    fr = PC.frame_of("grey", 8, 8)
    w = P.build(fr, np.ones((1, 64), np.int64), [P.S(0), P.S(0, 1, 5, 0, 0)])
    pre, segs = w.parts[1]
    k = pre.index(b"\xff\xda")
    ss, se, ah, al = params
    pre = pre[:k + 7] + bytes([ss, se, (ah << 4) | al])
    s = pjd_amd.Scanned(P.assemble([w.parts[0], (pre, segs)]), options=pjd_amd.SCAN_PROGRESSIVE)
    assert not s.valid and s.log == f"x.jpg: Error - {message}\nx.jpg: Error - Invalid JPEG\n", s.log


def test_an_ac_scan_over_two_components_is_rejected():
    fr = PC.frame_of("444", 8, 8)
    w = P.build(fr, np.ones((3, 64), np.int64), [P.S([0, 1, 2]), P.S(0, 1, 5, 0, 0)])
    pre, segs = w.parts[1]
    k = pre.index(b"\xff\xda")
    pre = pre[:k + 2] + bytes([0, 10, 2, 1, 0, 2, 0, 1, 5, 0])
    s = pjd_amd.Scanned(P.assemble([w.parts[0], (pre, segs)]), options=pjd_amd.SCAN_PROGRESSIVE)
    assert not s.valid and s.log == "x.jpg: Error - Invalid spectral selection (AC scan contains multiple components)\nx.jpg: Error - Invalid JPEG\n", s.log


def test_broken_streams_still_scan():
    """Damage inside the entropy-coded bytes is the decoder's to find: the scanner takes every broken stream, scan count unchanged."""
    for label, data, fr, status, scan, block, tags in PC.broken()[::7]:
        s = pjd_amd.Scanned(data, options=pjd_amd.SCAN_PROGRESSIVE)
        assert s.valid and int(s.desc.n_scans) == len(P.decode(data).scans), label


# ---- the model's scan geometry against libjpeg ------------------------------------------------------------------------------------------

def test_model_on_libjpeg_files(port):
    """Pillow's progressive files (libjpeg's scan script: interleaved DC, non-interleaved AC scans of subsampled frames at odd sizes):
    the model's coefficients equal the oracle port's on the baseline encoding of the same picture, under the standard map."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    n = 0
    port.standard_zigzag(True)
    try:
        for sub, name in [(0, "444"), (1, "422"), (2, "420")]:
            for w, h in [(17, 9), (61, 45), (40, 24), (1, 1)]:
                yy, xx = np.mgrid[0:h, 0:w]
                px = np.stack([(xx * 7 + yy * 3) % 256, (xx * yy) % 256, rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
                im = Image.fromarray(px, "RGB")
                files = []
                for prog in (True, False):
                    buf = io.BytesIO()
                    im.save(buf, "JPEG", quality=90, subsampling=sub, progressive=prog, optimize=False)
                    files.append(buf.getvalue())
                d = P.decode(files[0])
                assert d.status == J.OK and len(d.scans) > 3, (name, w, h)
                o = port.decode(files[1])
                assert o["valid"] and o["huff_rc"] == 0
                fr = PC.frame_of(name, w, h)
                assert np.array_equal(J.intent_buffer(fr, d.as_intent()), o["coef"]), (name, w, h)
                n += 1
    finally:
        port.standard_zigzag(False)
    assert n == 12


# ---- coverage ------------------------------------------------------------------------------------------------------------------------

REQUIRED_FORMS = (
    ["dc_first", "dc_refine", "ac_first", "ac_refine", "interleaved_dc_first", "interleaved_dc_refine",
     "noninterleaved_luma_ac_in_a_subsampled_frame", "noninterleaved_chroma_ac_in_a_subsampled_frame",
     "eob_run_ends_on_the_last_block", "eob_run_cut_by_a_restart_first", "eob_run_cut_by_a_restart_refine", "eobrun_flushed_at_32767", "corrections_inside_an_eob_run", "eob_in_a_block_that_owes_corrections",
     "zrl_first", "zrl_refine", "zrl_refine_with_corrections", "new_coefficient_after_a_nonzero_history_one", "new_coefficient_at_se",
     "first_coefficient_at_se", "correction_of_a_negative_coefficient", "three_or_more_levels",
     "restart_dc_first", "restart_dc_refine", "restart_ac_first", "restart_ac_refine", "dri", "dri_changed_between_scans", "dri_back_to_0",
     "table_id_0", "table_id_1", "table_id_2", "table_id_3", "ss_equals_se", "band_holds_slots_48_and_52",
     "band_split_between_slots_48_and_52", "refinement_repeated", "overlapping_ac_first_band"]
    + [f"eob{n}_first" for n in range(15)] + [f"eob{n}_refine" for n in list(range(10)) + [12, 13, 14]]
    + [f"eob{n}_extra_{b}" for n in range(1, 15) for b in ("zeros", "ones")])

# (procedure, status class) a broken stream must reach, each at the first and the last block, right after a restart, and in a first
# (DC first only: no legal file starts with anything else), a middle and the last scan
REQUIRED_ERRORS = [("dc_first", J.DC_SYM), ("dc_first", J.DC_LEN), ("dc_first", J.DC_BITS), ("dc_refine", J.DC_BITS),
                   ("ac_first", J.AC_SYM), ("ac_first", J.AC_RUN), ("ac_first", J.AC_LEN), ("ac_first", J.AC_BITS),
                   ("ac_refine", J.AC_SYM), ("ac_refine", J.AC_BITS)]
REQUIRED_KINDS = (["cut_code_dc", "cut_bits_dc", "cut_bits_dcbit", "cut_code_ac", "cut_bits_ac", "cut_code_eobn", "cut_bits_eobn", "cut_code_acr",
                   "cut_bits_acr", "cut_bits_corr", "cut_code_zrl", "raw", "sym_ff", "sym_02", "sym_13", "sym_f0", "sym_f1"]
                  + [f"sym_{s:02x}" for s in range(0x0B, 0x10)])


def test_coverage_of_forms_frames_progressions_and_errors():
    """Every form, frame, table case, progression and (procedure x status class x position) the suite is meant to hold occurs in the
    fixtures, the corpus, the big picture and the broken streams, by name, so that a later edit cannot drop one quietly."""
    items = PC.corpus() + [(PC.big().name, PC.big())]
    forms = set().union(*(w.forms for _, w in items))
    assert not [f for f in REQUIRED_FORMS if f not in forms], [f for f in REQUIRED_FORMS if f not in forms]
    frames = {(w.frame.sampling(), w.frame.width, w.frame.height) for _, w in items}
    assert {s for s, _, _ in frames} == {"grey", "444", "422", "420", "440"}
    assert {(w, h) for _, w, h in frames} >= {(1, 1), (8, 8), (17, 9), (1, 300), (300, 1), (2048, 1024)}
    n_scans = {label: len(w.scans) for label, w in items}
    assert min(n_scans.values()) == 1 and max(n_scans.values()) > 100
    intervals = {(w.frame.sampling(), sc["restart_interval"], sc["n_comp"]) for _, w in items for sc in w.scans}
    assert ("444", 1, 3) in intervals and ("440", 7, 3) in intervals and ("420", 5, 1) in intervals      # 1, a prime, one luma row of 40x24
    shapes = {tuple(t.counts) for _, w in items for sc in w.scans for t in sc["tables"] if t is not None}
    assert any(c[11] for c in shapes) and any(sum(c[:5]) == 5 for c in shapes)                           # 12-bit codes; a skewed table
    assert [n for n in PC.FIXTURES if n not in dict(items)] == []
    where, kinds = set(), set()
    for label, data, fr, status, scan, block, (proc, spos, bpos, kind) in PC.broken():
        where |= {(proc, status, "block", bpos), (proc, status, "scan", spos)}
        kinds.add(kind)
    assert not [k for k in REQUIRED_KINDS if k not in kinds], [k for k in REQUIRED_KINDS if k not in kinds]
    missing = []
    for proc, status in REQUIRED_ERRORS:
        for bpos in ("first", "last", "after_restart"):
            if (proc, status, "block", bpos) not in where:
                missing.append((proc, J.STATUS_NAMES[status], bpos))
        for spos in (["first"] if proc == "dc_first" else []) + ["middle", "last"]:
            if (proc, status, "scan", spos) not in where:
                missing.append((proc, J.STATUS_NAMES[status], spos))
    assert not missing, missing
    assert len(PC.desynchronised()) == 2               # a run and a ZRL that pass Se in a refinement scan: no error of their own
