"""DC prediction across entropy-decoder lanes on the GPU (run with -m gpu on an MI355X): the streams of tests/dc_scan_corpus.py at
128-byte lanes through both forms of the segmented scan -- the three launches pjd_k_image_verdict / pjd_k_lane_dc_local /
pjd_k_lane_dc_carry over the whole batch, and pjd_k_group_dc, one workgroup per picture -- with heads, headless blocks, chunk ends and
the carry kernel's second chunk where tests/test_dc_scan_cpu.py holds them, in every back end that consumes the predictors, and in
picture groups.  pjd_batch_info.dc_plan says which form a batch took.  Status, coefficients and pictures must equal the streams' intent
(tests/jpeg_symbols.py) and, where the reference's restart rule applies, the oracle port."""
import copy
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import dc_scan_corpus as D
import jpeg_symbols as J
from conftest import ROOT
from test_gpu_scaled import box
from test_gpu_symbol_streams import _decode_and_check, _scan, intent_rgb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN_ENV = ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_DC_FORM", "PJD_FORCE_SEQUENTIAL")
SCAN, PICTURE = 0, 1                  # pjd_batch_info.dc_plan, bits 0..7


@pytest.fixture(scope="module", autouse=True)
def built_once():
    """The corpus is built (some ten seconds) before the first test, not inside it."""
    D.corpus()


@pytest.fixture
def lanes128(monkeypatch):
    monkeypatch.setenv("PJD_SUB_BYTES", str(D.S))
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)


def _form(monkeypatch, form):
    if form == "unset":
        monkeypatch.delenv("PJD_DC_FORM", raising=False)
    else:
        monkeypatch.setenv("PJD_DC_FORM", form)


_EXPECTED = {}


def expected(port, item):
    """label -> (coefficients, picture) of the intent, computed once; the picture is also the port's own decode where its restart
    rule applies."""
    label, data, fr, it = item
    if label not in _EXPECTED:
        coef = J.intent_buffer(fr, it)
        rgb = intent_rgb(port, data, fr, it)
        if not (fr.standard_restart and fr.ri and (fr.hs, fr.vs) != (1, 1)):
            assert np.array_equal(rgb, port.decode(data)["rgb"]), label
        coef.setflags(write=False)
        rgb.setflags(write=False)
        _EXPECTED[label] = (coef, rgb)
    return _EXPECTED[label]


def _no_slow_path(info, items):
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0, (info["n_sequential"], info["n_fallback"], info["flag_waves"])
    if all(x[3].status == J.OK for x in items):
        assert sum(info["flag_waves"]) == 0, info["flag_waves"]


# ---- 1: both forms, the whole corpus ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["unset", "scan", "picture"])
def test_forms(port, lanes128, monkeypatch, form):
    """The whole corpus in one batch.  Left alone the planner takes the scan (a picture of 2049 lanes) and, without that picture, a
    workgroup per picture; PJD_DC_FORM forces either on the same batch."""
    import pjd_amd
    _form(monkeypatch, form)
    items = list(D.corpus())
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["sub_bytes"] == D.S and info["dc_plan"] == (PICTURE if form == "picture" else SCAN), info["dc_plan"]
        if form == "unset":
            rest = [x for x in items if x[0] != "ladder2049"]
            info = _decode_and_check(ctx, port, rest, _scan(rest))
            assert info["dc_plan"] == PICTURE
            _decode_and_check(ctx, port, D.clean(), _scan(D.clean()))          # and nothing flagged in the batch without the damaged member
    finally:
        ctx.close()


# ---- 2: where the batch's blocks cut the pictures ---------------------------------------------------------------------------------------
def test_lane_offsets_in_the_scan_form(port, lanes128):
    """An order (tests/test_dc_scan_cpu.py asserts it) in which a block of the batch-wide scan ends on the 2049-lane picture's head, the
    257-lane picture starts a block and the single head sits one lane into a block."""
    import pjd_amd
    by_label = {x[0]: x for x in D.clean()}
    lanes = {label: D.layout(s).n for label, s in zip(by_label, _scan(list(by_label.values())))}
    items = [by_label[l] for l in D.offsets_order(lanes)]
    ctx = pjd_amd.Context(0)
    try:
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["dc_plan"] == SCAN and info["n_subsequences"] == sum(lanes.values())
    finally:
        ctx.close()


# ---- 3: past 256 blocks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["scan", "picture"])
@pytest.mark.parametrize("name", sorted(D.CARRY_BATCHES))
def test_carry_chunks(port, lanes128, monkeypatch, name, form):
    """More than 65536 lanes, i.e. more than 256 blocks: the carry kernel walks a second chunk of block aggregates.  One-lane pictures,
    then copies of the 2049-lane member (its head one lane further into a block with every copy), with global lanes 65535..65537 in a
    headless stretch, or with the single-head member's head on lane 65536 / 65535.  Every copy is the one expected picture; coefficients
    of the first copy, the copy across lane 65536, the last copy and the last picture."""
    import pjd_amd
    _form(monkeypatch, form)
    monkeypatch.setenv("PJD_GROUPS", "1")                       # many pictures: keep to the single chain, whose form this is about
    labels = D.carry_batch(name)
    one = {l: D.member(l) for l in set(labels)}
    scanned = dict(zip(one, _scan(list(one.values()))))
    first, at = [], 0
    for l in labels:
        first.append(at)
        at += D.layout(scanned[l]).n
    copies = [k for k, l in enumerate(labels) if l == "ladder2049"]
    across = max(k for k in range(len(labels)) if first[k] <= 65536)
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([scanned[l].desc for l in labels]) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            info = b.info()
            assert info["n_subsequences"] == at > 65536 and info["dc_plan"] == (PICTURE if form == "picture" else SCAN), info
            assert st == [0] * len(labels)
            for k in sorted({0, copies[0], across, copies[-1], len(labels) - 1}):
                bad = np.argwhere(b.coefficients(k) != expected(port, one[labels[k]])[0])
                assert bad.size == 0, (name, form, k, labels[k], "coefficients differ from the intent at", bad[:4].tolist())
        for k, l in enumerate(labels):
            assert np.array_equal(outs[k], expected(port, one[l])[1]), (name, form, k, l, first[k])
        _no_slow_path(info, list(one.values()))
    finally:
        ctx.close()


# ---- 4: every back end that adds the carry ----------------------------------------------------------------------------------------------
BACK_ENDS = ["planar", "bmp", "gray", "scale_1_2", "scale_1_8", "libjpeg"]
_WANT = {}


def _want(port, item, kind):
    """The expected output of one member in one back-end form, from the intent's coefficients, computed once."""
    import gray_expected as G
    import libjpeg_model as M
    import pjd_amd
    label, data, fr, it = item
    key = (label, kind)
    if key not in _WANT:
        coef, rgb = expected(port, item)
        if kind == "planar":
            w = rgb.transpose(2, 0, 1)
        elif kind == "bmp":
            w = np.frombuffer(pjd_amd.rgb_to_bmp(rgb), np.uint8)
        elif kind == "gray":
            w = G.ref_plane_of_coefficients(port, data, coef)
        elif kind.startswith("scale"):
            w = box(rgb, int(kind.rsplit("_", 1)[1]))
        else:                                             # PJD_F_LIBJPEG decodes with T.81's zigzag map (and restart rule)
            from test_gpu_libjpeg import desc_qts
            t81 = copy.copy(fr)
            t81.standard_zigzag = True
            s = pjd_amd.Scanned(data)                     # (owns what its descriptor points to)
            w = M.decode(J.intent_buffer(t81, it), desc_qts(s.desc), fr.width, fr.height, len(fr.comps), fr.hs, fr.vs)
        _WANT[key] = np.ascontiguousarray(w)
    return _WANT[key]


@pytest.mark.parametrize("form", ["scan", "picture"])
@pytest.mark.parametrize("kind", BACK_ENDS)
def test_back_ends(port, lanes128, monkeypatch, kind, form):
    """The heads, fat-unit and samplings members through the planar, BMP, grey, reduced-size and libjpeg back ends (each parses the
    lane streams with pjd_k_lanes_parse_body.h and adds block carry and lane predictor itself), under either form."""
    import pjd_amd
    _form(monkeypatch, form)
    items = D.backend_members()
    if kind == "libjpeg":                                 # the mode's envelope: no 4:4:0, no two components
        items = [x for x in items if (x[2].hs, x[2].vs) != (1, 2) and len(x[2].comps) != 2]
        assert len(items) >= len(D.backend_members()) - 2
    scanned = _scan(items)
    flags = {"scale_1_2": pjd_amd.F_SCALE_1_2, "scale_1_8": pjd_amd.F_SCALE_1_8, "libjpeg": pjd_amd.F_LIBJPEG}.get(kind, 0)
    for s in scanned:
        s.desc.flags = int(s.desc.flags) | flags
    fmt = {"planar": pjd_amd.OUT_RGB8_PLANAR, "bmp": pjd_amd.OUT_BMP, "gray": pjd_amd.OUT_GRAY8}.get(kind, pjd_amd.OUT_RGB8)
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([s.desc for s in scanned], fmt) as b:
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            info = b.info()
    finally:
        ctx.close()
    assert info["dc_plan"] == (PICTURE if form == "picture" else SCAN) and info["sub_bytes"] == D.S
    for item, o, status in zip(items, outs, st):
        assert status == item[3].status == 0, (item[0], kind)
        want = _want(port, item, kind)
        assert np.array_equal(np.asarray(o).reshape(want.shape), want), (item[0], kind, form)
    _no_slow_path(info, items)


# ---- 5: picture groups ----------------------------------------------------------------------------------------------------------------------
def _group_items():
    """The group batch and, in front, one picture routed to the exact kernel (no lanes: pjd_k_group_dc leaves its status word alone)."""
    return [D.member("ladder64")] + [D.member(l) for l in D.group_batch()]


def _groups_run(port, items, want_groups, want_chains=None):
    """Decode the group batch in this process' environment; everything against the intent; -> a digest of statuses, coefficients and
    pictures.  want_chains: the form the decode must report (Batch.decode_chains); None: the planner's groups, one chain where it
    made none."""
    import pjd_amd
    scanned = _scan(items)
    scanned[0].desc.flags = int(scanned[0].desc.flags) | pjd_amd.F_FORCE_SEQUENTIAL
    h = hashlib.sha256()
    ctx = pjd_amd.Context(0)
    try:
        with ctx.batch([s.desc for s in scanned]) as b:
            b.upload(); b.decode(); b.sync()
            assert b.decode_chains() == ((want_groups or 1) if want_chains is None else want_chains), (b.decode_chains(), want_groups, want_chains)
            outs, st = b.download()
            info = b.info()
            assert info["dc_plan"] >> 8 == want_groups and info["sub_bytes"] == D.S, info["dc_plan"]
            assert info["n_sequential"] == 1 and info["n_fallback"] == 0, info
            for k, item in enumerate(items):
                coef, rgb = expected(port, item)
                assert st[k] == item[3].status, (k, item[0], st[k])
                got = b.coefficients(k)
                bad = np.argwhere(got != coef)
                assert bad.size == 0, (k, item[0], "coefficients differ from the intent at", bad[:4].tolist())
                assert np.array_equal(outs[k], rgb), (k, item[0])
                h.update(np.int32(st[k]).tobytes() + got.tobytes() + outs[k].tobytes())
    finally:
        ctx.close()
    return h.hexdigest()


_CHAIN_DIGEST = []


def _chain_digest(port, monkeypatch):
    if not _CHAIN_DIGEST:
        monkeypatch.setenv("PJD_GROUPS", "1")
        _CHAIN_DIGEST.append(_groups_run(port, _group_items(), 0))
        monkeypatch.delenv("PJD_GROUPS")
    return _CHAIN_DIGEST[0]


@pytest.mark.parametrize("groups", ["unset", "2", "8"])
def test_picture_groups(port, lanes128, monkeypatch, groups):
    """69 pictures -- the ladder up to 2048 lanes, the heads members and the damaged member four times over, and one picture routed to
    the exact kernel: every group settles its pictures with pjd_k_group_dc on a stream of its own.  Equal to the single chain's
    results (PJD_GROUPS=1) and to the intent."""
    chain = _chain_digest(port, monkeypatch)
    if groups != "unset":
        monkeypatch.setenv("PJD_GROUPS", groups)
    assert _groups_run(port, _group_items(), 3 if groups == "unset" else int(groups)) == chain


def _groups_child(path):
    """In a fresh process: the pickled group batch, groups planned but run as one chain (PJD_IDLE_FORM=chain)."""
    import oracle_lib
    with open(path, "rb") as f:
        items, exp = pickle.load(f)
    _EXPECTED.update(exp)
    return _groups_run(oracle_lib.Port(), items, 3, want_chains=1)


def test_picture_groups_planned_but_run_as_one_chain(port, lanes128, monkeypatch, tmp_path):
    """PJD_IDLE_FORM=chain (read once per process, so in a fresh child): the planner makes its three groups, the decode takes the
    single chain with a workgroup per picture; the same results."""
    chain = _chain_digest(port, monkeypatch)
    items = _group_items()
    path = str(tmp_path / "group_batch.pickle")
    with open(path, "wb") as f:
        pickle.dump((items, {x[0]: expected(port, x) for x in items}), f)
    sys_path = [os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"), HERE, os.path.join(ROOT, "tools")]
    code = "import sys\nsys.path[:0] = %r\nimport test_gpu_dc_scan as T\nprint('RESULT ok', T._groups_child(%r))\n" % (sys_path, path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, PJD_IDLE_FORM="chain"))
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout[-600:] + r.stderr[-3000:])
    assert r.stdout.split("RESULT ok")[1].split()[0] == chain


# ---- 6: the planner's own lane sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_product_chosen_sizes(port, monkeypatch, mode):
    """The ladder without PJD_SUB_BYTES: the batch's lane size and every picture's own adjustment are the planner's, the lane counts
    whatever they make."""
    import pjd_amd
    for k in PLAN_ENV + ("PJD_SUB_BYTES",):
        monkeypatch.delenv(k, raising=False)
    items = D.ladder()
    ctx = pjd_amd.Context(0)
    try:
        ctx.set_plan_mode(pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
        info = _decode_and_check(ctx, port, items, _scan(items))
        assert info["plan_mode"] == (pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
        assert info["dc_plan"] >> 8 == 0
    finally:
        ctx.close()
