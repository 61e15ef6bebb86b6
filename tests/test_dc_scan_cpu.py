"""The streams of tests/dc_scan_corpus.py held on the CPU (no GPU): the planner cuts every member into the lanes the plain-Python model
gives, heads and lanes without a unit start lie where the corpus claims, the DC sums leave 16 bits as often as it says, the intent is
what the oracle port decodes, the batch compositions of tests/test_gpu_dc_scan.py put their lanes on the global indices they are about,
and pjd_batch_info.dc_plan reports the form the planner chose."""
import numpy as np
import pytest

import dc_scan_corpus as D
import jpeg_symbols as J

PLAN_ENV = ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE", "PJD_DC_FORM", "PJD_FORCE_SEQUENTIAL")


@pytest.fixture
def lanes128(monkeypatch):
    monkeypatch.setenv("PJD_SUB_BYTES", str(D.S))
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)


def _scan(items):
    from test_gpu_symbol_streams import _scan as scan
    return scan(items)


@pytest.fixture(scope="module")
def layouts():
    """label -> (Scanned, Layout) of every member"""
    items = D.corpus()
    return {x[0]: (s, D.layout(s)) for x, s in zip(items, _scan(items))}


def _lanes(layouts):
    return {label: lay.n for label, (_, lay) in layouts.items()}


def test_planner_cuts_every_member_as_the_model_does(lanes128, layouts):
    import pjd_amd
    for label, data, fr, it in D.corpus():
        s, lay = layouts[label]
        info = pjd_amd.plan_info([s.desc])
        assert info["sub_bytes"] == D.S and info["n_sequential"] == 0, label
        assert info["n_subsequences"] == lay.n, (label, info["n_subsequences"], lay.n)
        want = D.MEMBERS[label]["seg_lanes"]
        if want is not None:
            assert lay.seg_lanes == want, (label, lay.seg_lanes[:8])
        assert len(data) < 300_000, label


def test_ladder_and_heads_lie_where_they_claim(layouts):
    for n in D.LADDER:
        _, lay = layouts[f"ladder{n}"]
        assert lay.n == n and lay.heads == [0], n
    assert layouts["heads_255_511"][1].heads == [0, 255, 511]
    assert layouts["heads_256_512"][1].heads == [0, 256, 512]
    assert layouts["heads_257"][1].heads == [0, 257]
    lay = layouts["heads_every_lane"][1]
    assert lay.heads == list(range(lay.n)) and lay.n == 576 > 2 * D.DC_BLOCK
    assert max(b1 - b0 for b0, b1 in lay.lanes) <= D.S
    # the single head: first lane of a block, 1023 headless lanes on either side (three whole blocks without a head each)
    lay = layouts["heads_single_1024"][1]
    assert lay.heads == [0, 1024] and lay.n == 2048 and 1024 % D.DC_BLOCK == 0
    assert {D.corpus()[k][2].sampling() for k in range(len(D.corpus())) if D.corpus()[k][0].startswith("heads_")} == {"444", "grey"}
    for label, (_, lay) in layouts.items():
        if label.startswith(("samp_", "damaged_")):
            assert lay.n >= 600, (label, lay.n)
    assert layouts["samp_420_dri_std"][1].heads == [0, 130, 330, 470]
    kinds = {(len(fr.comps), fr.hs, fr.vs, bool(fr.ri)) for label, _, fr, _ in D.corpus() if label.startswith("samp_")}
    assert kinds == {(3, 2, 2, False), (3, 2, 1, False), (3, 1, 2, False), (3, 2, 2, True), (1, 1, 1, False), (2, 1, 1, False)}


def test_fat_units_leave_lanes_without_a_unit_start(layouts):
    label, data, fr, it = D.member("fat_units")
    _, lay = layouts[label]
    fat = D.MEMBERS[label]["fat_units"]
    assert len(fat) >= 8 and fat == list(range(fat[0], fat[0] + len(fat))) and fat[0] > 100 and fat[-1] < fr.n_units() - 100
    for u in fat:
        nbits = it.unit_bit[u + 1] - it.unit_bit[u]
        assert 180 * 8 <= nbits <= 205 * 8 and it.visited[u].all(), (u, nbits / 8)
    empty = lay.without_unit_start(it.unit_bit)
    assert len(empty) >= 4, empty
    assert min(empty) < D.DC_BLOCK <= max(empty), empty          # on either side of the first block's edge
    for other, (_, l2) in layouts.items():
        if other != label:
            assert not l2.without_unit_start(D.member(other)[3].unit_bit), other


def test_sums_leave_16_bits(layouts):
    """On the intent: the running predictor wraps int16 many times in every member of a few hundred lanes, and some block's aggregate
    (the plain sum of the differences behind its last head) lies outside 0..65535 in every component -- upwards and downwards somewhere
    in the corpus -- so that a sum kept wider than 16 bits, or saturated, gives another picture."""
    above = below = 0
    for label, data, fr, it in D.corpus():
        _, lay = layouts[label]
        diffs = D.diffs_of(label)
        wraps = D.predictor_wraps(fr, it, diffs)
        if lay.n >= 255 and label != "heads_every_lane":
            assert wraps >= 10, (label, wraps)
        sums = np.array(D.block_sums(fr, it, diffs, lay))
        above += int((sums > 65535).sum())
        below += int((sums < 0).sum())
        if lay.n >= 512 and label != "heads_every_lane":
            assert ((sums > 65535) | (sums < 0)).any(axis=0).all(), (label, sums[:4].tolist())
        per = fr.unit_comps()
        if len(fr.comps) > 1:               # the components' sums differ: a predictor taken from another component shows
            tot = [sum(d for u, d in enumerate(diffs[:it.n_decoded]) if per[u % len(per)] == c) & 0xFFFF for c in range(len(fr.comps))]
            assert len(set(tot)) == len(tot), (label, tot)
    assert above >= 20 and below >= 20, (above, below)


def test_intent_is_what_the_port_decodes(port, layouts):
    from test_gpu_symbol_streams import intent_rgb
    skipped = []
    for label, data, fr, it in D.corpus():
        if fr.standard_restart and fr.ri and (fr.hs, fr.vs) != (1, 1):       # written for T.81's restart rule: the port follows the reference's
            skipped.append(label)
            continue
        o = port.decode(data)
        assert o["valid"] and o["huff_rc"] == it.status, (label, o["huff_rc"], it.status)
        assert np.array_equal(o["coef"], J.intent_buffer(fr, it)), label
        assert np.array_equal(o["rgb"], intent_rgb(port, data, fr, it)), label
    assert skipped == ["samp_420_dri_std"]
    label, data, fr, it = D.member("damaged_620")
    assert it.status == J.DC_SYM and 0 < it.n_decoded == it.err_unit < fr.n_units() and not it.visited[it.err_unit:].any()


def _global_heads(labels, layouts):
    """-> (first global lane of every picture, all global head lanes, total lanes) of a batch given by labels"""
    first, heads, at = [], [], 0
    for l in labels:
        lay = layouts[l][1]
        first.append(at)
        heads += [at + h for h in lay.heads]
        at += lay.n
    return first, heads, at


def test_offsets_order(lanes128, layouts):
    import pjd_amd
    order = D.offsets_order({x[0]: layouts[x[0]][1].n for x in D.clean()})
    assert sorted(order) == sorted(x[0] for x in D.clean())
    first, heads, total = _global_heads(order, layouts)
    at = dict(zip(order, first))
    assert at["ladder2049"] % D.DC_BLOCK == 255 and at["ladder257"] % D.DC_BLOCK == 0 and at["heads_single_1024"] % D.DC_BLOCK == 1
    assert (at["heads_single_1024"] + 1024) % D.DC_BLOCK == 1
    info = pjd_amd.plan_info([layouts[l][0].desc for l in order])
    assert info["n_subsequences"] == total and info["n_sequential"] == 0 and info["dc_plan"] == 0          # a picture of 2049 lanes: the scan


@pytest.mark.parametrize("name", sorted(D.CARRY_BATCHES))
def test_carry_batches(lanes128, layouts, monkeypatch, name):
    import pjd_amd
    labels = D.carry_batch(name)
    first, heads, total = _global_heads(labels, layouts)
    assert total > 65536 and -(-total // D.DC_BLOCK) > 256
    if name == "headless_65536":
        assert labels.count("ladder2049") == 32
        assert not {65535, 65536, 65537} & set(heads)
        j = max(k for k in range(len(labels)) if first[k] <= 65535)
        assert labels[j] == "ladder2049" and first[j] < 65535 - D.DC_BLOCK and first[j] + 2049 > 65537 + D.DC_BLOCK       # whole headless blocks around
    else:
        want = 65536 if name == "head_on_65536" else 65535
        assert labels[-1] == "heads_single_1024" and first[-1] + 1024 == want and want in heads
        assert not {want - 1, want + 1} & set(heads)
    descs = [layouts[l][0].desc for l in labels]
    assert sum(int(d.ecs_len) for d in descs) < 10_000_000
    monkeypatch.setenv("PJD_GROUPS", "1")
    info = pjd_amd.plan_info(descs)
    assert info["n_subsequences"] == total and info["n_sequential"] == 0 and info["dc_plan"] == 0


def test_dc_plan_reports_the_form(lanes128, layouts, monkeypatch):
    """Per picture up to 2048 lanes in the largest picture, the scan from 2049; PJD_DC_FORM overrides either way."""
    import pjd_amd
    form = lambda labels: pjd_amd.plan_info([layouts[l][0].desc for l in labels])["dc_plan"] & 0xFF
    for n in D.LADDER:
        assert form([f"ladder{n}"]) == (1 if n <= D.PICTURE_MAX_LANES else 0), n
    assert form(["ladder2048", "heads_single_1024", "ladder2047"]) == 1
    assert form(["ladder1", "ladder2049", "ladder2"]) == 0
    monkeypatch.setenv("PJD_DC_FORM", "scan")
    assert form(["ladder1"]) == 0 and form(["ladder2048"]) == 0
    monkeypatch.setenv("PJD_DC_FORM", "picture")
    assert form(["ladder2049"]) == 1 and form(["ladder1"]) == 1


def test_dc_plan_reports_the_groups(lanes128, layouts, monkeypatch):
    """0 groups below 64 pictures or with a picture of more than 8192 lanes; otherwise three, or what PJD_GROUPS asks for."""
    import pjd_amd
    labels = D.group_batch()
    descs = [layouts[l][0].desc for l in labels]
    assert len(descs) >= D.GROUP_MIN_PICTURES and sum(int(d.ecs_len) for d in descs) < 10_000_000
    groups = lambda ds: pjd_amd.plan_info(ds)["dc_plan"] >> 8
    assert groups(descs) == 3 and groups(descs[:63]) == 0 and groups(descs[:64]) == 3
    assert pjd_amd.plan_info(descs)["dc_plan"] & 0xFF == 1
    for want in (2, 8):
        monkeypatch.setenv("PJD_GROUPS", str(want))
        assert groups(descs) == want
    monkeypatch.setenv("PJD_GROUPS", "1")
    assert groups(descs) == 0
    monkeypatch.delenv("PJD_GROUPS")
    # one picture of exactly 8192 lanes keeps the groups, one of 8193 ends them (and takes the batch to the scan)
    for (mw, mh), want in [((128, 64), 3), ((3, 2731), 0)]:
        item = D.many_lanes(mw, mh)
        s = _scan([item])[0]
        assert D.layout(s).n == mw * mh == D.GROUP_MAX_LANES + (want == 0)
        info = pjd_amd.plan_info(descs + [s.desc])
        assert info["n_sequential"] == 0 and info["dc_plan"] >> 8 == want and info["dc_plan"] & 0xFF == 0, (mw * mh, info["dc_plan"])
