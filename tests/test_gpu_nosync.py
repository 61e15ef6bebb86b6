"""The entropy decoder's safety net on the GPU (run with -m gpu on an MI355X): the streams of tests/nosync_corpus.py, whose lanes never
fall into step by themselves, so that the truth has to travel lane by lane through the re-sync rounds, the cooperative walker, the
generations that stitch waves together and -- where those give up -- the exact kernel, with every downstream launch run again.

Expectation everywhere: the oracle port's status, picture and coefficients byte for byte (for 4:2:0 with ITU T.81's restart rule, which
the reference does not follow, the streams' intent through the port's back end, as in test_gpu_symbol_streams.py).  The routes -- rounds,
flag reasons, fallbacks -- were recorded on the device first and are asserted where the code explains them (DESIGN.md 4.2 has the table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_symbols as J
import nosync_corpus as N
from conftest import golden_bytes
from test_gpu_poisoned_memory import pctx, poison          # noqa: F401  (fixtures: a context whose allocations start as 0xFF / 0xA5)
from test_gpu_symbol_streams import intent_rgb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOL, SEGMENT, NOSYNC, STITCH, TIMEOUT, OVERFLOW, VERIFY = range(7)          # PJD_FLAG_* (pjd_internal.h)
REASONS = ["SYMBOL", "SEGMENT", "NOSYNC", "STITCH", "TIMEOUT", "OVERFLOW", "VERIFY"]

_expected = {}


def expected(port, s):
    """(status, coefficients, RGB picture) of a stream, computed once."""
    if s.name not in _expected:
        if s.fr.standard_restart and s.fr.ri and (s.fr.hs, s.fr.vs) != (1, 1):
            _expected[s.name] = (s.it.status, J.intent_buffer(s.fr, s.it), intent_rgb(port, s.data, s.fr, s.it))
        else:
            o = port.decode(s.data)
            assert o["valid"] and o["huff_rc"] == s.it.status, s.name
            _expected[s.name] = (o["huff_rc"], o["coef"], o["rgb"])
    return _expected[s.name]


def scanned(s, extra=0):
    import pjd_amd
    sc = pjd_amd.Scanned(s.data)
    assert sc.valid, s.name
    sc.desc.flags = (pjd_amd.F_STANDARD_RESTART if s.fr.standard_restart else 0) | extra
    return sc


def route(info):
    keys = ("n_fallback", "n_sequential", "sync_rounds", "fix_rounds", "walks", "walk_lanes", "n_huff_waves", "n_subsequences", "sub_bytes")
    r = {k: info[k] for k in keys}
    r["flags"] = {REASONS[k]: n for k, n in enumerate(info["flag_waves"][:7]) if n}
    return r


def check(port, b, k, s, outs, st, what):
    status, coef, rgb = expected(port, s)
    assert st[k] == status, (s.name, what, st[k], status)
    assert np.array_equal(outs[k], rgb), (s.name, what, "picture differs from the oracle")
    got = b.coefficients(k)
    bad = np.argwhere(got != coef)
    assert bad.size == 0, (s.name, what, "coefficients differ from the oracle at", bad[:4].tolist())


def no_defensive_flag(info, who):
    """No valid input may reach these: a lane that does not reproduce its synchronised state, a bounded wait that ran out, a region
    too small."""
    fw = info["flag_waves"]
    assert fw[VERIFY] == 0 and fw[TIMEOUT] == 0 and fw[OVERFLOW] == 0, (who, fw)


def decode_member(ctx, port, s, replay=True):
    """One picture alone in a batch: decoded, (decoded again, captured and replayed,) checked every time.  -> its route."""
    sc = scanned(s)
    with ctx.batch([sc.desc]) as b:
        b.upload()
        routes = []
        for what in (("first", "second", "replay") if replay else ("first",)):
            if what == "replay":
                b.capture()
            b.decode(); b.sync()
            outs, st = b.download()
            check(port, b, 0, s, outs, st, what)
            info = b.info()
            no_defensive_flag(info, (s.name, what))
            routes.append(route(info))
        assert all(r == routes[0] for r in routes), (s.name, routes)        # the route is a property of the stream, not of the run
    return routes[0]


# ---- 1: every member, both plan modes, decoded twice from one upload, captured and replayed ---------------------------------------------
@pytest.mark.parametrize("mode", ["latency", "throughput"])
@pytest.mark.parametrize("S", [128, 1024])
def test_every_member_equals_the_oracle(port, monkeypatch, S, mode):
    """Each member alone in a batch, cut into lanes of S bytes: status, picture and coefficients equal the oracle's after the first
    decode, after a second one from the same upload and after a captured graph's replay; the three take the same route; the planner
    cut the stream into the lanes the corpus counts on."""
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", str(S))
    monkeypatch.delenv("PJD_WALK_MAX", raising=False)
    ctx = pjd_amd.Context(0)
    try:
        ctx.set_plan_mode(pjd_amd.PLAN_THROUGHPUT if mode == "throughput" else pjd_amd.PLAN_LATENCY)
        for s in N.members(S):
            r = decode_member(ctx, port, s)
            assert r["sub_bytes"] == S and r["n_sequential"] == 0 and r["n_subsequences"] == s.n_lanes(S), (s.name, r)
    finally:
        ctx.close()


# ---- 2: the walker -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk_max", ["0", "1", "64"])
def test_every_member_with_and_without_the_walker(port, monkeypatch, walk_max):
    """PJD_WALK_MAX=0: every chain is settled by rounds alone; 1: the walker takes a chain's last lane -- and walks on into the lanes
    whose entry it changes; 64: every round of every wave is a walk."""
    import pjd_amd
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    monkeypatch.setenv("PJD_WALK_MAX", walk_max)
    ctx = pjd_amd.Context(0)
    try:
        walks = 0
        for s in N.members(128):
            r = decode_member(ctx, port, s, replay=False)
            walks += r["walks"]
            if s.name == "lock_grey_129" and walk_max == "0":
                # one wave of 64 lanes, none of lanes 1..63 ever in step with what enters it: 63 rounds take the truth through the
                # wave and the picture stays on the parallel path (PJD_SYNC_MAX_ITERS is 72; a wave has 64 lanes, so rounds alone
                # always get there, and PJD_FLAG_NOSYNC stays out of reach of a valid stream)
                assert r["n_huff_waves"] == 1 and r["sync_rounds"] == 63 and r["n_fallback"] == 0 and not r["flags"], r
            assert "NOSYNC" not in r["flags"], (s.name, r)
        assert (walks == 0) == (walk_max == "0"), walks
    finally:
        ctx.close()


# ---- 3: routes --------------------------------------------------------------------------------------------------------------------------
# name -> (n_fallback, flag reasons) at 128-byte lanes, default walker; recorded on the device, explained in DESIGN.md 4.2.
# The truth leaves a lane only through the lane behind it, one lane per round, and a wave publishes PJD_GENS = 6 generations of its
# exit: a chain that enters wave w is true there at generation w's + 1 at the earliest, so a chain across k wave boundaries needs
# k + 2 generations -- k <= 4 is stitched, the wave behind a fifth boundary finds at its final check that its entry was stale
# (PJD_FLAG_STITCH), and in a colour picture its stale entry's unit phase usually contradicts its unit count as well
# (PJD_FLAG_SEGMENT, the check in front of the write pass).  An error in front of that wave keeps the picture on the parallel path.
# A lane that STARTS in the true state does not end a chain: the rounds bridge it from its predecessor's exit like any other lane.
# So a class-1 picture is ONE chain: grey ones are stitched up to 6 waves (lane 63's speculative exit, generation 0 of the first
# wave, happens to be true: 63 * 128 bytes are 128 units), 4:2:0 ones up to 5.
ROUTES = {
    "lock_grey_129": (0, set()), "lock_grey_650": (0, set()), "lock_grey_780": (0, set()), "lock_grey_910": (1, {"STITCH"}),
    "lock_grey_1170": (1, {"STITCH"}), "lock_420_22": (0, set()), "lock_420_130": (1, {"SEGMENT", "STITCH"}),
    "chain_short": (0, set()), "chain_63": (0, set()), "chain_70": (0, set()), "chain_x3": (0, set()), "chain_x4": (0, set()),
    "chain_x5": (1, {"STITCH"}), "phase_420": (0, set()), "phase_420_big": (1, {"SEGMENT", "STITCH"}),
    "heads_grey_ri2": (0, set()), "heads_444_ri67": (0, set()), "heads_420_ri34_std": (0, set()), "heads_phase_444_ri500": (0, set()),
    "err_first_wave": (0, {"STITCH"}), "err_behind_flag": (1, {"STITCH"}), "cut_middle": (0, set()),
}


@pytest.fixture
def lanes128(monkeypatch):
    """Lanes of 128 bytes and the planner's own walker threshold and picture groups.  PJD_SUB_BYTES is read when a context opens: this
    fixture stands ahead of pctx in a test's arguments."""
    monkeypatch.setenv("PJD_SUB_BYTES", "128")
    for k in ("PJD_WALK_MAX", "PJD_GROUPS", "PJD_GROUP_CUTS", "PJD_PLAN_MODE"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def routes_128(port):
    """{name: route} of every member, and of the fallback variants, alone in a batch (128-byte lanes, default walker)."""
    import pjd_amd
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PJD_SUB_BYTES", "128")
        mp.delenv("PJD_WALK_MAX", raising=False)
        ctx = pjd_amd.Context(0)
        try:
            return {s.name: decode_member(ctx, port, s, replay=False) for s in N.members(128) + N.fallback_variants()}
        finally:
            ctx.close()


def test_routes(lanes128, routes_128):
    R = routes_128
    for name, (n_fb, reasons) in ROUTES.items():
        assert (R[name]["n_fallback"], set(R[name]["flags"])) == (n_fb, reasons), (name, R[name])
    # some picture ends in the exact kernel for a reason other than a misplaced restart marker
    assert any(r["n_fallback"] == 1 and set(r["flags"]) - {"SEGMENT"} for r in R.values())
    # One wave of 64 never-merging lanes on the DEFAULT route: 58 rounds, then one walk over the last 6 lanes, no fallback.  (That a
    # wave gets through 60 rounds and more -- 63 -- by rounds alone is asserted in test_every_member_with_and_without_the_walker at
    # PJD_WALK_MAX=0, not here.)  These figures pin the walker's threshold as well as the round logic: PJD_WALK_DENSE = 6 lanes for a
    # picture whose lane holds less than PJD_WALK_DENSE_MCUS MCUs' worth of stream (pjd_plan.cpp); whoever changes those constants on
    # purpose updates the numbers.
    one = R["lock_grey_129"]
    assert (one["n_huff_waves"], one["sync_rounds"], one["walks"], one["walk_lanes"], one["n_fallback"]) == (1, 58, 1, 6, 0), one
    # class 1: one chain over the picture -- the waves behind the sixth (grey) or fifth (4:2:0) boundary are flagged, each of them
    for s in N.members(128):
        if s.cls == 1:
            waves = -(-s.n_lanes(128) // N.WAVE)
            stale = max(0, waves - (6 if s.sub == "grey" else 5))
            assert R[s.name]["flags"].get("STITCH", 0) == stale and R[s.name]["n_fallback"] == (stale > 0), (s.name, R[s.name])
            assert set(R[s.name]["flags"]) <= {"STITCH", "SEGMENT"}, (s.name, R[s.name])
    # class 4: chains end at a restart segment's first lane before they cross five wave boundaries
    for s in N.members(128):
        if s.cls == 4:
            assert R[s.name]["n_fallback"] == 0 and not R[s.name]["flags"], (s.name, R[s.name])
    for s in N.fallback_variants():
        assert R[s.name]["n_fallback"] == 1 and set(R[s.name]["flags"]) == {"STITCH"}, (s.name, R[s.name])


# ---- 4: neighbours --------------------------------------------------------------------------------------------------------------------
FALL_BACK = ["chain_x5", "phase_420_big", "err_behind_flag"]
STAY = ["lock_grey_129", "lock_grey_261", "lock_420_22", "chain_short", "chain_70", "phase_444", "heads_444_ri1", "err_first_wave"]
FIXTURES = ["env_61x45_422_q30", "big_640x480_420_q85", "rst4_128x96_444", "env_128x96_420_q100_opt", "env_200x150_444_q85_opt",
            "env_17x9_420_q100", "env_64x48_444_q85", "gray_61x45"]
GROUPS_FROM = 64          # pjd_plan.cpp: picture groups -- the form a decode takes on an idle device -- exist only for batches with at
#                           least this many pictures on the parallel path (and none of them longer than 8192 lanes)


def test_neighbours_of_a_fallback_in_one_batch(lanes128, port, routes_128):
    """72 pictures interleaved -- three times eight that the parallel decoder gives up on, eight never-synchronising ones it settles and
    eight ordinary fixtures, in another order each time: enough for the planner to form picture groups (GROUPS_FROM).  Exactly the
    flagged pictures are decoded again, every picture equals the oracle, and the form a decode takes on an idle device (one chain of
    launches per picture group, each on its own stream; as a graph, parallel branches) and the one it takes beside another decode (a
    single chain) give the same bytes, also replayed as captured graphs: the exact kernel and every downstream launch behind it are
    run again in both."""
    import pjd_amd
    assert os.environ.get("PJD_IDLE_FORM") != "chain", "the idle-device forms are switched off for this process"
    ss = N.streams()
    fall = [ss[n] for n in FALL_BACK] + N.fallback_variants()
    stay = [ss[n] for n in STAY]
    assert len(fall) == len(stay) == len(FIXTURES) == 8
    n_flagged = 3 * sum(routes_128[s.name]["n_fallback"] for s in fall + stay)      # as each of them decoded alone
    assert n_flagged == 24
    fixtures = []
    for n in FIXTURES:
        data = golden_bytes(n)
        o = port.decode(data)
        fixtures.append((n, data, (o["huff_rc"], o["coef"], o["rgb"])))
    names, sc, want = [], [], []
    for rep in range(3):
        for k in range(8):
            trio = [("corpus", fall[k]), ("corpus", stay[(k + 3 * rep) % 8]), ("fixture", fixtures[(k + 5 * rep) % 8])]
            for kind, x in trio[rep:] + trio[:rep]:
                if kind == "corpus":
                    names.append(x.name); sc.append(scanned(x)); want.append(expected(port, x))
                else:
                    names.append(x[0]); sc.append(pjd_amd.Scanned(x[1])); want.append(x[2])
    descs = [s.desc for s in sc]
    plan = pjd_amd.plan_info(descs)
    assert plan["n_images"] - plan["n_sequential"] >= GROUPS_FROM, plan
    assert plan["n_subsequences"] < 72 * 8192 // 8                # far from a picture of 8192 lanes
    probe = (0, 1, 2, 25, 50, 71)
    ctx, other = pjd_amd.Context(0), pjd_amd.Context(0)
    try:
        busy = other.batch(descs + descs)
        busy.upload()
        with ctx.batch(descs) as b:
            b.upload()
            results = []
            for graph in (False, True):
                if graph:
                    b.capture()
                    busy.capture()
                b.decode(); b.sync()                              # alone: the device is idle -> picture groups
                outs, st = b.download()
                results.append(([o.tobytes() for o in outs], st, [b.coefficients(k).tobytes() for k in probe]))
                info = b.info()
                assert info["n_fallback"] == n_flagged and info["n_sequential"] == 0, (graph, info)
                assert info["flag_waves"][STITCH] >= n_flagged, info["flag_waves"]
                no_defensive_flag(info, graph)
                busy.decode()                                     # beside another decode -> one chain
                b.decode()
                busy.sync(); b.sync()
                outs, st = b.download()
                results.append(([o.tobytes() for o in outs], st, [b.coefficients(k).tobytes() for k in probe]))
                assert b.info()["n_fallback"] == n_flagged
            for k, (status, coef, rgb) in enumerate(want):
                assert st[k] == status, (names[k], st[k], status)
                assert np.array_equal(outs[k], rgb), names[k]
                if k < 24 or k in probe:
                    assert np.array_equal(b.coefficients(k), coef), names[k]
        busy.destroy()
    finally:
        other.close()
        ctx.close()
    for r in results[1:]:
        assert r[1] == results[0][1] and r[0] == results[0][0] and r[2] == results[0][2]


# ---- 5: the position rule -------------------------------------------------------------------------------------------------------------
def test_a_flag_behind_the_first_error_does_not_send_the_picture_back(routes_128):
    """what the parallel decoder cannot resolve counts only if it lies at or before the picture's first error.  The same
    chain across five wave boundaries, flagged in its sixth wave: with an invalid code in the first wave the picture keeps its place
    (the flag is counted, nothing is decoded again), with a run past slot 63 inside the sixth wave it goes to the exact kernel.  The
    reference's status and partial picture either way (decode_member checks them); a stream cut inside the chain ends before the wave
    that would flag."""
    R = routes_128
    ss = N.streams()
    assert ss["err_first_wave"].it.status == J.AC_SYM and ss["err_behind_flag"].it.status == J.AC_RUN
    assert R["chain_x5"]["n_fallback"] == 1 and R["chain_x5"]["flags"] == {"STITCH": 1}, R["chain_x5"]
    assert R["err_first_wave"]["n_fallback"] == 0 and R["err_first_wave"]["flags"] == {"STITCH": 1}, R["err_first_wave"]
    assert R["err_behind_flag"]["n_fallback"] == 1 and R["err_behind_flag"]["flags"] == {"STITCH": 1}, R["err_behind_flag"]
    assert R["cut_middle"]["n_fallback"] == 0 and not R["cut_middle"]["flags"], R["cut_middle"]


# ---- 6: downstream of the fallback ------------------------------------------------------------------------------------------------------
DOWNSTREAM = ["phase_420_big", "chain_x5"]          # a 4:2:0 and a grey picture that end in the exact kernel


def _both_ways(ctx, out_format, extra=0, prepare=None):
    """The two pictures in one batch, as they come (-> the parallel decoder, its flag, the exact kernel, every downstream launch again)
    and with PJD_F_FORCE_SEQUENTIAL (-> the exact kernel up front): the outputs of both, which must be the same bytes."""
    import pjd_amd
    got = []
    for force in (0, pjd_amd.F_FORCE_SEQUENTIAL):
        sc = [scanned(N.streams()[n], extra | force) for n in DOWNSTREAM]
        with ctx.batch([s.desc for s in sc], out_format) as b:
            if prepare:
                prepare(b)
            b.upload(); b.decode(); b.sync()
            outs, st = b.download()
            info = b.info()
            assert (info["n_fallback"], info["n_sequential"]) == ((0, 2) if force else (2, 0)), (force, info)
            assert st == [0, 0]
            got.append([o.copy() for o in outs])
    for k, n in enumerate(DOWNSTREAM):
        assert got[0][k].shape == got[1][k].shape and got[0][k].tobytes() == got[1][k].tobytes(), n
    return got[0]


def test_downstream_gray_output_on_poisoned_memory(lanes128, pctx, port):
    import pjd_amd
    outs = _both_ways(pctx, pjd_amd.OUT_GRAY8)
    s = N.streams()["chain_x5"]
    assert outs[1].shape == (s.fr.height, s.fr.width)
    assert np.array_equal(outs[1], expected(port, s)[2][:, :, 0])          # a one-component picture: R = G = B = the plane


def test_downstream_libjpeg_and_reduced_size(lanes128):
    import pjd_amd
    ctx = pjd_amd.Context(0)
    try:
        _both_ways(ctx, pjd_amd.OUT_RGB8, extra=pjd_amd.F_LIBJPEG)
        outs = _both_ways(ctx, pjd_amd.OUT_RGB8, extra=pjd_amd.F_SCALE_1_8)
        s = N.streams()["phase_420_big"]
        assert outs[0].shape == (s.fr.height // 8, s.fr.width // 8, 3)
    finally:
        ctx.close()


def test_downstream_antialiased_resize_and_fp16(lanes128):
    import pjd_amd

    def prepare(b):
        b.set_resize([(224, 224), (96, 160)])
        b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        b.set_normalize(pjd_amd.DT_F16, [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225])
    ctx = pjd_amd.Context(0)
    try:
        outs = _both_ways(ctx, pjd_amd.OUT_RGB8_PLANAR, prepare=prepare)
        assert outs[0].dtype == np.float16 and outs[0].shape == (3, 224, 224) and outs[1].shape == (3, 96, 160)
    finally:
        ctx.close()


def test_downstream_planar_output_bound_to_a_tensor(lanes128):
    """Planar pictures written into a torch tensor of the caller's (a process of its own: torch has to load before the library)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "nosync_torch_cases.py"), "bound_planar"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "CASE OK bound_planar" in r.stdout, (r.stdout[-1500:] + r.stderr[-3000:])
