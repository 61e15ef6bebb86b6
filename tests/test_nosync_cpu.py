"""The streams of tests/nosync_corpus.py do what they claim (CPU only): a plain model of the state-only pass shows that their lanes never
reach the true state (class 1), form chains of the designed length (class 2) or agree in everything but the unit's place in the MCU
(class 3); tools/sync_sim.c, where a C compiler is at hand, agrees with the model; the oracle port and the reference's own decoder make
of every file what its tokens intend; and the planner takes every one of them on the parallel path, cut into the lanes the model assumes."""
import bisect
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_symbols as J
import nosync_corpus as N
import symbol_corpus as SC
from test_symbol_streams import check_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(N.streams())


@functools.lru_cache(maxsize=None)
def model(name):
    return N.Model(N.streams()[name])


def of_class(*cls):
    return [s for s in N.streams().values() if s.cls in cls]


# ---- class 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [128, 256, 512, 1024])
def test_lockstep_lanes_never_reach_the_true_state(S):
    """Class 1: at least 90 % of the lanes never equal the true state, whatever the lane size -- over the class, and in every stream of
    32 lanes or more -- and the rest START in it (a unit boundary, in a colour picture the MCU's first).  A model that compares only at
    the lane's end would miss a decoder that is right for a while: the distance is taken over every byte to the end of the stream."""
    lanes_all = never_all = 0
    for s in of_class(1):
        lanes = model(s.name).lockstep_distances(S)
        never = sum(d is None for _, _, d in lanes)
        assert all(d is None or d == 0 for _, _, d in lanes), s.name
        assert lanes[0][2] == 0
        if len(lanes) >= 32:
            assert never >= 0.9 * len(lanes), (s.name, never, len(lanes))
        lanes_all += len(lanes)
        never_all += never
    assert never_all >= 0.9 * lanes_all, (never_all, lanes_all)


def test_lockstep_lane_counts():
    """The sizes the corpus is built for: 2, 63, 64, 65, 128, 129 lanes and 5 to 9 waves at 128 bytes; 2, 63, 64, 65 lanes at 1024."""
    at128 = {s.n_lanes(128) for s in N.members(128) if s.cls == 1 and s.sub == "grey"}
    assert {2, 63, 64, 65, 128, 129, 320, 384, 448, 512, 576} <= at128, at128
    at1024 = {s.n_lanes(1024) for s in N.members(1024) if s.cls == 1 and s.sub == "grey"}
    assert {2, 63, 64, 65} <= at1024, at1024
    assert {s.n_lanes(128) for s in N.members(128) if s.cls == 1 and s.sub == "420"} >= {65, 384, 520}


def test_a_wave_of_lockstep_lanes_is_one_chain():
    """64 lanes of 128 bytes: a grey wave is a chain of 62 lanes (lane 63 starts on a unit boundary: 63 * 128 = 128 * 63), a 4:2:0 wave
    one of 63 or more (that boundary is not the MCU's first unit)."""
    lanes = model("lock_grey_129").lockstep_distances(128)
    assert N.chain_and_cross(N.rounds_needed(lanes, N.scan_bytes(N.streams()["lock_grey_129"]))) == (62, 0)
    lanes = model("lock_420_22").lockstep_distances(128)
    assert len(lanes) == 65
    assert N.chain_and_cross(N.rounds_needed(lanes, N.scan_bytes(N.streams()["lock_420_22"]))) == (64, 1)


# ---- class 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in of_class(2)])
def test_chains_have_the_designed_length(name):
    """Class 2: the most rounds a lane's exit needs -- the truth moving one lane per round from the nearest lane behind it whose own
    decode becomes true in time -- and the most wave boundaries on such a way are what the synchronisers were placed for."""
    s = N.streams()[name]
    lanes = model(name).lockstep_distances(s.design_S)
    assert len(lanes) == s.n_lanes(s.design_S)
    R = N.rounds_needed(lanes, N.scan_bytes(s))
    assert N.chain_and_cross(R) == (s.chain, s.cross), (name, N.chain_and_cross(R))


def test_chain_lengths_and_crossings_in_the_corpus():
    got = {(s.chain, s.cross) for s in of_class(2)}
    assert {(17, 1), (63, 1), (70, 1), (66, 1)} <= got, got
    assert {c for _, c in got} >= {1, 3, 4, 5}
    s = N.streams()["chain_short"]
    R = N.rounds_needed(model("chain_short").lockstep_distances(128), N.scan_bytes(s))
    runs = sorted({r for j, r in enumerate(R) if r and (j + 1 == len(R) or R[j + 1] == 0)})          # the length of every chain
    assert runs == [2, 3, 5, 17], runs


# ---- class 3 ------------------------------------------------------------------------------------------------------------------------
SLOT_SYNC_BYTES = 300         # "a few hundred bytes".  A unit of these tables takes about 8 bytes and ends in an EOB three times in four;
#                               a guessing decoder that reads a true EOB while in a unit's AC part is at "DC expected" with the truth,
#                               so it misses some 37 chances in 300 bytes.  The longest distance in these seeds is 101 bytes.


@pytest.mark.parametrize("name", [s.name for s in of_class(3)])
def test_phase_only_streams_agree_in_all_but_the_phase(name):
    """Class 3: every lane's decoder is at the true bit position and slot within SLOT_SYNC_BYTES (or the stream's end).  From there on
    the two read the same symbols, so its unit phase is right then or never -- and it is wrong for most lanes: 1 in 6 (4:2:0), 4
    (4:2:2) or 3 (4:4:4) guesses is right, at least half of the lanes must never agree.  WHICH lanes agree follows from where they
    start: the guess counts from phase 0, the truth from the phase c0 of the unit the lane starts in, so with n_true and n_spec units
    completed on the way they agree exactly if c0 + n_true - n_spec is a multiple of the MCU's units -- and a lane that completes as
    many units as the truth (every second lane does) agrees exactly if it starts in a unit of phase 0."""
    s, m = N.streams()[name], model(name)
    nbits = 8 * N.scan_bytes(s)
    truth = m.truth(0, N.scan_bytes(s))
    at = sorted(truth)
    never = n = same = 0
    # the exhaustive walk to the stream's end for every lane of the small pictures; 4 KB past the slot's agreement in the large one
    reach = nbits if nbits < 8 * 10000 else 8 * (SLOT_SYNC_BYTES + 4096)
    for q, head in s.lane_starts(128)[1:]:
        slot = m.sync_distance(8 * q, truth, nbits, phase=False)
        full = m.sync_distance(8 * q, truth, min(nbits, 8 * q + reach), phase=True)
        if slot is None:
            assert nbits - 8 * q < 8 * SLOT_SYNC_BYTES, (name, q)
            continue
        assert slot <= 8 * SLOT_SYNC_BYTES, (name, q, slot)
        assert full is None or full == slot, (name, q, slot, full)
        n += 1
        never += full is None
        p, c, z, n_spec = 8 * q, 0, 0, 0
        while p < 8 * q + slot:
            p, c, z = m.step(p, c, z)
            n_spec += z == 0
        c0 = truth[at[bisect.bisect_right(at, 8 * q) - 1]][0]
        n_true = sum(truth[k][1] == 0 for k in at[bisect.bisect_right(at, 8 * q):bisect.bisect_right(at, p)])
        assert (full is not None) == ((c0 + n_true - n_spec) % m.dus == 0), (name, q, c0, n_true, n_spec)
        if n_true == n_spec:
            same += 1
            assert (full is not None) == (c0 == 0), (name, q, c0)
    assert n >= 20 and never >= n / 2 and same >= n / 3, (name, never, same, n)


# ---- tools/sync_sim.c ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lock_grey_129", "phase_444"])
def test_model_against_sync_sim(port, tmp_path, name):
    """tools/sync_sim.c (written for measurements, from the same rules) gives the same distance for every lane start: -1 for the
    lockstep stream's lanes, the model's bit count for the phase-only stream's."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler for tools/sync_sim.c")
    so = str(tmp_path / "libsyncsim.so")
    subprocess.run([cc, "-O2", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "sync_sim.c")], check=True)
    L = C.CDLL(so)
    L.sim_open.restype = C.c_void_p
    L.sim_open.argtypes = [C.c_void_p, C.c_long] + [C.c_void_p] * 6 + [C.c_int, C.c_int]
    L.sim_close.argtypes = [C.c_void_p]
    L.sim_sync_distance.restype = C.c_long
    L.sim_sync_distance.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long]
    s, m = N.streams()[name], model(name)
    pr = port.parse(s.data)
    info, ecs = pr["info"], np.ascontiguousarray(pr["ecs"])
    assert ecs.tobytes() == m.ecs
    arrs = [np.array(info[k], np.uint8) for k in ("dc_offsets", "dc_symbols", "ac_offsets", "ac_symbols")]
    ids = [np.array(list(info[k]), np.int32) for k in ("comp_dc", "comp_ac")]
    nl = info["hsamp"] * info["vsamp"]
    h = L.sim_open(ecs.ctypes.data, len(ecs), *[a.ctypes.data for a in arrs + ids], nl, nl + info["ncomp"] - 1)
    try:
        truth = m.truth(0, len(ecs))
        n_never = 0
        for q, head in s.lane_starts(128):
            want = m.sync_distance(8 * q, truth, 8 * len(ecs))
            got = L.sim_sync_distance(h, 8 * q, 0, 8 * len(ecs))
            assert got == (-1 if want is None else want), (name, q, got, want)
            n_never += want is None
        if s.cls == 1:
            assert n_never == 62, n_never                 # all but the first lane and lane 63
            byte_model = m.lockstep_distances(128)
            assert [d for _, _, d in byte_model] == [0] + [None] * 62 + [0]      # and the backward pass over bytes says the same
    finally:
        L.sim_close(h)


# ---- intent, port, reference --------------------------------------------------------------------------------------------------------
def _port_applies(s):
    return not (s.fr.standard_restart and s.fr.ri and (s.fr.hs, s.fr.vs) != (1, 1))     # T.81's restart rule: not the reference's


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_intent(port, name):
    s = N.streams()[name]
    if not _port_applies(s):
        assert s.it.status == J.OK                 # the GPU tests decode these against the intent, through the port's back end
        return
    check_port(port, s.data, s.fr, s.it, name)


def test_status_classes_of_the_error_members():
    got = {n: (s.it.status, s.it.err_unit) for n, s in N.streams().items() if s.cls == 5}
    assert got["err_first_wave"][0] == J.AC_SYM and got["err_behind_flag"][0] == J.AC_RUN and got["cut_middle"][0] == J.AC_SYM, got
    S, n_lanes, (a, b) = N.X5
    byte_of = lambda n: N.streams()[n].it.unit_bit[got[n][1]] // 8
    assert byte_of("err_first_wave") < 64 * S                                     # in the first wave
    assert byte_of("err_behind_flag") > 5 * 64 * S                                # behind the start of the sixth wave
    assert a * S < byte_of("cut_middle") < b * S                                  # inside the chain


def test_live_reference_accepts_the_files(port, live_ref, tmp_path):
    """The reference's own scanner and Huffman decoder: same coefficients and verdict as the port for every file."""
    if live_ref is None:
        pytest.skip("oracle/_ref not built")
    for k, (name, s) in enumerate(N.streams().items()):
        jp = tmp_path / f"n{k}.jpg"
        jp.write_bytes(s.data)
        r = live_ref.parse_and_huffman(str(jp))
        o = port.decode(s.data, name=str(jp))
        assert bool(r["info"]["valid"]) and o["valid"], name
        assert bool(r["huff_ok"]) == (o["huff_rc"] == 0), name
        assert np.array_equal(r["coef"], o["coef"]), name
        if _port_applies(s):
            assert o["huff_rc"] == s.it.status, name


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [128, 1024])
def test_planner_takes_every_member_on_the_parallel_path(monkeypatch, S):
    """symbol_corpus.tables_fit / expect_sequential and the planner itself: no member is routed to the exact kernel up front, and the
    planner cuts each into the lanes the model assumes (every S bytes of every restart segment)."""
    import pjd_amd
    for k in ("PJD_PLAN_MODE", "PJD_ODD_WAVE_PCT", "PJD_WALK_MAX"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PJD_SUB_BYTES", str(S))
    for s in N.members(S):
        assert SC.tables_fit(s.fr) and not SC.expect_sequential(s.fr, s.it), s.name
        sc = pjd_amd.Scanned(s.data)
        assert sc.valid, s.name
        sc.desc.flags = pjd_amd.F_STANDARD_RESTART if s.fr.standard_restart else 0
        info = pjd_amd.plan_info([sc.desc])
        assert info["n_sequential"] == 0 and info["sub_bytes"] == S, (s.name, info)
        assert info["n_subsequences"] == s.n_lanes(S), (s.name, info["n_subsequences"], s.n_lanes(S))
        assert info["n_huff_waves"] == -(-s.n_lanes(S) // N.WAVE), s.name
