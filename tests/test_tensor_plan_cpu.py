"""pjd_amd.tensors against a record of its own past (no GPU): tests/golden/tensor_plan_calls.json holds, per case of a matrix of the
keywords of the four public helpers, a digest of everything the helper handed to the batch -- the descriptors, the output format, every
Batch call in order with its arguments, the result's shape, strides and dtype -- or of the fact that it refused with nothing created.
The matrix and the recorder are tests/golden/make_tensor_plan_calls.py, which made the file; here it is replayed and compared."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_tensor_plan_calls as mk  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(mk.OUT) as f:
        return json.load(f)


def _keywords(key):
    return dict(kv.split("=") for kv in key.split(" "))


def test_the_fixture_covers_what_it_must(recorded):
    """At least half of the cases succeed; every value of every keyword occurs in a succeeding case; every refusal that the planner must
    keep occurs in a failing one; the fixture is the matrix of the generator, case for case."""
    assert [r[0] for r in recorded] == [mk.key(kw) for kw in mk.cases()]
    ok = [_keywords(key) for key, good, _ in recorded if good]
    bad = [_keywords(key) for key, good, _ in recorded if not good]
    assert 2 * len(ok) >= len(recorded), (len(ok), len(recorded))
    domains = dict(mk.PLAN, **mk.TAIL)
    domains.update(planar=["0", "1"], fn=mk.TAIL["fn"] + ["tensors", "batch"], ps=mk.PLAN["ps"] + ["draft2", "draft4", "draft8"])
    for name, values in domains.items():
        for v in values:
            assert any(kw.get(name) == v for kw in ok), f"no succeeding case has {name}={v}"
    for name in mk.REFUSALS:
        assert any(kw.get("extra") == name for kw in bad), f"no failing case for {name}"
    assert any(kw.get("lb") in ("center", "topleft") and kw.get("rs") == "64" for kw in bad)
    assert any(kw.get("c") == "all" and kw.get("rs") == "64" and kw.get("lb") == "none" for kw in bad)


def test_every_case_hands_the_batch_what_it_did(recorded):
    """The replay: every case's record has the digest of the fixture.  A case that differs is printed with its keywords and what the
    helper does now."""
    pytest.importorskip("torch")
    wrong = []
    for kw, (key, good, want) in zip(mk.cases(), recorded):
        rec = mk.run_case(kw)
        if "raises" in rec:
            assert rec["raises"] == "ValueError" and not rec["calls"] and not rec["batches"], (key, rec)
        if ("raises" not in rec, mk.digest(rec)) != (good, want):
            wrong.append(key)
            if len(wrong) <= 5:
                print(f"{key}\n  recorded: {'succeeds' if good else 'raises'}, {want}\n  now: {json.dumps(rec)}")
    assert not wrong, f"{len(wrong)} of {len(recorded)} cases differ from tests/golden/tensor_plan_calls.json: {wrong[:20]}"
