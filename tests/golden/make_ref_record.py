#!/usr/bin/env python3
"""Generate tests/golden/ref_record.json: what the reference's own code (oracle/_ref) answers on the fixtures, so that
the tests which pin the oracle port to it run where the reference tree is absent.  Run where oracle/_ref can be built,
like make_fixtures.py:  python tests/golden/make_ref_record.py

fixtures: name -> oracle_lib.ref_digest of read_JPEG's result, or null where read_JPEG rejects the file
synth:    key of test_synth.synth_cases() -> [sha256 of the JPEG, sha256 of the reference CLI's BMP]
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402
import test_synth  # noqa: E402


def main():
    oracle_lib.build_oracle()
    ref = oracle_lib.Ref()
    names = sorted(json.load(open(os.path.join(HERE, "manifest.json"))))
    fixtures, synth = {}, {}
    tmp = tempfile.mkdtemp()
    try:
        for name in names:
            r = ref.parse_and_huffman(shutil.copy(os.path.join(HERE, name + ".jpg"), tmp))
            fixtures[name] = oracle_lib.ref_digest(r) if r["info"]["valid"] else None
        for key, data in test_synth.synth_cases():
            jp, bp = os.path.join(tmp, key + ".jpg"), os.path.join(tmp, key + ".bmp")
            with open(jp, "wb") as f:
                f.write(data)
            assert ref.run_cli(jp, bp) == (0, "")
            synth[key] = [hashlib.sha256(data).hexdigest(), hashlib.sha256(open(bp, "rb").read()).hexdigest()]
    finally:
        shutil.rmtree(tmp)
    with open(os.path.join(HERE, "ref_record.json"), "w") as f:       # one entry per line
        f.write('{"fixtures": {\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in fixtures.items()) + '},\n')
        f.write('"synth": {\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in synth.items()) + "}}\n")
    print(f"{len(fixtures)} fixtures, {len(synth)} synthetic pictures recorded")


if __name__ == "__main__":
    main()
