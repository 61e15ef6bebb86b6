#!/usr/bin/env python3
"""Write tests/golden/progressive/: the committed hand-built progressive files (prog_*.jpg, progressive_corpus.FIXTURES) and
ref_record.json -- what the reference's own decode_MCU_component (oracle/_ref, driven one scan at a time by oracle/ref_driver.cpp)
answered on every stream of the fixtures, the seeded corpus, the broken streams and the big picture, so that the test which pins the
model to it runs where the reference tree is absent.  Run where oracle/_ref can be built:

    python tests/golden/make_progressive_record.py

ref_record.json: label -> [sha256 of the coefficient buffer (n_units x 64 int16, the reference's natural order), erring scan or -1,
good blocks of the last scan run, the reference's message]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "pim-jpeg-decoder_amd", "python"))
import oracle_lib  # noqa: E402
import jpeg_progressive as P  # noqa: E402
import progressive_corpus as PC  # noqa: E402
import test_progressive_streams as T  # noqa: E402


def main():
    oracle_lib.build_oracle()
    ref = oracle_lib.Ref()
    out = os.path.join(HERE, "progressive")
    os.makedirs(out, exist_ok=True)
    for name in PC.FIXTURES:
        with open(os.path.join(out, name + ".jpg"), "wb") as f:
            f.write(PC.named()[name].data)
    rec = {}
    for label, data in T.all_streams():
        coef, err_scan, good, msg = T.reference_answer(ref, P.decode(data, zigzag="reference"))
        rec[label] = [T.digest(coef), err_scan, good, msg]
    with open(os.path.join(out, "ref_record.json"), "w") as f:       # one entry per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items()) + "}\n")
    print(f"{len(PC.FIXTURES)} fixtures written, {len(rec)} streams recorded")


if __name__ == "__main__":
    main()
