"""Seeded damaged streams that more than one GPU test module decodes (tests/test_gpu_parity.py, tests/test_gpu_poisoned_memory.py):
built once per process, never changed by a test."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _synth():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import synth
    return synth


@functools.lru_cache(maxsize=None)
def corrupted_streams(n=200):
    """n seeded pictures (8..300 px per side, every sampling, restart intervals 0, 3 and 11) with 1-3 bytes of the second half of the
    file overwritten in place.  The first k of corrupted_streams(n) are corrupted_streams(k)."""
    synth = _synth()
    rng = np.random.default_rng(4242)
    jpegs = []
    for k in range(n):
        w, h = int(rng.integers(8, 301)), int(rng.integers(8, 301))
        sub = int(rng.choice([synth.SUB_444, synth.SUB_422, synth.SUB_420, synth.SUB_440, synth.SUB_GREY]))
        ri = int(rng.choice([0, 0, 3, 11]))
        ba = bytearray(synth.make(w, h, 5000 + k, int(rng.choice([25, 75, 95])), sub, ri, float(rng.choice([1.0, synth.DENSE_DETAIL])), bool(k & 1)))
        for _ in range(int(rng.integers(1, 4))):
            ba[int(rng.integers(len(ba) // 2, len(ba) - 2))] = int(rng.integers(0, 256))
        jpegs.append(bytes(ba))
    return tuple(jpegs)


@functools.lru_cache(maxsize=1)
def runon_error_streams():
    """16 one-bits (no table assigns that code) planted 2 and 5 bytes before every 128-byte boundary of the entropy-coded segment of a
    dense 200 x 152 4:2:0 picture: an error in a unit's AC part, right before the lane behind it begins (at PJD_SUB_BYTES=128)."""
    synth = _synth()
    good = synth.make(200, 152, 77, 95, synth.SUB_420, 0, synth.DENSE_DETAIL, True)
    body = good.rfind(b"\xff\xda") + 14
    end = len(good) - 2
    file_pos, i = [], body                    # file offset of every destuffed byte of the entropy-coded segment
    while i < end:
        file_pos.append(i)
        i += 2 if good[i] == 0xFF else 1
    jpegs = []
    for k in range(1, len(file_pos) // 128):
        for r in (2, 5):
            f = file_pos[k * 128 - r - 2]
            if 0xFF in good[f - 1:f + 5]:
                continue
            jpegs.append(good[:f] + b"\xff\x00\xff\x00" + good[f + 4:])
    return tuple(jpegs)
