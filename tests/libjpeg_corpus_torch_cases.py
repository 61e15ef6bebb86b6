"""The case of test_gpu_libjpeg_corpus.py that needs torch, run in a process of its own:

    python libjpeg_corpus_torch_cases.py <case>

As tests/libjpeg_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  The expected
picture is libjpeg_corpus.expected: the model over the oracle port's coefficients."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import os                                                         # noqa: E402
import sys                                                        # noqa: E402

import numpy as np                                                # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))

import libjpeg_corpus as LC                                       # noqa: E402
import oracle_lib                                                 # noqa: E402
import pjd_amd                                                    # noqa: E402

GUARD = 4096


def case_bound_output_wide():
    """The 65535-wide 4:2:0 member beside a 7 x 2 one, flagged, planar and interleaved, bound at base + 1 (no picture starts aligned;
    an odd gap between the two) in a buffer of 0xA5: the pictures are the model's, every other byte is still 0xA5 -- the tail store of
    the colour kernel (65535 % 4 == 3) writes three bytes, not four."""
    names = [LC.WIDE_420, "e7x2_420"]
    port = oracle_lib.Port()
    want = []
    for n in names:
        status, rgb = LC.expected(port, LC.model_bytes(n))
        assert status == 0
        want.append(rgb)
    c = pjd_amd.Context(0)
    n_checked = 0
    for fmt in (pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_RGB8):
        scanned = [pjd_amd.Scanned(LC.jpeg(n)) for n in names]
        for s in scanned:
            assert s.valid
            s.desc.flags = int(s.desc.flags) | pjd_amd.F_LIBJPEG
        with c.batch([s.desc for s in scanned], fmt) as b:
            offs, pos = [], 1
            for i in range(b.n):
                offs.append(pos)
                pos += b.output_size(i) + 2 * i + 1
            total = pos + GUARD
            buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert buf.data_ptr() % 4 == 0
            b.bind_output(buf.data_ptr(), total, offs)
            b.upload()
            b.decode(); b.sync()
            assert b.statuses() == [0] * b.n
            host = buf.cpu().numpy()
            covered = np.zeros(total, bool)
            for i, n in enumerate(names):
                w = np.ascontiguousarray(want[i].transpose(2, 0, 1)) if fmt == pjd_amd.OUT_RGB8_PLANAR else want[i]
                assert b.output_size(i) == w.size, n
                got = host[offs[i]:offs[i] + w.size]
                bad = np.flatnonzero(got != w.reshape(-1))
                assert bad.size == 0, (fmt, n, "first differing byte", int(bad[0]), "differing", int(bad.size))
                covered[offs[i]:offs[i] + w.size] = True
                n_checked += 1
            assert not covered[0] and not covered[offs[1] - 1] and not covered[-GUARD:].any()
            stray = np.flatnonzero(~covered & (host != 0xA5))
            assert stray.size == 0, (fmt, "bytes outside every picture were written, first at", stray[:8].tolist(), offs)
    c.close()
    assert n_checked == 4


if __name__ == "__main__":
    case = sys.argv[1]
    {"bound_output_wide": case_bound_output_wide}[case]()
    print(f"CASE OK {case}")
