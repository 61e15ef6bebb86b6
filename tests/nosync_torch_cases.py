"""The case of test_gpu_nosync.py that needs torch, run in a process of its own:

    python nosync_torch_cases.py bound_planar

torch is loaded, and touches the device, before anything of pjd_amd, so that both use one HIP runtime (as planar_torch_cases.py).
Prints "CASE OK <case>" at the end; a failed assertion ends the process with a traceback."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import os                                                         # noqa: E402
import sys                                                        # noqa: E402

import numpy as np                                                # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pim-jpeg-decoder_amd", "python"))

import nosync_corpus as N                                         # noqa: E402
import pjd_amd                                                    # noqa: E402

DOWNSTREAM = ["phase_420_big", "chain_x5"]


def case_bound_planar():
    """A 4:2:0 and a grey picture that the parallel decoder gives up on, planar, into a tensor filled with 0x5A: the same bytes as
    with PJD_F_FORCE_SEQUENTIAL, picture by picture, and the gaps between the pictures untouched."""
    os.environ["PJD_SUB_BYTES"] = "128"
    os.environ.pop("PJD_WALK_MAX", None)                          # the planner's own walker threshold: the route asserted below
    ctx = pjd_amd.Context(0)
    try:
        got = []
        for force in (0, pjd_amd.F_FORCE_SEQUENTIAL):
            sc = []
            for n in DOWNSTREAM:
                s = pjd_amd.Scanned(N.streams()[n].data)
                s.desc.flags = force
                sc.append(s)
            with ctx.batch([s.desc for s in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
                size = b.packed_size()
                buf = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                b.bind_output(buf.data_ptr(), size)
                b.upload(); b.decode(); b.sync()
                assert b.statuses() == [0, 0]
                info = b.info()
                assert (info["n_fallback"], info["n_sequential"]) == ((0, 2) if force else (2, 0)), info
                spans = [(b.output_offset(i), b.output_size(i)) for i in range(2)]
                got.append((buf.cpu().numpy(), spans))
        (a, spans), (f, spans_f) = got
        assert spans == spans_f and np.array_equal(a, f)
        used = np.zeros(a.size, bool)
        for off, n in spans:
            used[off:off + n] = True
            fr = N.streams()[DOWNSTREAM[spans.index((off, n))]].fr
            assert n == 3 * fr.width * fr.height
        assert (a[~used] == 0x5A).all() and not (a[used] == 0x5A).all()
    finally:
        ctx.close()


if __name__ == "__main__":
    {"bound_planar": case_bound_planar}[sys.argv[1]]()
    print("CASE OK", sys.argv[1])
