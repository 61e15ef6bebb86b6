"""The cases of test_gpu_resize.py that need torch, each run in a process of its own:

    python resize_torch_cases.py <case> [arguments]

As tests/planar_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected
pictures are tests/resize_model.py over the box filter of the oracle's picture (for the 1024-picture batch: of this library's
PJD_OUT_RGB8 full-size decode, six of them of the oracle's)."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import ctypes as C                                                # noqa: E402
import os                                                         # noqa: E402
import sys                                                        # noqa: E402

import numpy as np                                                # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle_lib                                                 # noqa: E402
import pjd_amd                                                    # noqa: E402
import synth                                                      # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from conftest import golden_bytes                                 # noqa: E402
from test_gpu_resize import SCALES, expected, target_of, _scanned  # noqa: E402
from test_gpu_planar import GUARD                                 # noqa: E402


def case_resized_batch_tensor():
    port = oracle_lib.Port()
    jpegs = synth.cfg3_imagenet_like(1024, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    c = pjd_amd.Context(0)
    full_sc = [_scanned(j, 0) for j in jpegs]
    descs = [x.desc for x in full_sc]
    assert len({(int(d.width), int(d.height)) for d in descs}) > 1, "the batch is ragged"
    with c.batch(descs) as b:
        b.upload(); b.decode()
        full, st_full = b.download()
    before = [bytes(C.string_at(C.byref(d), C.sizeof(pjd_amd.ImageDesc))) for d in descs]
    t, st = tensors.decode_resized_batch_tensor(c, descs, (224, 224))
    assert [bytes(C.string_at(C.byref(d), C.sizeof(pjd_amd.ImageDesc))) for d in descs] == before
    assert st == st_full
    assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (1024, 3, 224, 224) and t.is_contiguous()
    assert t[5].data_ptr() == t.data_ptr() + 5 * 3 * 224 * 224 and t[5].untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
    host = t.cpu().numpy()
    flags = [tensors.pick_scale_flags(d.width, d.height, 224, 224) for d in descs]
    for i in range(1024):
        assert np.array_equal(host[i], expected(full[i], 1 << (flags[i] >> 4), 224, 224, True)), i
    for i in (0, 1, 2, 3, 513, 1022):
        assert np.array_equal(host[i], expected(port.decode(jpegs[i])["rgb"], 1 << (flags[i] >> 4), 224, 224, True)), i
    # torch computes on the memory
    assert int(t.sum(dtype=torch.int64).item()) == int(host.astype(np.int64).sum())
    # without prescale: the descriptors' own flags hold (here: full size), a non-square target
    t2, st2 = tensors.decode_resized_batch_tensor(c, descs[:48], (96, 160), prescale=False)
    assert st2 == st_full[:48] and tuple(t2.shape) == (48, 3, 96, 160)
    host2 = t2.cpu().numpy()
    for i in range(48):
        assert np.array_equal(host2[i], expected(full[i], 1, 160, 96, True)), i
    c.close()


def case_guard_bytes(fmt, mode):
    ctx = pjd_amd.Context(0)
    port = oracle_lib.Port()
    planar = fmt == "planar"
    out_fmt = pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    names, scanned, sizes, want = [], [], [], []
    k = 0
    for n in GUARD:
        o = port.decode(golden_bytes(n))
        for flags, s in SCALES:
            sc = _scanned(golden_bytes(n), flags | extra)
            sw, sh = pjd_amd.scaled_dims(sc.desc.width, sc.desc.height, flags)
            tw, th = target_of(k, sw, sh)
            if k % 7 == 3:
                tw, th = 261, 9                       # more than one tile across, a ragged last lane
            k += 1
            names.append((n, s, tw, th)); scanned.append(sc); sizes.append((th, tw))
            want.append((o["huff_rc"], expected(o["rgb"], s, tw, th, planar)))
    with ctx.batch([x.desc for x in scanned], out_fmt) as b:
        b.set_resize(sizes)
        offs, pos = [], 1                             # base + 1: nothing is aligned
        for i in range(b.n):
            offs.append(pos)
            pos += b.output_size(i) + 2 * i + 1       # odd gaps
        total = pos + 4096
        buf = torch.full((total + 1,), 0xA5, dtype=torch.uint8, device="cuda:0")
        base = buf[1:]                                # an odd base address as well
        assert base.data_ptr() % 2 == 1
        torch.cuda.synchronize()
        b.bind_output(base.data_ptr(), total, offs)
        assert [b.output_offset(i) for i in range(b.n)] == offs
        b.upload(); b.capture(); b.decode(); b.sync()
        st = b.statuses()
        outs, st_dl = b.download()
        assert st_dl == st
        sizes_b = [b.output_size(i) for i in range(b.n)]
        host = base.cpu().numpy()
        covered = np.zeros(total, bool)
        for i, (nm, (wst, wpic)) in enumerate(zip(names, want)):
            assert st[i] == wst, nm
            assert sizes_b[i] == wpic.size
            assert np.array_equal(host[offs[i]:offs[i] + sizes_b[i]], wpic.reshape(-1)), nm
            assert np.array_equal(outs[i], wpic), nm
            covered[offs[i]:offs[i] + sizes_b[i]] = True
        stray = np.flatnonzero(~covered & (host != 0xA5))
        assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"
        assert int(buf[0].item()) == 0xA5
        # every decode writes every byte of every range: two different fill patterns, the graph replayed after each
        for pattern in (0x3C, 0xC3):
            buf.fill_(pattern)
            torch.cuda.synchronize()
            b.decode(); b.sync()
            host = base.cpu().numpy()
            for i, (nm, (wst, wpic)) in enumerate(zip(names, want)):
                assert np.array_equal(host[offs[i]:offs[i] + sizes_b[i]], wpic.reshape(-1)), (nm, pattern)
            assert np.all(host[~covered] == pattern)
    ctx.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
