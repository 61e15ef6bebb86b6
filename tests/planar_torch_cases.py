"""The cases of test_gpu_planar.py that need torch, each run in a process of its own:

    python planar_torch_cases.py <case> [arguments]

torch brings its own HIP runtime, and torch and libpjd.so use ONE runtime -- so that a tensor's data_ptr() means something to the
library -- only if torch is loaded first: this file imports torch, and touches the device with it, before anything of pjd_amd.
Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected pictures come from the oracle
(or, for the 1024-picture batch, from this library's PJD_OUT_RGB8 full-size decode), as in test_gpu_planar.py."""
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
from test_gpu_scaled import box                                   # noqa: E402
from test_gpu_planar import GUARD, SCALES, E_ARG, E_STATE, chw, _scanned   # noqa: E402


def raises(exc, pattern, fn):
    try:
        fn()
    except exc as e:
        assert pattern in str(e), str(e)
        return
    raise AssertionError(f"{exc.__name__} not raised")


def oracle_of(port, names):
    out = {}
    for n in names:
        o = port.decode(golden_bytes(n))
        out[n] = (o["huff_rc"], o["rgb"])
    return out


def case_cfg3_bound(plan_mode):
    plan_mode = int(plan_mode)
    port = oracle_lib.Port()
    jpegs = synth.cfg3_imagenet_like(1024, seed=3, detail=synth.DENSE_DETAIL, optimize=True, quality_shift=True)
    c = pjd_amd.Context(0, plan_mode=plan_mode)
    try:
        full_sc = [_scanned(j, 0) for j in jpegs]
        with c.batch([x.desc for x in full_sc]) as b:
            b.upload(); b.decode()
            full, st_full = b.download()
            fb_full = b.info()["n_fallback"]
        scales = [1, 2, 4, 8]
        flag_of = {1: 0, 2: 16, 4: 32, 8: 48}
        sc = [_scanned(j, flag_of[scales[i % 4]]) for i, j in enumerate(jpegs)]
        want = [chw(full[i], scales[i % 4]) for i in range(1024)]
        with c.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
            size = b.packed_size()
            buf = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            offs = [b.output_offset(i) for i in range(1024)]
            b.bind_output(buf.data_ptr(), size)
            assert [b.output_offset(i) for i in range(1024)] == offs and b.device_output(0) == buf.data_ptr() + offs[0]
            b.upload(); b.capture()
            b.decode(); b.sync()
            st = b.statuses()
            info = b.info()
            host = buf.cpu().numpy()
            assert st == st_full and info["n_fallback"] == fb_full and info["plan_mode"] == plan_mode
            for i in range(1024):
                assert np.array_equal(host[offs[i]:offs[i] + want[i].size], want[i].reshape(-1)), i
            for i in (0, 1, 2, 3, 513, 1022):
                assert np.array_equal(host[offs[i]:offs[i] + want[i].size], chw(port.decode(jpegs[i])["rgb"], scales[i % 4]).reshape(-1)), i
            buf.fill_(0xA5)
            torch.cuda.synchronize()
            b.decode(); b.decode(); b.sync()
            assert b.statuses() == st_full
            host = buf.cpu().numpy()
            for i in range(1024):
                assert np.array_equal(host[offs[i]:offs[i] + want[i].size], want[i].reshape(-1)), i
            packed, st3 = b.download_packed()
            assert st3 == st_full
            for i in (0, 5, 1023):
                assert np.array_equal(packed[i], want[i].reshape(-1)), i
        tens, st64 = tensors.decode_to_tensors(c, [x.desc for x in sc[:64]])
        assert st64 == st_full[:64]
        for i, t in enumerate(tens):
            assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == want[i].shape
            assert np.array_equal(t.cpu().numpy(), want[i]), i
        tens, _ = tensors.decode_to_tensors(c, [x.desc for x in sc[:8]], planar=False)
        for i, t in enumerate(tens):
            assert np.array_equal(t.cpu().numpy(), box(full[i], scales[i % 4])), i
    finally:
        c.close()


def case_guard_bytes(fmt, mode):
    ctx = pjd_amd.Context(0)
    oracle = oracle_of(oracle_lib.Port(), GUARD)
    out_fmt = pjd_amd.OUT_RGB8_PLANAR if fmt == "planar" else pjd_amd.OUT_RGB8
    extra = pjd_amd.F_FORCE_SEQUENTIAL if mode == "exact" else 0
    names, scanned = [], []
    for n in GUARD:
        for flags, s in SCALES:
            names.append((n, s))
            scanned.append(_scanned(golden_bytes(n), flags | extra))
    with ctx.batch([x.desc for x in scanned], out_fmt) as b:
        offs, pos = [], 37
        for i in range(b.n):
            offs.append(pos)
            pos += b.output_size(i) + 2 * i + 1
        total = pos + 4096
        buf = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        b.bind_output(buf.data_ptr(), total, offs)
        assert [b.output_offset(i) for i in range(b.n)] == offs
        b.upload(); b.decode(); b.sync()
        st = b.statuses()
        outs, st_dl = b.download()                      # copies from the bound addresses
        assert st_dl == st
        raises(pjd_amd.PjdError, "(-5)", b.download_packed)     # explicit offsets: no packed layout
        sizes = [b.output_size(i) for i in range(b.n)]
    host = buf.cpu().numpy()
    covered = np.zeros(total, bool)
    for i, ((n, s), status) in enumerate(zip(names, st)):
        want = chw(oracle[n][1], s) if fmt == "planar" else box(oracle[n][1], s)
        assert status == oracle[n][0], (n, s)
        assert sizes[i] == want.size
        assert np.array_equal(host[offs[i]:offs[i] + sizes[i]], want.reshape(-1)), (n, s)
        assert np.array_equal(outs[i], want), (n, s)
        covered[offs[i]:offs[i] + sizes[i]] = True
    stray = np.flatnonzero(~covered & (host != 0xA5))
    assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"
    ctx.close()


def case_batch_tensor():
    ctx = pjd_amd.Context(0)
    port = oracle_lib.Port()
    w, h = 203, 157                                      # 4:2:0, width not a multiple of 16
    jpegs = [synth.make(w, h, 9000 + k, 90, synth.SUB_420, 0, synth.DENSE_DETAIL, True) for k in range(64)]
    sc = [_scanned(j, 0) for j in jpegs]
    t, st = tensors.decode_to_batch_tensor(ctx, [x.desc for x in sc])
    assert st == [0] * 64
    assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (64, 3, h, w) and t.is_contiguous()
    want = np.stack([chw(port.decode(j)["rgb"]) for j in jpegs])
    assert np.array_equal(t.cpu().numpy(), want)
    # the memory is torch's: torch computes on it.  The integer sum is exact; the float32 mean of 6.1 M values is a tree of
    # additions in torch (error <= log2(N) x 2^-24 ~ 1.4e-6 relative), compared to within 1e-5
    assert int(t.sum(dtype=torch.int64).item()) == int(want.astype(np.int64).sum())
    mean_dev, mean_host = float(t.float().mean().item()), float(want.astype(np.float64).mean())
    print("mean on the device", mean_dev, "on the host", mean_host)
    assert abs(mean_dev - mean_host) <= 1e-5 * mean_host
    half = [_scanned(j, pjd_amd.F_SCALE_1_2) for j in jpegs[:4]]
    t2, _ = tensors.decode_to_batch_tensor(ctx, [x.desc for x in half])
    assert tuple(t2.shape) == (4, 3, -(-h // 2), -(-w // 2))
    assert np.array_equal(t2.cpu().numpy(), np.stack([chw(port.decode(j)["rgb"], 2) for j in jpegs[:4]]))
    raises(ValueError, "uniform_output_shape", lambda: tensors.decode_to_batch_tensor(ctx, [sc[0].desc, half[0].desc]))
    ctx.close()


def case_stream_order():
    """tensors.py orders torch's stream before the library's writes: tensors of one call are dropped while work queued on torch's
    stream has not read them yet, the next call gets the same block from torch's caching allocator, and the queued work must still
    see the first call's pictures."""
    ctx = pjd_amd.Context(0)
    w, h = 203, 157
    first = [_scanned(synth.make(w, h, 9000 + k, 90, synth.SUB_420, 0, synth.DENSE_DETAIL, True), 0) for k in range(64)]
    second = [_scanned(synth.make(w, h, 9500 + k, 90, synth.SUB_420, 0, synth.DENSE_DETAIL, True), 0) for k in range(64)]
    t1, st = tensors.decode_to_batch_tensor(ctx, [x.desc for x in first])
    assert st == [0] * 64
    want = t1.cpu().numpy().astype(np.int64).sum(axis=(1, 2, 3))          # the pictures themselves are checked in case_batch_tensor
    ptr = t1.data_ptr()
    busy = torch.randn(8192, 8192, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(24):                                                   # some tenths of a second of work on torch's stream ...
        busy = (busy @ busy) * 1e-4
    sums = t1.sum(dim=(1, 2, 3), dtype=torch.int64)                       # ... and behind it the reader of the first pictures
    del t1
    t2, st = tensors.decode_to_batch_tensor(ctx, [x.desc for x in second])
    assert st == [0] * 64
    assert t2.data_ptr() == ptr, "the allocator did not hand the block back: this case exercised nothing"
    assert np.array_equal(sums.cpu().numpy(), want), "the second decode overwrote pictures that queued torch work had not read yet"
    assert not np.array_equal(t2.cpu().numpy().astype(np.int64).sum(axis=(1, 2, 3)), want)
    ctx.close()


def case_bind_errors():
    ctx = pjd_amd.Context(0)
    oracle = oracle_of(oracle_lib.Port(), ["env_61x45_420_q100_opt", "gray_33x70", "rst4_128x96_444"])
    L = pjd_amd.dev_lib()
    names = ["env_61x45_420_q100_opt", "gray_33x70", "rst4_128x96_444"]
    sc = [_scanned(golden_bytes(n), 0) for n in names]
    descs = [x.desc for x in sc]
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ptr, cap = C.c_void_p(buf.data_ptr()), 1 << 20

    def offsets(v):
        return (C.c_uint64 * len(v))(*v)

    with ctx.batch(descs, pjd_amd.OUT_BMP) as b:
        assert L.pjd_batch_bind_output(b._h, ptr, cap, None) == E_ARG                     # a BMP batch
        b.upload(); b.decode()                                                             # ... which still decodes into its own buffer
        outs, st = b.download()
        for n, o, s in zip(names, outs, st):
            assert s == oracle[n][0] and np.array_equal(o, np.frombuffer(pjd_amd.rgb_to_bmp(oracle[n][1]), np.uint8)), n
    for fmt in (pjd_amd.OUT_RGB8_PLANAR, pjd_amd.OUT_RGB8):
        with ctx.batch(descs, fmt) as b:
            sizes = [b.output_size(i) for i in range(3)]
            last_end = b.output_offset(2) + sizes[2]
            assert L.pjd_batch_bind_output(None, ptr, cap, None) == E_ARG
            assert L.pjd_batch_bind_output(b._h, None, cap, None) == E_ARG
            assert L.pjd_batch_bind_output(b._h, ptr, last_end - 1, None) == E_ARG        # short capacity, packed layout
            assert L.pjd_batch_bind_output(b._h, ptr, 1 << 30, None) == E_ARG             # a capacity the 1 MiB allocation does not hold
            assert L.pjd_batch_bind_output(b._h, ptr, cap, offsets([0, sizes[0], cap - sizes[2] + 1])) == E_ARG   # ends beyond
            assert L.pjd_batch_bind_output(b._h, ptr, cap, offsets([0, sizes[0] - 1, 500000])) == E_ARG           # overlap by one byte
            assert L.pjd_batch_bind_output(b._h, ptr, cap, offsets([500000, 0, 500000 + sizes[0] - 1])) == E_ARG  # overlap, unsorted
            host = np.zeros(1 << 20, np.uint8)
            assert L.pjd_batch_bind_output(b._h, C.c_void_p(host.ctypes.data), cap, None) == E_ARG   # pageable host memory
            pinned = L.pjd_host_alloc(1 << 20)
            try:
                assert L.pjd_batch_bind_output(b._h, C.c_void_p(pinned), cap, None) == E_ARG      # page-locked host memory
            finally:
                L.pjd_host_free(pinned)
            # every refusal left the batch as it was: it decodes into its own buffer
            b.upload(); b.decode()
            outs, st = b.download()
            for n, o, s in zip(names, outs, st):
                want = chw(oracle[n][1]) if fmt == pjd_amd.OUT_RGB8_PLANAR else oracle[n][1]
                assert s == oracle[n][0] and np.array_equal(o, want), n
            assert L.pjd_batch_bind_output(b._h, ptr, cap, None) == E_STATE                 # after upload
    # exactly enough: the capacity ends with the last picture
    with ctx.batch(descs, pjd_amd.OUT_RGB8_PLANAR) as b:
        last_end = b.output_offset(2) + b.output_size(2)
        b.bind_output(buf.data_ptr(), last_end)
        b.upload(); b.decode()
        outs, st = b.download()
        packed, _ = b.download_packed()
        for n, o, p in zip(names, outs, packed):
            assert np.array_equal(o, chw(oracle[n][1])) and np.array_equal(p, o.reshape(-1)), n
    ctx.close()


def case_device_bytes():
    ctx = pjd_amd.Context(0)
    sc = [_scanned(golden_bytes(n), 0) for n in ("big_640x480_420_q85", "ilsvrc_val_00000001")]
    with ctx.batch([x.desc for x in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        own = b.info()["device_bytes"]
        size = b.packed_size()
        buf = torch.empty(size, dtype=torch.uint8, device="cuda:0")
        b.bind_output(buf.data_ptr(), size)
        assert b.info()["device_bytes"] == own - size
        b.bind_output(buf.data_ptr(), size)              # binding again (before upload) gives nothing back twice
        assert b.info()["device_bytes"] == own - size
    ctx.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
