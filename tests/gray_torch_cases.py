"""The cases of test_gpu_gray.py that need torch, each run in a process of its own:

    python gray_torch_cases.py <case>

As tests/libjpeg_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected planes are
those of tests/gray_expected.py: the oracle with neutral chroma, Pillow's recorded draft("L") decode."""
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

import gray_expected as G                                         # noqa: E402
import oracle_lib                                                 # noqa: E402
import pjd_amd                                                    # noqa: E402
from gray_expected import golden_bytes                            # noqa: E402
from pjd_amd import tensors                                       # noqa: E402

PORT = oracle_lib.Port()
# widths 3, 4, 5, 17, 33 and 61: (file bytes, libjpeg fixture name or None)
WIDTHS = [("lj_3x5_420_q90", True), ("lj_4x9_422_q90", True), ("lj_5x4_420_q90", True), ("env_17x9_420_q100", False),
          ("lj_17x17_420_q90", True), ("gray_33x70", False), ("lj_33x31_420_q100", True), ("env_61x45_420_q100_opt", False),
          ("lj_61x45_grey_q50", True), ("env_61x45_444_q85_opt", False), ("h1v2_45x61", False)]


def _bytes(name, lj):
    return G.lj_bytes(name) if lj else golden_bytes(name)


def case_bound_canaries():
    """Every picture of WIDTHS unflagged at the four scales and, where it is a libjpeg fixture, flagged at full size; the whole list once
    on the parallel path and once with PJD_F_FORCE_SEQUENTIAL, in ONE batch bound at an odd address with odd gaps."""
    items, want = [], []
    for extra in (0, pjd_amd.F_FORCE_SEQUENTIAL):
        for name, lj in WIDTHS:
            data = _bytes(name, lj)
            st, plane = G.ref_plane(PORT, data)
            for flags, s in [(0, 1), (16, 2), (32, 4), (48, 8)]:
                items.append((data, flags | extra)); want.append((st, G.box1(plane, s)))
            if lj:
                items.append((data, pjd_amd.F_LIBJPEG | extra)); want.append((0, G.l8(name)))
    assert {w.shape[1] for _, w in want} >= {3, 4, 5, 17, 33, 61}
    scanned = []
    for data, flags in items:
        s = pjd_amd.Scanned(data)
        assert s.valid
        s.desc.flags = int(s.desc.flags) | flags
        scanned.append(s)
    sizes = [w.size for _, w in want]
    offsets, pos = [], 37
    for k, n in enumerate(sizes):
        offsets.append(pos)
        pos += n + 1 + 2 * (k % 7)                                 # odd gaps: 1, 3, 5, ...
    cap = pos + 64
    buf = torch.empty(cap + 2, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr() + (1 if buf.data_ptr() % 2 == 0 else 0)  # an odd device address
    view = buf[base - buf.data_ptr(): base - buf.data_ptr() + cap]
    assert base % 2 == 1 and any((base + o) % 4 for o in offsets)
    c = pjd_amd.Context(0)
    with c.batch([s.desc for s in scanned], pjd_amd.OUT_GRAY8) as b:
        assert [b.output_size(i) for i in range(b.n)] == sizes
        own = b.info()["device_bytes"]
        b.bind_output(base, cap, offsets)
        assert b.info()["device_bytes"] < own                     # the batch's own output buffer went back to the pool
        b.upload()
        inside = np.zeros(cap, bool)
        for o, n in zip(offsets, sizes):
            inside[o:o + n] = True
        for canary in (0xC3, 0x3C):
            buf.fill_(canary)
            torch.cuda.synchronize()
            b.decode(); b.sync()
            st = b.statuses()
            host = view.cpu().numpy()
            assert (host[~inside] == canary).all(), ("a byte outside the picture ranges was written", canary)
            for k, ((status, w), o) in enumerate(zip(want, offsets)):
                assert st[k] == status, k
                assert np.array_equal(host[o:o + w.size], w.reshape(-1)), (k, canary, w.shape)
        info = b.info()
        assert info["n_fallback"] == 0 and info["n_sequential"] == len(items) // 2, info
    c.close()
    print("poison", os.environ.get("PJD_DEBUG_POISON"))


def case_tensors():
    names = ["env_61x45_420_q100_opt", "gray_33x70", "h1v2_48x64", "env_17x9_444_q85"]
    scanned = [pjd_amd.Scanned(golden_bytes(n)) for n in names]
    descs = [s.desc for s in scanned]
    c = pjd_amd.Context(0)
    outs, st = tensors.decode_to_tensors(c, descs, gray=True)
    for n, d, t, status in zip(names, descs, outs, st):
        want_st, want = G.ref_plane(PORT, golden_bytes(n))
        assert status == want_st and t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (1, d.height, d.width), n
        assert np.array_equal(t.cpu().numpy()[0], want), n
    # scaled descriptors: views at the output scale
    s4 = pjd_amd.Scanned(golden_bytes(names[0]))
    s4.desc.flags = int(s4.desc.flags) | pjd_amd.F_SCALE_1_4
    outs, st = tensors.decode_to_tensors(c, [s4.desc], gray=True)
    assert tuple(outs[0].shape) == (1, 12, 16)
    assert np.array_equal(outs[0].cpu().numpy()[0], G.box1(G.ref_plane(PORT, golden_bytes(names[0]))[1], 4))
    # libjpeg=True: libjpeg's luma; the caller's descriptors keep their flags
    lj = ["lj_136x72_420_q90", "lj_136x72_420_q90_rst4"]
    sl = [pjd_amd.Scanned(G.lj_bytes(n)) for n in lj]
    outs, st = tensors.decode_to_tensors(c, [s.desc for s in sl], libjpeg=True, gray=True)
    assert st == [0, 0] and all(np.array_equal(t.cpu().numpy()[0], G.l8(n)) for t, n in zip(outs, lj))
    assert all(not (int(s.desc.flags) & pjd_amd.F_LIBJPEG) for s in sl)
    t, st = tensors.decode_to_batch_tensor(c, [s.desc for s in sl], libjpeg=True, gray=True)
    assert st == [0, 0] and tuple(t.shape) == (2, 1, 72, 136) and t.dtype == torch.uint8 and t.is_contiguous()
    assert all(np.array_equal(t[i, 0].cpu().numpy(), G.l8(n)) for i, n in enumerate(lj))
    t, st = tensors.decode_to_batch_tensor(c, [s.desc for s in sl], gray=True)
    assert tuple(t.shape) == (2, 1, 72, 136)
    assert all(np.array_equal(t[i, 0].cpu().numpy(), G.ref_plane(PORT, G.lj_bytes(n))[1]) for i, n in enumerate(lj))
    assert not np.array_equal(t[0, 0].cpu().numpy(), G.l8(lj[0]))             # the two arithmetics differ
    # without the keyword nothing changed
    t3, _ = tensors.decode_to_batch_tensor(c, [s.desc for s in sl])
    assert tuple(t3.shape) == (2, 3, 72, 136)
    c.close()


def case_misaligned_bind():
    """A normalised grey batch bound at an address that is no multiple of the element size: PJD_E_ARG, the picture named; the same batch
    bound at an aligned address (not 8- or 16-byte aligned: element alignment is all that is promised) decodes right."""
    import normalize_model as nm
    import resize_pad_model as pm
    name = "env_61x45_420_q100_opt"
    plane = G.ref_plane(PORT, golden_bytes(name))[1]
    scale, bias = [1 / 255.0] * 3, [-0.5] * 3
    c = pjd_amd.Context(0)
    for dt, es, tdt in ((pjd_amd.DT_F16, 2, torch.float16), (pjd_amd.DT_F32, 4, torch.float32)):
        s = pjd_amd.Scanned(golden_bytes(name))
        with c.batch([s.desc], pjd_amd.OUT_GRAY8) as b:
            b.set_resize([(9, 13)])
            b.set_normalize(dt, scale, bias)
            n = b.output_size(0)
            assert n == 9 * 13 * es
            buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for off in range(1, es):
                try:
                    b.bind_output(buf.data_ptr() + off, n, [0])
                    raise AssertionError("a misaligned bind was accepted")
                except pjd_amd.PjdError as e:
                    assert "(-3)" in str(e) and "picture 0" in str(e) and "element size" in str(e), str(e)
            b.bind_output(buf.data_ptr() + es, n, [0])
            b.upload(); b.decode(); b.sync()
            assert b.statuses() == [0]
            got = buf[es:es + n].view(tdt).view(9, 13).cpu().numpy()
            C = pm.padded(np.repeat(plane[:, :, None], 3, axis=2), None, 13, 9, (0, 0, 0, 0))
            want = nm.normalize(C, dt, np.float32(scale), np.float32(bias))[..., 0]
            assert np.array_equal(nm.bits(got), nm.bits(want)), dt
            assert (buf[:es] == 0).all() and (buf[es + n:] == 0).all()
    c.close()


def case_resized_tensors():
    import normalize_model as nm
    import resize_pad_model as pm
    names = ["env_61x45_420_q100_opt", "gray_33x70", "h1v2_48x64"]
    scanned = [pjd_amd.Scanned(golden_bytes(n)) for n in names]
    descs = [s.desc for s in scanned]
    P3 = [np.repeat(G.ref_plane(PORT, golden_bytes(n))[1][:, :, None], 3, axis=2) for n in names]
    c = pjd_amd.Context(0)
    th, tw = 21, 27
    # the three filters, prescale=False: exactly the filter over the full-size plane
    for kw, filt in ((dict(), "bilinear"), (dict(antialias=True), "antialias"), (dict(interpolation="bicubic"), "bicubic")):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (th, tw), prescale=False, gray=True, **kw)
        assert st == [0, 0, 0] and tuple(t.shape) == (3, 1, th, tw) and t.dtype == torch.uint8 and t.is_contiguous()
        for i, n in enumerate(names):
            want = pm.padded(P3[i], None, tw, th, (0, 0, 0, 0), (0, 0, 0), 1, filt)[..., 0]
            assert np.array_equal(t[i, 0].cpu().numpy(), want), (n, filt)
    # prescale=True: the box filter first, as for three channels
    t, st = tensors.decode_resized_batch_tensor(c, descs, (9, 11), gray=True)
    for i, d in enumerate(descs):
        log = tensors.pick_scale_flags(d.width, d.height, 11, 9) >> 4
        src = np.repeat(G.box1(P3[i][..., 0], 1 << log)[:, :, None], 3, axis=2)
        assert np.array_equal(t[i, 0].cpu().numpy(), pm.padded(src, None, 11, 9, (0, 0, 0, 0))[..., 0]), i
    # crops + flips + orientations, uint8
    oris, flips = [6, 3, 8], [True, False, True]
    crops = []
    for d, o in zip(descs, oris):
        uh, uw = tensors.orient_hw(o, d.height, d.width)
        crops.append((2, 1, uw - 5, uh - 3))
    t, st = tensors.decode_resized_batch_tensor(c, descs, (th, tw), prescale=False, gray=True, crops=crops, flips=flips, orientations=oris, antialias=True)
    assert tuple(t.shape) == (3, 1, th, tw)
    for i, d in enumerate(descs):
        win = dict(zip("xywh", tensors.crop_to_stored(oris[i], crops[i], d.width, d.height)))
        o = tensors.orient_then_hflip(oris[i]) if flips[i] else oris[i]
        want = pm.padded(P3[i], win, tw, th, (0, 0, 0, 0), (0, 0, 0), o, "antialias")[..., 0]
        assert np.array_equal(t[i, 0].cpu().numpy(), want), i
    # letterbox with a scalar fill
    t, st = tensors.decode_resized_batch_tensor(c, descs, (32, 32), prescale=False, gray=True, letterbox="center", fill=114)
    for i, d in enumerate(descs):
        ch, cw, left, top, right, bottom = tensors.letterbox_plan((d.height, d.width), (32, 32))
        want = pm.padded(P3[i], None, 32, 32, (left, top, right, bottom), (114,) * 3)[..., 0]
        assert np.array_equal(t[i, 0].cpu().numpy(), want), i
    # normalised: scalar mean / std / fill / pad_value, the three element types, resize_short
    for dtype, dt in ((torch.float16, pjd_amd.DT_F16), (torch.bfloat16, pjd_amd.DT_BF16), (torch.float32, pjd_amd.DT_F32)):
        scale, bias = tensors.normalize_constants([0.449] * 3, [0.226] * 3)
        t, st = tensors.decode_normalized_batch_tensor(c, descs, (32, 32), 0.449, [0.226], dtype=dtype, prescale=False, gray=True,
                                                       letterbox="topleft", fill=[7], pad_value=0)
        assert st == [0, 0, 0] and tuple(t.shape) == (3, 1, 32, 32) and t.dtype == dtype and t.is_contiguous()
        bits = t.view(torch.int32 if dtype == torch.float32 else torch.int16).cpu().numpy()
        for i, d in enumerate(descs):
            ch, cw, left, top, right, bottom = tensors.letterbox_plan((d.height, d.width), (32, 32), "topleft")
            pad = (left, top, right, bottom)
            C = pm.padded(P3[i], None, 32, 32, pad, (7, 7, 7))
            want = nm.bits(pm.normalized(C, 32, 32, pad, dt, scale, bias, (0.0, 0.0, 0.0))[..., 0])
            assert np.array_equal(bits[i, 0].view(want.dtype), want), (i, dt)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (20, 20), [0.5], 0.25, prescale=False, gray=True, resize_short=24)
    assert tuple(t.shape) == (3, 1, 20, 20) and t.dtype == torch.float16
    scale, bias = tensors.normalize_constants([0.5] * 3, [0.25] * 3)
    for i, d in enumerate(descs):
        win = tensors.center_crop_window((d.height, d.width), 24, (20, 20))
        C = pm.padded(P3[i], win, 20, 20, (0, 0, 0, 0))
        want = nm.bits(nm.normalize(C, pjd_amd.DT_F16, scale, bias)[..., 0])
        assert np.array_equal(t[i, 0].view(torch.int16).cpu().numpy().view(want.dtype), want), i
    # libjpeg=True: the filters read libjpeg's luma plane
    lj = ["lj_136x72_420_q90", "lj_40x24_422_q90", "lj_61x45_grey_q50"]
    sl = [pjd_amd.Scanned(G.lj_bytes(n)) for n in lj]
    t, st = tensors.decode_resized_batch_tensor(c, [s.desc for s in sl], (24, 40), prescale=False, gray=True, libjpeg=True, interpolation="bicubic")
    for i, n in enumerate(lj):
        want = pm.padded(np.repeat(G.l8(n)[:, :, None], 3, axis=2), None, 40, 24, (0, 0, 0, 0), (0, 0, 0), 1, "bicubic")[..., 0]
        assert np.array_equal(t[i, 0].cpu().numpy(), want), n
    # decode_to_tensors with orientations: the exact permutation of the plane
    import orientation_model as om
    outs, st = tensors.decode_to_tensors(c, descs, orientations=[5, 2, 7], gray=True)
    for i, o in enumerate([5, 2, 7]):
        assert np.array_equal(outs[i].cpu().numpy()[0], om.orient(P3[i][..., 0], o)), (i, o)
    # without the keyword nothing changed
    t3, _ = tensors.decode_resized_batch_tensor(c, descs, (th, tw))
    assert tuple(t3.shape) == (3, 3, th, tw)
    c.close()


if __name__ == "__main__":
    case = sys.argv[1]
    {"bound_canaries": case_bound_canaries, "tensors": case_tensors, "misaligned_bind": case_misaligned_bind,
     "resized_tensors": case_resized_tensors}[case]()
    print(f"CASE OK {case}")
