"""The cases of test_gpu_libjpeg_scaled.py that need torch, each run in a process of its own:

    python libjpeg_scaled_torch_cases.py <case>       # bound_poisoned_rgb8 | bound_poisoned_planar | bound_poisoned_gray | draft_resize

As tests/libjpeg_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected pictures
are Pillow's recorded draft decodes (tests/golden/libjpeg_scaled/), and the existing numpy models of the resize and the normalisation
applied to them: with draft=True the filters read libjpeg's reduced picture, byte for byte."""
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

import normalize_model as nm                                      # noqa: E402
import orientation_model as om                                    # noqa: E402
import pjd_amd                                                    # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from test_libjpeg_scaled_cpu import FLAG, MODEL_ONLY, jpeg, manifest, recording   # noqa: E402

NAMES = sorted(manifest()["cases"])


def _scanned(name, flags=0):
    c = manifest()["cases"][name]
    s = pjd_amd.Scanned(jpeg(name), options=pjd_amd.SCAN_PROGRESSIVE if c["progressive"] else 0)
    assert s.valid
    s.desc.flags = int(s.desc.flags) | flags
    return s


def case_bound_poisoned(fmt):
    """Every fixture at every recorded reduced scale, bound at odd offsets with gaps into a tensor filled with a poison byte, once per
    byte of two: each range holds the recording whichever the poison was -- so every byte of it was written -- and no byte outside the
    ranges changed."""
    items = [(n, s) for n in NAMES for s in (2, 4, 8) if (n, s) not in MODEL_ONLY]
    out_fmt = {"rgb8": pjd_amd.OUT_RGB8, "planar": pjd_amd.OUT_RGB8_PLANAR, "gray": pjd_amd.OUT_GRAY8}[fmt]
    ctx = pjd_amd.Context(0)
    for poison in (0xA5, 0x5A):
        sc = [_scanned(n, pjd_amd.F_LIBJPEG | FLAG[s]) for n, s in items]
        with ctx.batch([x.desc for x in sc], out_fmt) as b:
            offs, pos = [], 37
            for i in range(b.n):
                offs.append(pos)
                pos += b.output_size(i) + 2 * i + 1
            total = pos + 4096
            buf = torch.full((total,), poison, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            b.bind_output(buf.data_ptr(), total, offs)
            b.upload(); b.decode(); b.sync()
            st = b.statuses()
            sizes = [b.output_size(i) for i in range(b.n)]
        host = buf.cpu().numpy()
        covered = np.zeros(total, bool)
        for i, (n, s) in enumerate(items):
            rec = recording(n, s, "l8" if fmt == "gray" else "rgb")
            want = np.ascontiguousarray(rec.transpose(2, 0, 1)) if fmt == "planar" else rec
            assert st[i] == 0 and sizes[i] == want.size, (n, s)
            assert np.array_equal(host[offs[i]:offs[i] + sizes[i]], want.reshape(-1)), (n, s, hex(poison))
            covered[offs[i]:offs[i] + sizes[i]] = True
        stray = np.flatnonzero(~covered & (host != poison))
        assert stray.size == 0, f"bytes outside every picture range were written, first at {stray[:8]}"
    ctx.close()


def case_draft_resize():
    """draft=True: each picture is decoded at the scale pick_libjpeg_scale_flags chooses for the target and the filters read that
    reduced picture -- the existing models over Pillow's recording at that scale; uint8 with the three filters, normalised fp16, grey;
    decode_to_tensors(draft=s) is the recording itself."""
    names = ["ls_136x72_420_q90", "ls_136x72_420_q100_rst4", "ls_259x19_422_q50", "ls_61x45_grey_q50", "ls_33x31_420_q90_prog", "ls_40x24_422_q90"]
    th, tw = 9, 17
    scanned = [_scanned(n) for n in names]
    descs = [s.desc for s in scanned]
    scales = [1 << (tensors.pick_libjpeg_scale_flags(d.width, d.height, tw, th) >> 7) for d in descs]
    assert scales == [8, 8, 2, 2, 2, 2], scales
    rgb = [recording(n, s, "rgb") for n, s in zip(names, scales)]
    c = pjd_amd.Context(0)
    for kw, filt in ((dict(), "bilinear"), (dict(antialias=True), "antialias"), (dict(interpolation="bicubic"), "bicubic")):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (th, tw), prescale=False, libjpeg=True, draft=True, **kw)
        assert st == [0] * len(names) and tuple(t.shape) == (len(names), 3, th, tw)
        host = t.cpu().numpy()
        for i, n in enumerate(names):
            assert np.array_equal(host[i], om.window(rgb[i], None, tw, th, filt).transpose(2, 0, 1)), (n, filt)
    assert all(not (int(d.flags) & (pjd_amd.F_LIBJPEG | pjd_amd.F_LIBJPEG_SCALE_MASK)) for d in descs)
    # without draft the same call reads the full-size picture: another result for the pictures that were reduced
    full, _ = tensors.decode_resized_batch_tensor(c, descs, (th, tw), prescale=False, libjpeg=True, interpolation="bicubic")
    assert not np.array_equal(full[0].cpu().numpy(), host[0])
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (th, tw), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.float16, prescale=False,
                                                   antialias=True, libjpeg=True, draft=True)
    assert st == [0] * len(names) and tuple(t.shape) == (len(names), 3, th, tw)
    bits = t.contiguous().view(torch.int16).cpu().numpy()
    for i, n in enumerate(names):
        want = nm.bits(nm.normalize(om.window(rgb[i], None, tw, th, "antialias"), nm.DT_F16, scale, bias))
        assert np.array_equal(bits[i].view(want.dtype), want.transpose(2, 0, 1)), n
    # grey: channel 0 of what the filter makes of the recorded luma plane
    t, st = tensors.decode_resized_batch_tensor(c, descs, (th, tw), prescale=False, libjpeg=True, draft=True, gray=True, antialias=True)
    assert st == [0] * len(names) and tuple(t.shape) == (len(names), 1, th, tw)
    host = t.cpu().numpy()
    for i, (n, s) in enumerate(zip(names, scales)):
        l8 = recording(n, s, "l8")
        want = om.window(np.stack([l8, l8, l8], axis=-1), None, tw, th, "antialias")[:, :, 0]
        assert np.array_equal(host[i, 0], want), n
    # decode_to_tensors at a given denominator
    for s in (2, 4, 8):
        outs, st = tensors.decode_to_tensors(c, descs, libjpeg=True, draft=s)
        assert st == [0] * len(names)
        for n, o in zip(names, outs):
            assert np.array_equal(o.cpu().numpy(), recording(n, s, "rgb").transpose(2, 0, 1)), (n, s)
    outs, _ = tensors.decode_to_tensors(c, descs, libjpeg=True, draft=4, gray=True)
    for n, o in zip(names, outs):
        assert np.array_equal(o.cpu().numpy()[0], recording(n, 4, "l8")), n
    c.close()


if __name__ == "__main__":
    case = sys.argv[1]
    if case.startswith("bound_poisoned_"):
        case_bound_poisoned(case[len("bound_poisoned_"):])
    else:
        {"draft_resize": case_draft_resize}[case]()
    print(f"CASE OK {case}")
