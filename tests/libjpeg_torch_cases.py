"""The cases of test_gpu_libjpeg.py that need torch, each run in a process of its own:

    python libjpeg_torch_cases.py <case>          # bound_output | composition | progressive

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.  Expected pictures
are the existing numpy models of the resize, the orientation and the normalisation applied to PILLOW'S recorded decode of the fixture:
with libjpeg=True the filters read libjpeg's picture, byte for byte."""
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
from test_libjpeg_cpu import fixture, manifest                    # noqa: E402

import libjpeg_progressive_corpus as LP                           # noqa: E402

NAMES = sorted(manifest()["cases"])                               # the progressive member included
PROGRESSIVE = ["lj_33x31_420_q90_prog", "lp_136x72_420_q50_skew_ri3", "lp_259x19_422_q75_two_bands"]
LP_JPEG = {n: data for n, data, _, _ in LP.fixtures()}


def _member(name):
    """(jpeg, Pillow's recorded decode, progressive) of a member of tests/golden/libjpeg/ or tests/golden/libjpeg_progressive/"""
    if name in LP_JPEG:
        return LP_JPEG[name], LP.record(name)[0], True
    data, rgb, c = fixture(name)
    return data, rgb, bool(c["progressive"])


def _batch(names):
    """Scanned with SCAN_PROGRESSIVE where the manifest says the member is progressive"""
    scanned = [pjd_amd.Scanned(_member(n)[0], options=pjd_amd.SCAN_PROGRESSIVE if _member(n)[2] else 0) for n in names]
    assert all(s.valid for s in scanned)
    return scanned, [s.desc for s in scanned], [_member(n)[1] for n in names]


def case_bound_output():
    """decode_to_tensors(libjpeg=True): the pictures land in a torch buffer, planar and interleaved; the caller's descriptors keep
    their flags; without the keyword the same call gives another picture (the reference's)."""
    scanned, descs, rgb = _batch(NAMES)
    c = pjd_amd.Context(0)
    for planar in (True, False):
        outs, st = tensors.decode_to_tensors(c, descs, planar=planar, libjpeg=True)
        assert st == [0] * len(NAMES)
        for n, t, want in zip(NAMES, outs, rgb):
            assert t.is_cuda and t.dtype == torch.uint8
            assert np.array_equal(t.cpu().numpy(), want.transpose(2, 0, 1) if planar else want), (n, planar)
    assert all(not (int(d.flags) & pjd_amd.F_LIBJPEG) for d in descs)
    plain, _ = tensors.decode_to_tensors(c, descs)
    assert any(not np.array_equal(t.cpu().numpy(), w.transpose(2, 0, 1)) for t, w in zip(plain, rgb))
    same = [n for n in NAMES if manifest()["cases"][n]["width"] == 136] + [n for n in sorted(LP_JPEG) if n.startswith("lp_136x72")]
    assert len(same) == 4
    _keep, d2, r2 = _batch(same)
    t, st = tensors.decode_to_batch_tensor(c, d2, libjpeg=True)
    assert st == [0] * len(same) and tuple(t.shape) == (len(same), 3, 72, 136)
    assert all(np.array_equal(t[i].cpu().numpy(), r2[i].transpose(2, 0, 1)) for i in range(len(same)))
    c.close()


def case_composition():
    """The three filters of decode_resized_batch_tensor, and decode_normalized_batch_tensor with an orientation and a crop, on top of
    the libjpeg picture: the existing models applied to the fixture's RGB, byte for byte."""
    names = ["lj_136x72_420_q90", "lj_136x72_420_q90_rst4", "lj_40x24_422_q90", "lj_61x45_grey_q50", "lj_33x31_420_q100", "lj_17x17_420_q90"]
    scanned, descs, rgb = _batch(names)
    c = pjd_amd.Context(0)
    th, tw = 24, 40
    for kw, filt in ((dict(), "bilinear"), (dict(antialias=True), "antialias"), (dict(interpolation="bicubic"), "bicubic")):
        t, st = tensors.decode_resized_batch_tensor(c, descs, (th, tw), prescale=False, libjpeg=True, **kw)
        assert st == [0] * len(names) and tuple(t.shape) == (len(names), 3, th, tw)
        host = t.cpu().numpy()
        for i, n in enumerate(names):
            want = om.window(rgb[i], None, tw, th, filt)
            assert np.array_equal(host[i], want.transpose(2, 0, 1)), (n, filt)
    # normalised fp16, every picture turned a quarter (orientation 6) and cropped in the upright picture's coordinates
    oris = [6] * len(names)
    crops = []
    for d in descs:
        uh, uw = tensors.orient_hw(6, d.height, d.width)
        crops.append((1, 2, uw - 3, uh - 4))
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (th, tw), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.float16, prescale=False,
                                                   crops=crops, orientations=oris, libjpeg=True)
    assert st == [0] * len(names) and tuple(t.shape) == (len(names), 3, th, tw)
    bits = t.contiguous().view(torch.int16).cpu().numpy()
    for i, (n, d) in enumerate(zip(names, descs)):
        win = dict(zip("xywh", tensors.crop_to_stored(6, crops[i], d.width, d.height)))
        u8 = om.oriented(rgb[i], win, tw, th, 6)
        want = nm.bits(nm.normalize(u8, nm.DT_F16, scale, bias))
        assert np.array_equal(bits[i].view(want.dtype), want.transpose(2, 0, 1)), n
    c.close()


def case_progressive():
    """The progressive members -- Pillow's own scan script and two hand-made ones that span several back-end ranges -- through bound
    output, planar and interleaved, and through one antialiased resize to 32 x 32 with normalisation: the existing models over Pillow's
    record, byte for byte and bit for bit."""
    scanned, descs, rgb = _batch(PROGRESSIVE)
    assert all(int(d.flags) & pjd_amd.F_PROGRESSIVE for d in descs)
    c = pjd_amd.Context(0)
    for planar in (True, False):
        outs, st = tensors.decode_to_tensors(c, descs, planar=planar, libjpeg=True)
        assert st == [0] * len(PROGRESSIVE)
        for n, t, want in zip(PROGRESSIVE, outs, rgb):
            assert np.array_equal(t.cpu().numpy(), want.transpose(2, 0, 1) if planar else want), (n, planar)
    th, tw = 32, 32
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    t, st = tensors.decode_normalized_batch_tensor(c, descs, (th, tw), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.float16, prescale=False,
                                                   antialias=True, libjpeg=True)
    assert st == [0] * len(PROGRESSIVE) and tuple(t.shape) == (len(PROGRESSIVE), 3, th, tw)
    bits = t.contiguous().view(torch.int16).cpu().numpy()
    for i, n in enumerate(PROGRESSIVE):
        want = nm.bits(nm.normalize(om.window(rgb[i], None, tw, th, "antialias"), nm.DT_F16, scale, bias))
        assert np.array_equal(bits[i].view(want.dtype), want.transpose(2, 0, 1)), n
    c.close()


if __name__ == "__main__":
    case = sys.argv[1]
    {"bound_output": case_bound_output, "composition": case_composition, "progressive": case_progressive}[case]()
    print(f"CASE OK {case}")
