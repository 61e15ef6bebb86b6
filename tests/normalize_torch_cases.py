"""The cases of test_gpu_normalize.py that need torch, each run in a process of its own:

    python normalize_torch_cases.py <case> [arguments]

As tests/resize_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and libpjd.so
use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback."""
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
import pjd_amd                                                    # noqa: E402
from pjd_amd import tensors                                       # noqa: E402
from conftest import golden_bytes                                 # noqa: E402

NAMES = ["env_61x45_444_q85_opt", "noise_80x96_422_q50_opt", "wrap_420_q65535", "wrap_440_q65535", "wrap_gray_q65535", "err_truncated_eoi_420",
         "big_640x480_420_q85"]


def case_normalized_batch_tensor(channels_last):
    channels_last = bool(int(channels_last))
    ctx = pjd_amd.Context(0)
    scanned = [pjd_amd.Scanned(golden_bytes(n)) for n in NAMES]
    descs = [s.desc for s in scanned]
    n = len(descs)
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    for size, prescale in (((37, 53), True), ((224, 224), True), ((45, 61), False)):
        th, tw = size
        u8, st_u8 = tensors.decode_resized_batch_tensor(ctx, descs, size, prescale=prescale)
        u8 = u8.cpu().numpy()                                     # [N, 3, H, W]: the P' of include/pjd.h
        assert u8.shape == (n, 3, th, tw)
        for dtype, dt, as_int in ((torch.float16, nm.DT_F16, torch.int16), (torch.bfloat16, nm.DT_BF16, torch.int16), (torch.float32, nm.DT_F32, torch.int32)):
            t, st = tensors.decode_normalized_batch_tensor(ctx, descs, size, nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=dtype,
                                                           channels_last=channels_last, prescale=prescale)
            assert st == st_u8 and st[5] != 0
            assert t.dtype == dtype and t.is_cuda and tuple(t.shape) == (n, 3, th, tw)
            if channels_last:
                assert t.is_contiguous(memory_format=torch.channels_last) and t.permute(0, 2, 3, 1).is_contiguous()
            else:
                assert t.is_contiguous()
            assert t[3].data_ptr() == t.data_ptr() + 3 * 3 * th * tw * t.element_size()
            got = t.contiguous().view(as_int).cpu().numpy()       # NCHW order on the host, raw bits
            want = nm.normalize(u8.transpose(0, 2, 3, 1), dt, scale, bias).transpose(0, 3, 1, 2)
            assert np.array_equal(got.view(nm.bits(want).dtype), nm.bits(want)), (size, str(dtype), channels_last)
            # torch computes on the memory
            assert torch.isfinite(t.float().sum()).item()
    t, _ = tensors.decode_normalized_batch_tensor(ctx, descs[:2], (8, 8), nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    assert t.dtype == torch.float16                               # the default
    try:
        tensors.decode_normalized_batch_tensor(ctx, descs[:2], (8, 8), nm.IMAGENET_MEAN, nm.IMAGENET_STD, dtype=torch.float64)
        raise AssertionError("float64 accepted")
    except ValueError:
        pass
    ctx.close()


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]](*sys.argv[2:])
    print("CASE OK", sys.argv[1], flush=True)
