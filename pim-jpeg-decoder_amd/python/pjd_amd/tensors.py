"""pjd_amd.tensors -- decoded pictures as torch tensors on the GPU, with no copy after the decode.

The batch is bound (Batch.bind_output, pjd_batch_bind_output of include/pjd.h) to ONE torch.uint8 buffer this module allocates
on the context's device; the back end writes the pictures straight into it -- planar R, G, B (OUT_RGB8_PLANAR, "CHW") by
default -- and the results are views of that buffer.  No native code of its own.  torch is imported inside the functions that
need it: uniform_output_shape(), pick_scale_flags() and normalize_constants() are pure.

Pictures of different sizes become ONE [N, 3, H, W] tensor with decode_resized_batch_tensor: the library resamples every picture to
H x W inside the decode (Batch.set_resize, pjd_batch_set_resize), after the box pre-scale pick_scale_flags chooses.

The tensor a model takes -- fp16, bf16 or fp32, (x / 255 - mean) / std -- comes out of the same launch with
decode_normalized_batch_tensor (Batch.set_normalize, pjd_batch_set_normalize): no uint8 tensor, no elementwise kernels after it.

torch ships a HIP runtime of its own.  A tensor's address means something to libpjd.so only if both use ONE runtime, which is the
case when torch is loaded first (libpjd.so then binds to the runtime torch brought): `import torch` before the first pjd_amd call
that loads the library (Context(), plan_info(), ...).  The other way round torch finds no GPU, and these functions say so.

Stream order.  The library works on its own stream (pjd_stream(ctx), non-blocking: no implicit order with torch's streams), and
this module is the caller that include/pjd.h makes responsible for ordering the two.  Before the decode: torch's caching allocator
may hand out a block that kernels still queued on torch's current stream read (tensors of an earlier call, dropped while a model
was consuming them) -- stream order protects such a block on torch's stream only -- so torch's current stream is drained after
the allocation and before the library writes.  After the decode: Batch.sync() has drained the library's stream and settled the
statuses (fallback re-decodes included), so the returned tensors are complete and safe to read on any stream.
"""
import pjd_amd


def _scale_log(flags):
    return (int(flags) & pjd_amd.F_SCALE_MASK) >> 4


def output_hw(desc):
    """(h, w) of the picture a descriptor gives at its output scale (F_SCALE_*): ceil(H / s), ceil(W / s).  Pure."""
    s = _scale_log(desc.flags)
    return (int(desc.height) + (1 << s) - 1) >> s, (int(desc.width) + (1 << s) - 1) >> s


def uniform_output_shape(descs):
    """(N, 3, H, W) if every descriptor gives a picture of the same output size (scale flags included), else ValueError.  Pure: no
    context, no torch."""
    if len(descs) == 0:
        raise ValueError("uniform_output_shape: no pictures")
    h, w = output_hw(descs[0])
    for i, d in enumerate(descs):
        if output_hw(d) != (h, w):
            raise ValueError(f"uniform_output_shape: picture {i} is {output_hw(d)[1]}x{output_hw(d)[0]}, picture 0 is {w}x{h}")
    return len(descs), 3, h, w


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise pjd_amd.PjdError("torch sees no GPU in this process: import torch before the first pjd_amd call that loads libpjd.so, "
                               "so that both use one HIP runtime")
    return torch


def _run(ctx, descs, out_format, capacity, offsets, device, resize=None, normalize=None, antialias=False):
    """Create, (set the resize, its filter, the normalisation,) bind to a fresh torch buffer, upload, decode, sync -> (buffer, batch offsets,
    statuses).  The buffer is torch.uint8 whatever the elements are: torch aligns it far beyond an element."""
    torch = _torch()
    with ctx.batch(descs, out_format) as b:
        if resize is not None:
            b.set_resize(resize)
            if antialias:
                b.set_resize_filter(pjd_amd.RESIZE_ANTIALIAS)
        if normalize is not None:
            b.set_normalize(*normalize)
        cap = b.packed_size() if capacity is None else capacity
        buf = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
        # the block may be a recycled one that work queued on torch's current stream still reads: order that work before ours
        torch.cuda.current_stream(device).synchronize()
        b.bind_output(buf.data_ptr(), cap, offsets)
        b.upload()
        b.decode()
        b.sync()                                    # the library's stream has drained, fallbacks are settled: readable on any stream
        st = b.statuses()
        offs = [b.output_offset(i) for i in range(b.n)]
    return buf, offs, st


def decode_to_tensors(ctx, descs, planar=True, device=None):
    """Decode `descs` on `ctx` into ONE torch.uint8 buffer on the context's device -> (list of tensors, statuses).  Tensor i is
    a view of that buffer shaped (3, sh, sw) -- or (sh, sw, 3) with planar=False -- at the picture's output scale.  The tensors
    are complete on return and may be read on any torch stream (module docstring, "Stream order")."""
    torch = _torch()
    device = torch.device("cuda", ctx.device) if device is None else device
    buf, offs, st = _run(ctx, descs, pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8, None, None, device)
    out = []
    for d, off in zip(descs, offs):
        h, w = output_hw(d)
        flat = buf[off:off + 3 * h * w]
        out.append(flat.view(3, h, w) if planar else flat.view(h, w, 3))
    return out, st


def decode_to_batch_tensor(ctx, descs, device=None):
    """Pictures of ONE output size -> (uint8 tensor [N, 3, H, W], statuses): picture i is bound at offset i * 3 * H * W, so the
    result is one contiguous NCHW tensor with no copy after the decode, complete on return and readable on any torch stream.
    ValueError (before anything is created) otherwise."""
    n, c, h, w = uniform_output_shape(descs)
    torch = _torch()
    device = torch.device("cuda", ctx.device) if device is None else device
    size = c * h * w
    buf, _, st = _run(ctx, descs, pjd_amd.OUT_RGB8_PLANAR, n * size, [i * size for i in range(n)], device)
    return buf.view(n, c, h, w), st


def pick_scale_flags(w, h, tw, th):
    """The F_SCALE_* value to decode a w x h picture with before it is resized to tw x th: that of the largest s of 1, 2, 4, 8 with
    ceil(w / s) >= tw and ceil(h / s) >= th, so that the bilinear step shrinks by less than 2x on the axis that limits s (s < 8) whenever
    the source is at least the target; 0 when the target is larger than the source on either axis.  Pure."""
    w, h, tw, th = int(w), int(h), int(tw), int(th)
    for log in (3, 2, 1):
        if (w + (1 << log) - 1) >> log >= tw and (h + (1 << log) - 1) >> log >= th:
            return log << 4
    return 0


def prescaled_descs(descs, size):
    """Copies of `descs` whose scale flags are pick_scale_flags for the target size = (H, W); the caller's descriptors are not
    touched (the copies share their bitstream and table memory, which the caller keeps alive as for any batch).  No device."""
    import ctypes
    th, tw = size
    out = []
    for d in descs:
        c = pjd_amd.ImageDesc()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(pjd_amd.ImageDesc))
        c.flags = (int(d.flags) & ~pjd_amd.F_SCALE_MASK) | pick_scale_flags(d.width, d.height, tw, th)
        out.append(c)
    return out


def decode_resized_batch_tensor(ctx, descs, size, prescale=True, device=None, antialias=False):
    """Pictures of ANY sizes -> (uint8 tensor [N, 3, H, W], statuses), size = (H, W): every picture is resampled to H x W inside
    the decode (the bilinear filter of include/pjd.h, pjd_batch_set_resize) and lands at offset i * 3 * H * W of one buffer, so
    the result is one contiguous NCHW tensor with no copy after the decode, complete on return and readable on any torch stream
    (module docstring, "Stream order").  prescale: decode copies of the descriptors at the reduced size pick_scale_flags chooses
    (the box filter takes the bulk of a large reduction: no aliasing, and less to decode); else the descriptors' own flags hold.
    antialias=True: the resize is the antialiased triangle filter of include/pjd.h (Batch.set_resize_filter) -- what
    torch.nn.functional.interpolate(mode="bilinear", antialias=True), torchvision's Resize(antialias=True) and Pillow's BILINEAR
    compute, to within 1 level.  With prescale=True the box pre-scale is still chosen (less to decode; the triangle filter removes
    what the box leaves), so the result differs from an antialiased resize of the full-size picture; prescale=False gives exactly
    that, for pictures up to 16x the target on each axis (beyond that the call raises)."""
    if len(descs) == 0:
        raise ValueError("decode_resized_batch_tensor: no pictures")
    th, tw = int(size[0]), int(size[1])
    torch = _torch()
    device = torch.device("cuda", ctx.device) if device is None else device
    run = prescaled_descs(descs, (th, tw)) if prescale else descs
    n, plane = len(descs), 3 * th * tw
    buf, _, st = _run(ctx, run, pjd_amd.OUT_RGB8_PLANAR, n * plane, [i * plane for i in range(n)], device, resize=[(th, tw)] * n,
                      antialias=antialias)
    return buf.view(n, 3, th, tw), st


def normalize_constants(mean, std):
    """(scale, bias), three np.float32 each, for Batch.set_normalize: scale[c] = 1 / (255 * std[c]), bias[c] = -mean[c] / std[c], so that
    fma(v, scale, bias) is (v / 255 - mean) / std.  Computed in float64 and rounded once to float32.  Pure."""
    import numpy as np
    mean, std = np.asarray(mean, np.float64).reshape(-1), np.asarray(std, np.float64).reshape(-1)
    if mean.shape != (3,) or std.shape != (3,):
        raise ValueError("normalize_constants: three means and three standard deviations (R, G, B)")
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0)):
        raise ValueError("normalize_constants: finite means, finite non-zero standard deviations")
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def decode_normalized_batch_tensor(ctx, descs, size, mean, std, dtype=None, channels_last=False, prescale=True, device=None,
                                   antialias=False):
    """Pictures of ANY sizes -> (tensor of `dtype` [N, 3, H, W], statuses), size = (H, W); dtype torch.float16 (the default),
    torch.bfloat16 or torch.float32.  As decode_resized_batch_tensor, and every sample v of channel c leaves the same launch as
    fma(v, scale[c], bias[c]) with the constants of normalize_constants(mean, std), converted once to `dtype` (include/pjd.h,
    pjd_batch_set_normalize): what x.float().div(255).sub(mean).div(std).to(dtype) makes of the uint8 tensor, which never exists.
    channels_last=False: one contiguous NCHW tensor.  channels_last=True: the batch is decoded interleaved into an [N, H, W, 3] buffer
    and the result is its permute(0, 3, 1, 2) view: shape [N, 3, H, W] in torch's channels_last memory format.  Complete on return and
    readable on any torch stream (module docstring, "Stream order").  antialias=True: the antialiased filter, as in
    decode_resized_batch_tensor -- with prescale=True the result differs from an antialiased resize of the full-size picture (the box
    pre-scale comes first), prescale=False gives exactly that up to the 16x limit."""
    if len(descs) == 0:
        raise ValueError("decode_normalized_batch_tensor: no pictures")
    th, tw = int(size[0]), int(size[1])
    scale, bias = normalize_constants(mean, std)
    torch = _torch()
    dtype = torch.float16 if dtype is None else dtype
    dts = {torch.float16: (pjd_amd.DT_F16, 2), torch.bfloat16: (pjd_amd.DT_BF16, 2), torch.float32: (pjd_amd.DT_F32, 4)}
    if dtype not in dts:
        raise ValueError("decode_normalized_batch_tensor: dtype must be torch.float16, torch.bfloat16 or torch.float32")
    dt, es = dts[dtype]
    device = torch.device("cuda", ctx.device) if device is None else device
    run = prescaled_descs(descs, (th, tw)) if prescale else descs
    n, pic = len(descs), 3 * th * tw * es
    buf, _, st = _run(ctx, run, pjd_amd.OUT_RGB8 if channels_last else pjd_amd.OUT_RGB8_PLANAR, n * pic, [i * pic for i in range(n)], device,
                      resize=[(th, tw)] * n, normalize=(dt, scale, bias), antialias=antialias)
    t = buf.view(dtype)
    return (t.view(n, th, tw, 3).permute(0, 3, 1, 2) if channels_last else t.view(n, 3, th, tw)), st
