"""pjd_amd.tensors -- decoded pictures as torch tensors on the GPU, with no copy after the decode.

The batch is bound (Batch.bind_output, pjd_batch_bind_output of include/pjd.h) to ONE torch.uint8 buffer this module allocates
on the context's device; the back end writes the pictures straight into it -- planar R, G, B (OUT_RGB8_PLANAR, "CHW") by
default -- and the results are views of that buffer.  No native code of its own.  torch is imported inside the functions that
need it: uniform_output_shape() is pure.

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


def _run(ctx, descs, out_format, capacity, offsets, device):
    """Create, bind to a fresh torch buffer, upload, decode, sync -> (buffer, batch offsets, statuses)."""
    torch = _torch()
    with ctx.batch(descs, out_format) as b:
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
