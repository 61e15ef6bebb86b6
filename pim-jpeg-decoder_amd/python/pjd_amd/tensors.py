"""pjd_amd.tensors -- decoded pictures as torch tensors on the GPU, with no copy after the decode.

The batch is bound (Batch.bind_output, pjd_batch_bind_output of include/pjd.h) to ONE torch.uint8 buffer this module allocates
on the context's device; the back end writes the pictures straight into it -- planar R, G, B (OUT_RGB8_PLANAR, "CHW") by
default -- and the results are views of that buffer.  No native code of its own.  torch is imported inside the functions that
need it: uniform_output_shape(), pick_scale_flags(), pick_libjpeg_scale_flags(), normalize_constants(), center_crop_window(), window_at_scale(), orient_hw(),
orient_then_hflip(), crop_to_stored(), tile_views(), least_reduced_scale_flags(), plan_views(), affine_inverse_matrix(), orientation_matrix(),
plan_affines() and colour_matrix() are pure.

Pictures of different sizes become ONE [N, 3, H, W] tensor with decode_resized_batch_tensor: the library resamples every picture to
H x W inside the decode (Batch.set_resize, pjd_batch_set_resize), after the box pre-scale pick_scale_flags chooses.

Crops and flips ride in that resample (Batch.set_resize_window, pjd_batch_set_resize_window): crops= takes what
RandomResizedCrop.get_params returns, flips= mirrors, resize_short= is Resize(int) + CenterCrop(size).  Every picture is still decoded
whole; the window costs no launch and no uint8 tensor.

Orientation rides there too (Batch.set_orientation, pjd_batch_set_orientation): orientations= takes the EXIF orientation of every
picture (Scanned.orientation) and the pictures come out upright -- what torchvision.io.decode_jpeg(apply_exif_orientation=True) and
PIL.ImageOps.exif_transpose give -- with crops=, flips= and resize_short= speaking about the UPRIGHT picture.  No transpose / flip +
.contiguous() pass over the finished tensor.

Several outputs of one picture -- two augmented views, multi-crop, FiveCrop, two scales of a crop, tiles -- come from ONE decode of it
with views= (Batch.set_views, pjd_batch_set_views): view v is a resample of picture views[v], every per-picture keyword then has one
entry per view, the result is [V, C, H, W] and the statuses stay per picture.  tile_views() cuts one picture into a grid of tiles.

Rotation, shear, anisotropic scale and translation -- torchvision's RandomRotation / RandomAffine, DALI's warp_affine, the geometric
ops of RandAugment -- come out of the decode with affines= (Batch.set_resize_affine, pjd_batch_set_resize_affine): one inverse 2 x 3
matrix per output, which affine_inverse_matrix() makes from an angle, a translation, a scale and a shear; `fill` where the output looks
outside the picture.  No grid_sample pass over a float tensor.

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
import collections
import math

import pjd_amd


def _copy_desc(d, mask, bits):
    """A copy of descriptor d whose flag bits under `mask` are `bits`: the one place a descriptor is copied.  d is not written; the
    copy shares its bitstream and table memory, which the caller keeps alive as for any batch."""
    import ctypes
    c = pjd_amd.ImageDesc()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(pjd_amd.ImageDesc))
    c.flags = (int(d.flags) & ~mask) | bits
    return c


def libjpeg_descs(descs):
    """Copies of `descs` with F_LIBJPEG set (the picture libjpeg decodes, include/pjd.h); the caller's descriptors are not touched (the
    copies share their bitstream and table memory, as prescaled_descs' do).  No device."""
    return [_copy_desc(d, pjd_amd.F_LIBJPEG, pjd_amd.F_LIBJPEG) for d in descs]


def _libjpeg(descs, libjpeg, prescale=False, draft=False):
    """The descriptors a helper decodes for its `libjpeg` keyword, checked before anything is created: the mode takes no output scale
    but libjpeg's own (`draft`), which in turn needs the mode."""
    if draft and not libjpeg:
        raise ValueError("draft needs libjpeg=True: libjpeg's reduced decode (F_LIBJPEG_SCALE_*) exists only for its picture; the box pre-scale is prescale=True")
    if not libjpeg:
        return descs
    if prescale:
        raise ValueError("libjpeg=True takes prescale=False: the box pre-scale (F_SCALE_*) is not libjpeg's reduced decode")
    for i, d in enumerate(descs):
        if int(d.flags) & pjd_amd.F_SCALE_MASK:
            raise ValueError(f"libjpeg=True: picture {i} carries an output scale (F_SCALE_*)")
    return libjpeg_descs(descs)


def _scale_log(flags):
    """log2 of the output scale denominator: the box filter's (F_SCALE_*) or, on a flagged picture, libjpeg's (F_LIBJPEG_SCALE_*)."""
    return ((int(flags) & pjd_amd.F_SCALE_MASK) >> 4) or ((int(flags) & pjd_amd.F_LIBJPEG_SCALE_MASK) >> 7)


def output_hw(desc):
    """(h, w) of the picture a descriptor gives at its output scale (F_SCALE_* or F_LIBJPEG_SCALE_*): ceil(H / s), ceil(W / s).  Pure."""
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


# What one call asks of a batch, settled before the batch exists: the descriptors to decode and the output format; the capacity and the
# offsets to bind (None: packed); then what the setters take, each None where its setter is not called -- views, sizes (set_resize), pads
# with fill (set_resize_pad), orientations, windows, filter (set_resize_filter), normalize = (dtype, scale, bias), pad_value.
# affines (set_resize_affine, with fill) stands in place of pads, orientations, windows and filter.  colours (set_colour) comes behind
# all of them and before normalize, blurs (set_blur) behind colours.
_Request = collections.namedtuple("_Request", "descs out_format capacity offsets views sizes pads fill orientations windows filter normalize pad_value affines colours blurs",
                                  defaults=(None,) * 14)


def _run(ctx, req, device):
    """Create the batch of request `req`, make the setter calls it holds, bind to a fresh torch buffer, upload, decode, sync -> (buffer,
    batch offsets, statuses).  The buffer is torch.uint8 whatever the elements are: torch aligns it far beyond an element."""
    torch = _torch()
    device = torch.device("cuda", ctx.device) if device is None else device
    with ctx.batch(req.descs, req.out_format) as b:
        if req.views is not None:
            b.set_views(req.views)                  # from here on every per-picture argument is per view; the statuses stay per picture
        if req.sizes is not None:
            b.set_resize(req.sizes)
            if req.affines is not None:
                b.set_resize_affine(req.affines, req.fill)
            if req.pads is not None:
                b.set_resize_pad(req.pads, req.fill)
            if req.orientations is not None:
                b.set_orientation(req.orientations)
            if req.windows is not None:
                b.set_resize_window(req.windows)
            if req.filter is not None:
                b.set_resize_filter(req.filter)
            if req.colours is not None:
                b.set_colour(req.colours)
            if req.blurs is not None:
                b.set_blur(req.blurs)
        if req.normalize is not None:
            b.set_normalize(*req.normalize)
            if req.pads is not None and req.pad_value is not None:
                b.set_pad_value(req.pad_value)
        cap = b.packed_size() if req.capacity is None else req.capacity
        buf = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
        # the block may be a recycled one that work queued on torch's current stream still reads: order that work before ours
        torch.cuda.current_stream(device).synchronize()
        b.bind_output(buf.data_ptr(), cap, req.offsets)
        b.upload()
        b.decode()
        b.sync()                                    # the library's stream has drained, fallbacks are settled: readable on any stream
        st = b.statuses()
        offs = [b.output_offset(i) for i in range(b.n if req.views is None else len(req.views))]
    return buf, offs, st


def _gray_layout(gray, planar=True):
    """The `gray` keyword, checked before anything is created: one plane has no interleaved form."""
    if gray and not planar:
        raise ValueError("gray=True takes planar=True (and no channels_last): one plane has no interleaved form")


def _gray3(v, what):
    """A per-channel argument of a gray=True call -- one number, or a sequence of length 1 (or 3: entries [1] and [2] are ignored, as the
    library ignores them) -- as the three entries the C ABI takes."""
    if isinstance(v, (int, float)):
        return [v, v, v]
    v = list(v)
    if len(v) == 1:
        return [v[0]] * 3
    if len(v) != 3:
        raise ValueError(f"{what}: with gray=True one number, or a sequence of length 1 (or 3)")
    return v


def pick_libjpeg_scale_flags(w, h, tw, th):
    """The F_LIBJPEG_SCALE_* value to decode a flagged w x h picture with before it is resized to tw x th: that of the largest s of 1, 2,
    4, 8 with ceil(w / s) >= tw and ceil(h / s) >= th (what a loader that drafts before it resizes asks libjpeg for); 0 when the target
    is larger than the source on either axis.  Pure."""
    return (pick_scale_flags(w, h, tw, th) >> 4) << 7


def drafted_descs(descs, size):
    """Copies of `descs` (flagged F_LIBJPEG, or about to be) whose F_LIBJPEG_SCALE_* bits are pick_libjpeg_scale_flags for the target
    size = (H, W); the caller's descriptors are not touched.  No device."""
    th, tw = size
    return [_scaled_copy(d, "draft", d.width, d.height, tw, th) for d in descs]


def _scaled_copy(d, prescale, cw, ch, vw, vh):
    """A copy of descriptor d with the scale picked for a cw x ch source against a vw x vh target: the box filter's (prescale true) or
    libjpeg's own (prescale == "draft")."""
    if prescale == "draft":
        return _copy_desc(d, pjd_amd.F_LIBJPEG_SCALE_MASK, pick_libjpeg_scale_flags(cw, ch, vw, vh))
    return _copy_desc(d, pjd_amd.F_SCALE_MASK, pick_scale_flags(cw, ch, vw, vh))


def _draft_flags(draft):
    """The `draft` keyword of decode_to_tensors: False, or the denominator 1, 2, 4 or 8 -> F_LIBJPEG_SCALE_* bits."""
    if draft is False or draft is None:
        return 0
    if draft is True or int(draft) != draft or int(draft) not in (1, 2, 4, 8):
        raise ValueError("decode_to_tensors: draft is False or a scale denominator 1, 2, 4 or 8 (there is no target size to pick one from)")
    return {1: 0, 2: pjd_amd.F_LIBJPEG_SCALE_1_2, 4: pjd_amd.F_LIBJPEG_SCALE_1_4, 8: pjd_amd.F_LIBJPEG_SCALE_1_8}[int(draft)]


def decode_to_tensors(ctx, descs, planar=True, device=None, orientations=None, libjpeg=False, gray=False, draft=False):
    """Decode `descs` on `ctx` into ONE torch.uint8 buffer on the context's device -> (list of tensors, statuses).  Tensor i is
    a view of that buffer shaped (3, sh, sw) -- or (sh, sw, 3) with planar=False -- at the picture's output scale.  The tensors
    are complete on return and may be read on any torch stream (module docstring, "Stream order").
    orientations=[1..8, ...] (Scanned.orientation): every picture comes out upright, at its own size -- (3, sw, sh) for 5..8 --, the
    exact permutation of the decoded picture (the identity resample of Batch.set_resize with Batch.set_orientation).  None: as the file
    stores them.  libjpeg=True: the pictures are libjpeg's, byte for byte (F_LIBJPEG on copies of the descriptors).
    gray=True: one plane per picture (OUT_GRAY8: the luma, what libjpeg's JCS_GRAYSCALE delivers with libjpeg=True), views shaped
    (1, sh, sw) -- (1, sw, sh) for orientations 5..8 --; a third of the bytes.  It takes planar=True (ValueError before anything is created
    otherwise).  draft=2 | 4 | 8 (only with libjpeg=True, ValueError otherwise): libjpeg's reduced decode at 1/draft (F_LIBJPEG_SCALE_* on
    the flagged copies) -- what PIL's Image.draft() or OpenCV's IMREAD_REDUCED_* deliver, byte for byte, ceil(H / s) x ceil(W / s)."""
    _gray_layout(gray, planar)
    dflags = _draft_flags(draft)
    descs = _libjpeg(descs, libjpeg, draft=draft not in (False, None))
    if dflags:
        descs = [_copy_desc(d, pjd_amd.F_LIBJPEG_SCALE_MASK, dflags) for d in descs]
    sizes = None
    if orientations is not None:
        if len(orientations) != len(descs):
            raise ValueError("orientations: one entry per picture")
        sizes = [orient_hw(o, *output_hw(d)) for o, d in zip(orientations, descs)]
    fmt = pjd_amd.OUT_GRAY8 if gray else (pjd_amd.OUT_RGB8_PLANAR if planar else pjd_amd.OUT_RGB8)
    buf, offs, st = _run(ctx, _Request(descs, fmt, sizes=sizes, orientations=orientations), device)
    out = []
    nc = 1 if gray else 3
    for i, (d, off) in enumerate(zip(descs, offs)):
        h, w = output_hw(d) if sizes is None else sizes[i]
        flat = buf[off:off + nc * h * w]
        out.append(flat.view(nc, h, w) if planar else flat.view(h, w, 3))
    return out, st


def decode_to_batch_tensor(ctx, descs, device=None, libjpeg=False, gray=False):
    """Pictures of ONE output size -> (uint8 tensor [N, 3, H, W], statuses): picture i is bound at offset i * 3 * H * W, so the
    result is one contiguous NCHW tensor with no copy after the decode, complete on return and readable on any torch stream.
    ValueError (before anything is created) otherwise.  libjpeg=True: as in decode_to_tensors.  gray=True: [N, 1, H, W] (OUT_GRAY8),
    picture i at offset i * H * W."""
    descs = _libjpeg(descs, libjpeg)
    n, c, h, w = uniform_output_shape(descs)
    if gray:
        c = 1
    size = c * h * w
    buf, _, st = _run(ctx, _Request(descs, pjd_amd.OUT_GRAY8 if gray else pjd_amd.OUT_RGB8_PLANAR, n * size, [i * size for i in range(n)]), device)
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
    th, tw = size
    return [_scaled_copy(d, True, d.width, d.height, tw, th) for d in descs]


def center_crop_window(src_hw, resize_short, size):
    """torchvision's Resize(resize_short) followed by CenterCrop(size) of a picture of src_hw = (h, w), as the fields of a window over
    the whole picture: {"vw", "vh", "ox", "oy"}.  The short side becomes resize_short, the long one int(resize_short * long / short);
    ox, oy = int(round((v - t) / 2.0)) with Python's round-half-even, as torchvision.transforms.functional.center_crop has it.
    ValueError where the resized picture is smaller than size = (H, W) on an axis: there is no padding here.  Pure."""
    h, w = int(src_hw[0]), int(src_hw[1])
    rs, th, tw = int(resize_short), int(size[0]), int(size[1])
    if h < 1 or w < 1 or rs < 1 or th < 1 or tw < 1:
        raise ValueError("center_crop_window: sizes must be at least 1")
    if w <= h:
        vw, vh = rs, int(rs * h / w)
    else:
        vw, vh = int(rs * w / h), rs
    if vw < tw or vh < th:
        raise ValueError(f"center_crop_window: a {w}x{h} picture resized to {vw}x{vh} is smaller than the crop {tw}x{th} (no padding)")
    return {"vw": vw, "vh": vh, "ox": int(round((vw - tw) / 2.0)), "oy": int(round((vh - th) / 2.0))}


def window_at_scale(crop, log2s, sw, sh):
    """The crop (x, y, w, h), given in FULL-SIZE picture coordinates, at the decode scale s = 1 << log2s, where the picture is sw x sh:
    the hull [x >> log2s, ceil((x + w) / s)) x [y >> log2s, ceil((y + h) / s)), clipped to the scaled picture -> (x, y, w, h).  An
    approximation where s > 1: the box pre-scale comes first and its cells do not end at the crop's edges, so the result differs from a
    resize of the crop of the full-size picture (as prescale=True differs for antialias); s = 1 is exact.  Pure."""
    x, y, w, h = (int(v) for v in crop)
    log, sw, sh = int(log2s), int(sw), int(sh)
    if x < 0 or y < 0 or w < 1 or h < 1:
        raise ValueError("window_at_scale: crop (x, y, w, h) with x, y >= 0 and w, h >= 1")
    r = (1 << log) - 1
    x0, y0 = min(x >> log, sw - 1), min(y >> log, sh - 1)
    x1, y1 = min((x + w + r) >> log, sw), min((y + h + r) >> log, sh)
    return x0, y0, max(x1 - x0, 1), max(y1 - y0, 1)


def _tvh(o):
    """The bits (t, v, h) of an EXIF orientation 1..8: D = H^h(V^v(T^t(Q))) (include/pjd.h)."""
    o = int(o)
    if not 1 <= o <= 8:
        raise ValueError(f"an orientation is 1..8, not {o}")
    return ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0))[o - 1]


def orient_hw(o, h, w):
    """(h, w) of a picture of (h, w) after orientation o: swapped for 5..8.  Its own inverse: stored -> upright and back.  Pure."""
    return (int(w), int(h)) if _tvh(o)[0] else (int(h), int(w))


def orient_then_hflip(o):
    """The orientation that delivers the picture of orientation o mirrored left-right (RandomHorizontalFlip of the UPRIGHT picture): the
    mirror is the last step of D = H^h(V^v(T^t(Q))), so h ^= 1, which pairs 1 and 2, 3 and 4, 5 and 6, 7 and 8.  Pure."""
    _tvh(o)
    return ((int(o) - 1) ^ 1) + 1


def crop_to_stored(o, crop, W, H):
    """The crop (x, y, w, h), given in the UPRIGHT picture's coordinates, in the coordinates of the STORED picture of W x H, whose
    orientation is o: orient(S, o)[y:y+h, x:x+w] == orient(S[ys:ys+hs, xs:xs+ws], o).  The mirrors are undone in the upright frame, then
    the axes are swapped where o transposes -> (xs, ys, ws, hs).  ValueError where the crop is not inside the upright picture.  Pure."""
    t, v, hm = _tvh(o)
    x, y, w, h = (int(a) for a in crop)
    UH, UW = orient_hw(o, H, W)
    if x < 0 or y < 0 or w < 1 or h < 1 or x + w > UW or y + h > UH:
        raise ValueError(f"crop_to_stored: the crop {(x, y, w, h)} is not inside the upright {UW}x{UH} picture")
    if hm:
        x = UW - x - w
    if v:
        y = UH - y - h
    return (y, x, h, w) if t else (x, y, w, h)


def letterbox_plan(src_hw, size, mode="center"):
    """Where an upright picture of src_hw = (h, w) goes in a canvas of size = (H, W) with its aspect ratio kept: (content_h, content_w,
    left, top, right, bottom).  The side that limits fills the canvas, the other one is rounded to nearest (half up), at least 1 and at
    most the canvas: if w * H <= h * W the height limits, ch = H and cw = (2 * w * H + h) // (2 * h); else cw = W and
    ch = (2 * h * W + w) // (2 * w).  mode="center": left = (W - cw) // 2 and top = (H - ch) // 2, the odd column and row go right and
    below (YOLO's letterbox, "expand to square"); mode="topleft": left = top = 0 (DETR, SAM).  Integers only.  Pure."""
    h, w, H, W = int(src_hw[0]), int(src_hw[1]), int(size[0]), int(size[1])
    if h < 1 or w < 1 or H < 1 or W < 1:
        raise ValueError("letterbox_plan: sizes must be at least 1")
    if mode not in ("center", "topleft"):
        raise ValueError(f"letterbox_plan: mode must be \"center\" or \"topleft\", not {mode!r}")
    if w * H <= h * W:
        ch, cw = H, max(1, min(W, (2 * w * H + h) // (2 * h)))
    else:
        cw, ch = W, max(1, min(H, (2 * h * W + w) // (2 * w)))
    left, top = ((W - cw) // 2, (H - ch) // 2) if mode == "center" else (0, 0)
    return ch, cw, left, top, W - cw - left, H - ch - top


def _fill(fill, gray=False):
    """The `fill` keyword of the letterboxing helpers: three bytes; with gray=True one byte (a number or a sequence of length 1) will do."""
    fill = tuple(_gray3(fill, "fill") if gray else fill)
    if len(fill) != 3 or any(int(v) != v or not 0 <= int(v) <= 255 for v in fill):
        raise ValueError("fill: three bytes (R, G, B), each 0..255")
    return tuple(int(v) for v in fill)


def _pad_value(pad_value):
    """The `pad_value` keyword: None, one finite number for all three channels, or three."""
    import math
    if pad_value is None:
        return None
    vals = [float(pad_value)] * 3 if isinstance(pad_value, (int, float)) else [float(v) for v in pad_value]
    if len(vals) != 3 or not all(math.isfinite(v) for v in vals):
        raise ValueError("pad_value: one finite number, or three (R, G, B)")
    return vals


def _plan_outputs(descs, size, prescale, crops, flips, orientations, resize_short=None, letterbox=None):
    """The one planner of the resizing helpers -> (descriptors to decode, windows or None, orientations or None, pads or None), one entry
    per output.  crops, flips and orientations have one entry per output or are None; everything speaks about the UPRIGHT picture, and
    an absent orientation is orientation 1.  Per output: the crop is mapped into the stored picture (crop_to_stored); the centre crop
    of resize_short is worked out; with a letterbox the content size -- letterbox_plan of the upright picture, or of its crop --
    becomes the target; the pre-scale (prescale true, or "draft" for libjpeg's own) is picked from the crop's size (else the
    picture's) against Q's virtual target, the axes swapped for orientations 5..8; the window is taken at the scale the descriptor
    ended with.  A flip is RW_HFLIP in the window where no orientations were given, and folded into the orientation
    (orient_then_hflip) where they were.  A window holds x, y, w, h iff there is a crop and every other field iff it is not zero."""
    if letterbox not in (None, "center", "topleft"):
        raise ValueError(f"letterbox must be None, \"center\" or \"topleft\", not {letterbox!r}")
    if resize_short is not None and crops is not None:
        raise ValueError("crops and resize_short exclude each other")
    if resize_short is not None and letterbox is not None:
        raise ValueError("letterbox and resize_short exclude each other: one crops to the target, the other pads to it")
    for name, v in (("crops", crops), ("flips", flips), ("orientations", orientations)):
        if v is not None and len(v) != len(descs):
            raise ValueError(f"{name}: one entry per picture")
    th, tw = size
    run, windows, oris, pads = [], [], [], []
    for i, d in enumerate(descs):
        W, H = int(d.width), int(d.height)
        o = 1 if orientations is None else int(orientations[i])
        t = _tvh(o)[0]
        UW, UH = (H, W) if t else (W, H)                  # the upright picture; below, its crop where there is one
        win = {}
        crop = crops[i] if crops is not None else None
        if crop is not None:
            try:
                crop = crop_to_stored(o, crop, W, H)
            except ValueError:
                raise ValueError(f"crops[{i}] = {tuple(crop)}: (x, y, w, h) with w, h >= 1, inside the upright {UW}x{UH} picture "
                                 f"(the {W}x{H} one, orientation {o})")
            UW, UH = (crop[3], crop[2]) if t else (crop[2], crop[3])
        vw, vh = (th, tw) if t else (tw, th)              # Q's target: the delivered one with the axes swapped where o transposes
        if resize_short is not None:
            cc = center_crop_window((UH, UW), resize_short, size)
            vw, vh = (cc["vh"], cc["vw"]) if t else (cc["vw"], cc["vh"])
            ox, oy, _, _ = crop_to_stored(o, (cc["ox"], cc["oy"], tw, th), vw, vh)
            win.update(vw=vw, vh=vh, ox=ox, oy=oy)
        if letterbox is not None:
            ch, cw, left, top, right, bottom = letterbox_plan((UH, UW), size, letterbox)
            vw, vh = (ch, cw) if t else (cw, ch)
            pads.append((left, top, right, bottom))
        if prescale:
            sw, sh = crop[2:] if crop is not None else (W, H)
            d = _scaled_copy(d, prescale, sw, sh, vw, vh)
        if crop is not None:
            sh, sw = output_hw(d)
            win["x"], win["y"], win["w"], win["h"] = window_at_scale(crop, _scale_log(d.flags), sw, sh)
        flip = flips is not None and flips[i]
        if flip and orientations is None:
            win["flags"] = pjd_amd.RW_HFLIP
        run.append(d)
        windows.append({k: v for k, v in win.items() if v or k in ("x", "y", "w", "h")} or None)
        oris.append(orient_then_hflip(o) if flip else o)
    # windows that are all None are still set where the plain path was asked for any: a window array can select another resample kernel
    asked = orientations is None and letterbox is None and not (crops is None and flips is None and resize_short is None)
    return ((run if prescale else descs), (windows if asked or any(w is not None for w in windows) else None),
            (oris if orientations is not None else None), (pads if letterbox is not None else None))


def affine_inverse_matrix(src_hw, out_hw, angle=0, translate=(0, 0), scale=1, shear=(0, 0), center=None):
    """The inverse 2 x 3 matrix (m00, m01, m02, m10, m11, m12) that Batch.set_resize_affine and affines= take, for a picture of
    src_hw = (h, w) delivered as out_hw = (H, W): torchvision's affine -- rotate by `angle` degrees about `center`, shear by `shear` = (x, y)
    degrees, scale by `scale`, then translate by `translate` = (tx, ty) pixels -- with the centre of the output on the centre of the
    source.  A positive angle turns the picture COUNTER-CLOCKWISE, as torchvision.transforms.functional.rotate and RandomRotation have
    it; functional.affine and RandomAffine count clockwise, so their angle goes in negated (the matrix is functional's
    _get_inverse_affine_matrix(center, -angle, translate, scale, shear)).  center = (x, y) in the source picture's coordinates, origin
    at its top-left corner; None: its middle, (w / 2, h / 2).  The output frame is the source frame shifted so that the two middles
    coincide: out_hw == src_hw is torchvision's same-size output, out_hw = (w, h) with angle=90 is numpy.rot90(P, 1) exactly.  Angles
    that are multiples of 90 use exact sines.  Coordinates are at full size: the helpers divide by the decode scale.  Pure."""
    import math
    sh, sw = float(src_hw[0]), float(src_hw[1])
    oh, ow = float(out_hw[0]), float(out_hw[1])
    if min(sh, sw, oh, ow) < 1 or not float(scale) > 0:
        raise ValueError("affine_inverse_matrix: sizes of at least 1 and a scale above 0")
    shear = (shear, 0.0) if isinstance(shear, (int, float)) else tuple(shear)
    tx, ty = (float(v) for v in translate)
    cx, cy = (sw / 2, sh / 2) if center is None else (float(center[0]), float(center[1]))

    def cs(deg):                                           # exact at the quarter turns
        q, r = divmod(deg, 90.0)
        if r == 0:
            return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
        return math.cos(math.radians(deg)), math.sin(math.radians(deg))

    rot = -float(angle)
    sx, sy = float(shear[0]), float(shear[1])
    if math.cos(math.radians(sy)) == 0:
        raise ValueError("affine_inverse_matrix: a shear of 90 degrees has no matrix")
    c_rs, s_rs = cs(rot - sy)
    c_r, s_r = cs(rot)
    csy, tsx = math.cos(math.radians(sy)), math.tan(math.radians(sx))
    a, b = c_rs / csy, -c_rs * tsx / csy - s_r
    c, d = s_rs / csy, -s_rs * tsx / csy + c_r
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    # the output pixel at p (its own frame) lies at p - (ow / 2, oh / 2) + (sw / 2, sh / 2) of the source frame
    ox, oy = sw / 2 - ow / 2, sh / 2 - oh / 2
    m[2] = m[0] * (ox - cx - tx) + m[1] * (oy - cy - ty) + cx
    m[5] = m[3] * (ox - cx - tx) + m[4] * (oy - cy - ty) + cy
    return tuple(m)


def orientation_matrix(o, W, H):
    """The exact integer 2 x 3 matrix from the UPRIGHT picture's coordinates to those of the STORED picture of W x H whose EXIF
    orientation is o (pixel centres at +1/2, as everywhere): the mirrors undone in the upright frame, then the axes swapped where o
    transposes -- crop_to_stored for points.  With the identity as the map and the upright size as the target it is
    Batch.set_orientation's permutation.  Pure."""
    t, v, hm = _tvh(o)
    UH, UW = orient_hw(o, H, W)
    rx = (-1, 0, UW) if hm else (1, 0, 0)
    ry = (0, -1, UH) if v else (0, 1, 0)
    return (ry + rx) if t else (rx + ry)


def _compose(a, b):
    """the 2 x 3 map a after b"""
    return (a[0] * b[0] + a[1] * b[3], a[0] * b[1] + a[1] * b[4], a[0] * b[2] + a[1] * b[5] + a[2],
            a[3] * b[0] + a[4] * b[3], a[3] * b[1] + a[4] * b[4], a[3] * b[2] + a[4] * b[5] + a[5])


def plan_affines(descs, affines, prescale=True, orientations=None, views=None):
    """What the resizing helpers do with affines= -> (descriptors to decode, one per PICTURE; matrices for Batch.set_resize_affine, one
    per OUTPUT).  affines[i]: six values, or two rows of three: the inverse map of output i from its pixel centres to the FULL-SIZE
    picture's -- the UPRIGHT one where orientations are given: orientation_matrix is then multiplied in, exactly.  The pre-scale
    (prescale true: F_SCALE_*, "draft": F_LIBJPEG_SCALE_*) of a picture is the largest s of 8, 4, 2 for which both column norms of the
    matrix -- the source pixels one step along each target axis covers -- are at least s, the least reduced among a picture's views; else
    the descriptors' own flags hold.  Every matrix is then divided by the scale its picture is decoded at.  Pure."""
    import math
    pic_of = list(range(len(descs))) if views is None else _views(views, len(descs))
    for name, v in (("affines", affines), ("orientations", orientations)):
        if v is not None and len(v) != len(pic_of):
            raise ValueError(f"{name}: one entry per picture (per view with views=)")
    full = []
    for i, p in enumerate(pic_of):
        m = tuple(float(v) for row in affines[i] for v in (row if hasattr(row, "__len__") else (row,)))
        if len(m) != 6 or not all(math.isfinite(v) for v in m):
            raise ValueError(f"affines[{i}]: six finite values (m00, m01, m02, m10, m11, m12), or two rows of three")
        if orientations is not None:
            m = _compose(orientation_matrix(orientations[i], int(descs[p].width), int(descs[p].height)), m)
        full.append(m)
    run = list(descs)
    if prescale:
        draft = prescale == "draft"
        mask, low = (pjd_amd.F_LIBJPEG_SCALE_MASK, pjd_amd.F_LIBJPEG_SCALE_1_2) if draft else (pjd_amd.F_SCALE_MASK, pjd_amd.F_SCALE_1_2)
        logs = [3] * len(descs)                            # no view at all: 1/8, nothing reads the picture
        for m, p in zip(full, pic_of):
            shrink = min(math.hypot(m[0], m[3]), math.hypot(m[1], m[4]))
            logs[p] = min(logs[p], 3 if shrink >= 8 else 2 if shrink >= 4 else 1 if shrink >= 2 else 0)
        run = [_copy_desc(d, mask, log * low) for d, log in zip(descs, logs)]
    return run, [tuple(v / (1 << _scale_log(run[p].flags)) for v in m) for m, p in zip(full, pic_of)]


_LUMA = (0.299, 0.587, 0.114)
_YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))


def colour_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, grayscale=False, channel_order="rgb", pivot=128.0,
                  order=("brightness", "contrast", "saturation", "hue")):
    """The twelve numbers of a 3 x 4 colour map (row-major, the last column in 8-bit levels) for Batch.set_colour and colours=: the
    product of 4 x 4 homogeneous factors applied in `order` (a permutation of the four names; a factor at its neutral value is left out,
    so the defaults give the identity exactly):
      brightness b: b * x;
      contrast c: c * x + (1 - c) * pivot, about the CONSTANT `pivot`;
      saturation s: s * x + (1 - s) * L with L = 0.299 R + 0.587 G + 0.114 B;
      hue h: a rotation by h turns (h = 0.5: half a turn) about the grey axis in YIQ.
    Then grayscale=True puts L of the result in all three rows (RandomGrayscale: a grey picture of three equal channels), and
    channel_order="bgr" swaps the first and the last row, last of all.  Pure; float64.
    This is the model of DALI's color_twist / hsv / brightness_contrast.  It differs from torchvision's ColorJitter, which works on the
    pixels step by step: there is no clamp to 0..255 BETWEEN the factors (one clamp at the end); contrast pivots on a constant and not
    on the picture's mean grey (that needs a reduction over the picture); and torchvision truncates its grey to uint8 before it blends
    for saturation and contrast.  For small jitters the results are within a few levels of each other."""
    import numpy as np
    if sorted(order) != ["brightness", "contrast", "hue", "saturation"]:
        raise ValueError("colour_matrix: order is a permutation of (\"brightness\", \"contrast\", \"saturation\", \"hue\")")
    if channel_order not in ("rgb", "bgr"):
        raise ValueError("colour_matrix: channel_order is \"rgb\" or \"bgr\"")
    vals = [float(v) for v in (brightness, contrast, saturation, hue, pivot)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("colour_matrix: finite values")
    b, c, s, h, pivot = vals
    luma = np.tile(np.asarray(_LUMA, np.float64), (3, 1))
    m = np.eye(4)
    for name in order:
        f = np.eye(4)
        if name == "brightness" and b != 1.0:
            f[:3, :3] *= b
        elif name == "contrast" and c != 1.0:
            f[:3, :3] *= c
            f[:3, 3] = (1.0 - c) * pivot
        elif name == "saturation" and s != 1.0:
            f[:3, :3] = s * np.eye(3) + (1.0 - s) * luma
        elif name == "hue" and h != 0.0:
            t = np.asarray(_YIQ, np.float64)
            a = 2.0 * math.pi * h
            rot = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]])
            f[:3, :3] = np.linalg.inv(t) @ rot @ t
        else:
            continue
        m = f @ m
    if grayscale:
        g = np.eye(4)
        g[:3, :3] = luma
        m = g @ m
    if channel_order == "bgr":
        m = m[[2, 1, 0, 3]]
    return tuple(float(v) for v in m[:3].reshape(-1))


def tile_views(h, w, th, tw):
    """An h x w picture cut into a grid of tiles of at most th x tw, edge tiles smaller -> (windows, sizes), row-major (left to right,
    then top to bottom): windows[k] = {"x", "y", "w", "h"} for Batch.set_resize_window and sizes[k] = (tile_h, tile_w) for
    Batch.set_resize, ceil(h / th) * ceil(w / tw) of each.  Every target equals its window, so every tap weight of every filter is the
    identity and the tiles put side by side are the decoded picture byte for byte.  With Batch.set_views([p] * len(sizes)) one picture
    leaves its one decode as its tiles.  Pure."""
    h, w, th, tw = int(h), int(w), int(th), int(tw)
    if h < 1 or w < 1 or th < 1 or tw < 1:
        raise ValueError("tile_views: sizes must be at least 1")
    windows, sizes = [], []
    for y in range(0, h, th):
        for x in range(0, w, tw):
            ww, hh = min(tw, w - x), min(th, h - y)
            windows.append({"x": x, "y": y, "w": ww, "h": hh})
            sizes.append((hh, ww))
    return windows, sizes


def least_reduced_scale_flags(flags_of_views, draft=False):
    """The pre-scale of a picture that has several views: the LEAST reduced of the scales its views picked for themselves
    (pick_scale_flags / pick_libjpeg_scale_flags of each view's window against its target) -- the view with the largest target against
    its window decides, and no view is resampled up from a picture decoded too small for it.  flags_of_views: the F_SCALE_* values
    (draft: F_LIBJPEG_SCALE_*) of the views, other bits ignored.  No view at all: 1/8, nothing reads the picture.  Pure."""
    mask, low = (pjd_amd.F_LIBJPEG_SCALE_MASK, pjd_amd.F_LIBJPEG_SCALE_1_2) if draft else (pjd_amd.F_SCALE_MASK, pjd_amd.F_SCALE_1_2)
    logs = [(int(f) & mask) // low for f in flags_of_views]
    return (min(logs) if logs else 3) * low


def _views(views, n_pictures):
    """The `views` keyword, checked before anything is created -> list of ints."""
    views = [int(p) for p in views]
    if len(views) == 0:
        raise ValueError("views: at least one view")
    for v, p in enumerate(views):
        if not 0 <= p < n_pictures:
            raise ValueError(f"views[{v}] = {p}: the batch has {n_pictures} pictures")
    return views


def plan_views(descs, views, size, prescale=True, crops=None, flips=None, resize_short=None, orientations=None, letterbox=None):
    """What the resizing helpers do with views=: -> (descriptors to decode, one per PICTURE; windows, orientations, pads, one per VIEW or
    None).  crops, flips, orientations have one entry per view and speak about that view's picture, exactly as they speak about picture i
    without views.  The pre-scale (prescale true, or "draft" for libjpeg's own) is chosen per PICTURE: each view picks as a picture of
    its own would, the least reduced of a picture's views wins (least_reduced_scale_flags), and every view's window is then taken at
    THAT scale (window_at_scale).  Pure: no device, no torch."""
    views = _views(views, len(descs))

    def plan(pics, ps):
        return _plan_outputs([pics[p] for p in views], size, ps, crops, flips, orientations, resize_short, letterbox)

    pics = list(descs)
    if prescale:
        draft = prescale == "draft"
        mask = pjd_amd.F_LIBJPEG_SCALE_MASK if draft else pjd_amd.F_SCALE_MASK
        picked = plan(descs, prescale)[0]                  # every view as a picture of its own
        pics = [_copy_desc(d, mask, least_reduced_scale_flags([picked[v].flags for v in range(len(views)) if views[v] == p], draft))
                for p, d in enumerate(descs)]
    return (pics,) + plan(pics, False)[1:]                 # the windows at the scale the pictures are decoded at


def _resize_request(who, descs, size, out_format, prescale, antialias, crops, flips, resize_short, interpolation, orientations, libjpeg,
                    letterbox, fill, draft, views, affines=None, colours=None, blurs=None):
    """The _Request of one of the two resizing helpers (`who`): its geometry (_resize_request_geometry), and colours= checked against it
    -- one map or None per output, none on a grey batch -- before anything is created; blurs= likewise -- one (ksize, sigma) or None per
    output, none beside letterbox=."""
    req = _resize_request_geometry(who, descs, size, out_format, prescale, antialias, crops, flips, resize_short, interpolation, orientations, libjpeg,
                                   letterbox, fill, draft, views, affines)
    if blurs is not None:
        if letterbox is not None:
            raise ValueError(f"{who}: blurs= excludes letterbox= (the border is not content; Batch.set_blur)")
        if len(blurs) != len(req.sizes):
            raise ValueError(f"{who}: blurs= has one (ksize, sigma) (or None) per output: {len(req.sizes)}, not {len(blurs)}")
        req = req._replace(blurs=[None if e is None else (int(e[0]), float(e[1])) for e in blurs])
    if colours is None:
        return req
    if out_format == pjd_amd.OUT_GRAY8:
        raise ValueError(f"{who}: colours= takes gray=False (one plane has no colour map; grayscale=True of colour_matrix makes a grey RGB picture)")
    if len(colours) != len(req.sizes):
        raise ValueError(f"{who}: colours= has one matrix (or None) per output: {len(req.sizes)}, not {len(colours)}")
    return req._replace(colours=[None if m is None else tuple(float(v) for row in m for v in (row if hasattr(row, "__len__") else (row,))) for m in colours])


def _resize_request_geometry(who, descs, size, out_format, prescale, antialias, crops, flips, resize_short, interpolation, orientations, libjpeg,
                             letterbox, fill, draft, views, affines=None):
    """What the two resizing helpers (`who`) share, all of it before anything is created: the keywords are checked, the outputs are
    planned (_plan_outputs, plan_views) -> the _Request of a batch of uint8 outputs of `size`, one after the other in one buffer."""
    if interpolation not in ("bilinear", "bicubic"):
        raise ValueError(f"interpolation must be \"bilinear\" or \"bicubic\", not {interpolation!r}")
    if len(descs) == 0:
        raise ValueError(f"{who}: no pictures")
    descs = _libjpeg(descs, libjpeg, prescale, draft)
    prescale = "draft" if draft else prescale
    th, tw = int(size[0]), int(size[1])
    gray = out_format == pjd_amd.OUT_GRAY8
    fill = _fill(fill, gray)
    if affines is not None:
        # the map is the whole geometry: each of these is a matrix the caller multiplies in (affine_inverse_matrix, orientation_matrix)
        for name, given in (("crops", crops is not None), ("flips", flips is not None), ("resize_short", resize_short is not None), ("letterbox", letterbox is not None),
                            ("antialias", bool(antialias)), ("interpolation", interpolation != "bilinear")):
            if given:
                raise ValueError(f"{who}: affines= excludes {name}= (fold it into the matrix; the warp is bilinear)")
        views = None if views is None else _views(views, len(descs))
        run, mats = plan_affines(descs, affines, prescale, orientations, views)
        n, plane = len(mats), (1 if gray else 3) * th * tw
        return _Request(run, out_format, n * plane, [i * plane for i in range(n)], views, [(th, tw)] * n, fill=fill, affines=mats)
    if views is not None:
        views = _views(views, len(descs))
        run, windows, oris, pads = plan_views(descs, views, (th, tw), prescale, crops, flips, resize_short, orientations, letterbox)
    else:
        run, windows, oris, pads = _plan_outputs(descs, (th, tw), prescale, crops, flips, orientations, resize_short, letterbox)
    n, plane = (len(descs) if views is None else len(views)), (1 if gray else 3) * th * tw
    filter = pjd_amd.RESIZE_BICUBIC if interpolation == "bicubic" else pjd_amd.RESIZE_ANTIALIAS if antialias else None
    return _Request(run, out_format, n * plane, [i * plane for i in range(n)], views, [(th, tw)] * n, pads, fill, oris, windows, filter)


def decode_resized_batch_tensor(ctx, descs, size, prescale=True, device=None, antialias=False, crops=None, flips=None, resize_short=None,
                                interpolation="bilinear", orientations=None, libjpeg=False, letterbox=None, fill=(0, 0, 0), gray=False, draft=False,
                                views=None, affines=None, colours=None, blurs=None):
    """Pictures of ANY sizes -> (uint8 tensor [N, 3, H, W], statuses), size = (H, W): every picture is resampled to H x W inside
    the decode (the bilinear filter of include/pjd.h, pjd_batch_set_resize) and lands at offset i * 3 * H * W of one buffer, so
    the result is one contiguous NCHW tensor with no copy after the decode, complete on return and readable on any torch stream
    (module docstring, "Stream order").  prescale: decode copies of the descriptors at the reduced size pick_scale_flags chooses
    (the box filter takes the bulk of a large reduction: no aliasing, and less to decode); else the descriptors' own flags hold.
    antialias=True: the resize is the antialiased triangle filter of include/pjd.h (Batch.set_resize_filter) -- what
    torch.nn.functional.interpolate(mode="bilinear", antialias=True), torchvision's Resize(antialias=True) and Pillow's BILINEAR
    compute, to within 1 level.  With prescale=True the box pre-scale is still chosen (less to decode; the triangle filter removes
    what the box leaves), so the result differs from an antialiased resize of the full-size picture; prescale=False gives exactly
    that, for pictures up to 16x the target on each axis (beyond that the call raises).
    crops=[(x, y, w, h) | None, ...]: picture i is that crop of the FULL-SIZE picture resized to H x W (what
    RandomResizedCrop.get_params returns: x = left, y = top); flips=[bool, ...]: mirrored left-right; resize_short=int: torchvision's
    Resize(int) + CenterCrop(size) (center_crop_window; ValueError where the resized picture is smaller than size).  All three ride in
    the one resample launch (Batch.set_resize_window); the picture is decoded whole.  With prescale=False the result is exactly the
    filter of include/pjd.h over the crop of the full-size picture; with prescale=True the pre-scale is chosen from the crop's size
    and the crop becomes window_at_scale's hull of it, an approximation in the same sense as for antialias above.
    interpolation="bicubic": the bicubic filter of include/pjd.h (RESIZE_BICUBIC: Keys' cubic with a = -0.5 -- Pillow's BICUBIC,
    torch.nn.functional.interpolate(mode="bicubic", antialias=True), the default of timm's ViT-family transforms -- to within 1
    level of the float64 filter).  It is always the widened form where an axis shrinks: `antialias` is not consulted.  With
    prescale=True the box filter still comes first (less to decode), so the result is the bicubic filter over the box-filtered
    picture; prescale=False is exactly the filter over the full-size picture, for pictures up to 16x the target on each axis.  Any
    other string than "bilinear" (the default) or "bicubic" raises ValueError before anything is created.
    orientations=[1..8, ...] (Scanned.orientation): the pictures are delivered upright (Batch.set_orientation: D = H^h(V^v(T^t(Q))) of
    include/pjd.h, in the same launch), and crops, resize_short and flips speak about the UPRIGHT picture: crops are mapped with
    crop_to_stored, the centre crop is computed from the upright size, flips are folded into the orientation (orient_then_hflip).  The
    picture is resampled in the stored picture's coordinates and permuted on the way out, which is within each filter's one-level
    bound of "orient, then resize".  None: today's behaviour, byte for byte.
    libjpeg=True: the picture the filters read is libjpeg's, byte for byte (F_LIBJPEG on copies of the descriptors): what a PIL or
    torchvision.io pipeline resizes.  It takes prescale=False (ValueError before anything is created otherwise): the box pre-scale is
    not libjpeg's reduced decode.  draft=True (only with libjpeg=True, ValueError otherwise) IS that reduced decode: every flagged copy
    is decoded at the scale pick_libjpeg_scale_flags chooses for it (F_LIBJPEG_SCALE_*: libjpeg's reduced IDCTs, what Image.draft() and
    the loaders built on it do before they resize) and the filters read that reduced picture; crops become window_at_scale's hull.
    letterbox="center" | "topleft": every picture keeps its aspect ratio inside the H x W canvas (letterbox_plan of the UPRIGHT picture,
    or of its crop) and the rest of the canvas is `fill` (three bytes; YOLO: 114) -- Batch.set_resize_pad, in the same launch and one
    small one behind it.  crops and orientations work as above against the content size, flips mirror the content inside its
    rectangle, the pre-scale is picked from the content size; resize_short is excluded (ValueError).  None: today's behaviour.
    gray=True: uint8 [N, 1, H, W] (OUT_GRAY8: the luma plane -- with libjpeg=True what libjpeg's JCS_GRAYSCALE delivers -- through the same
    filters: channel 0 of what they make of the picture with neutral chroma); every other keyword composes as without it, and `fill` may
    be one byte.
    views=[picture index, ...] of length V (Batch.set_views): the result is [V, C, H, W], view v a resample of picture views[v] -- any
    order, any number of views of a picture, none included -- and every picture is decoded ONCE.  crops, flips and orientations then have V
    entries (entry v speaks about picture views[v] as entry i speaks about picture i without views); resize_short and letterbox apply to
    every view.  The statuses stay per picture.  The pre-scale of a picture is the least reduced of what its views would pick
    (plan_views).  None: nothing changes.
    affines=[(m00, m01, m02, m10, m11, m12), ...]: output i is the picture under that INVERSE map, from the centres of the H x W target's
    pixels to those of the FULL-SIZE stored picture (affine_inverse_matrix makes it from an angle, a translation, a scale and a shear:
    RandomRotation, RandomAffine), bilinear in the fixed point of include/pjd.h (Batch.set_resize_affine), with `fill` wherever a tap
    lies outside the picture -- one launch, no grid_sample pass.  With orientations= the map speaks about the UPRIGHT picture and the
    exact orientation matrix is multiplied in (plan_affines); with views= there is one matrix per view.  prescale=True decodes a picture
    at the largest box scale that every one of its maps shrinks by; prescale=False is exactly the filter over the full-size picture.
    crops, flips, resize_short, letterbox, antialias and interpolation raise ValueError beside it: each is a matrix to fold in.
    colours=[m | None, ...]: output i's resampled 8-bit triple goes through the 3 x 4 colour map m (twelve values, row-major, the last
    column in 8-bit levels: colour_matrix makes them; None: the identity) inside the same launch, in the fixed point of include/pjd.h
    (Batch.set_colour): ColorJitter, RandomGrayscale, BGR.  One entry per OUTPUT (per view with views=).  It composes with every keyword
    above; a letterbox border keeps its `fill`, the `fill` of affines= passes through the map.  With gray=True it raises ValueError.
    blurs=[(ksize, sigma) | None, ...]: output i leaves as the separable Gaussian of what it would be without the keyword -- ksize odd, up
    to 63, the taps, the reflect border and the fixed point of include/pjd.h (Batch.set_blur; one more launch behind the resample):
    torchvision's GaussianBlur on the uint8 tensor to within 1 level, NOT Pillow's ImageFilter.GaussianBlur, which is a box approximation.
    One entry per OUTPUT (per view with views=); None: that output is not blurred.  It comes behind colours= and composes with every
    keyword above but letterbox=, beside which it raises ValueError, as it does for a wrong count."""
    req = _resize_request("decode_resized_batch_tensor", descs, size, pjd_amd.OUT_GRAY8 if gray else pjd_amd.OUT_RGB8_PLANAR, prescale, antialias,
                          crops, flips, resize_short, interpolation, orientations, libjpeg, letterbox, fill, draft, views, affines, colours, blurs)
    buf, _, st = _run(ctx, req, device)
    return buf.view(len(req.sizes), 1 if gray else 3, *req.sizes[0]), st


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
                                   antialias=False, crops=None, flips=None, resize_short=None, interpolation="bilinear", orientations=None,
                                   libjpeg=False, letterbox=None, fill=(0, 0, 0), pad_value=None, gray=False, draft=False, views=None, affines=None,
                                   colours=None, blurs=None):
    """Pictures of ANY sizes -> (tensor of `dtype` [N, 3, H, W], statuses), size = (H, W); dtype torch.float16 (the default),
    torch.bfloat16 or torch.float32.  As decode_resized_batch_tensor, and every sample v of channel c leaves the same launch as
    fma(v, scale[c], bias[c]) with the constants of normalize_constants(mean, std), converted once to `dtype` (include/pjd.h,
    pjd_batch_set_normalize): what x.float().div(255).sub(mean).div(std).to(dtype) makes of the uint8 tensor, which never exists.
    channels_last=False: one contiguous NCHW tensor.  channels_last=True: the batch is decoded interleaved into an [N, H, W, 3] buffer
    and the result is its permute(0, 3, 1, 2) view: shape [N, 3, H, W] in torch's channels_last memory format.  Complete on return and
    readable on any torch stream (module docstring, "Stream order").  antialias=True: the antialiased filter, as in
    decode_resized_batch_tensor -- with prescale=True the result differs from an antialiased resize of the full-size picture (the box
    pre-scale comes first), prescale=False gives exactly that up to the 16x limit.  crops, flips, resize_short: as in
    decode_resized_batch_tensor.  interpolation="bicubic": the bicubic filter (RESIZE_BICUBIC), as there -- `antialias` is not consulted,
    prescale=True still puts the box filter first, prescale=False is exactly the filter over the full-size picture up to the 16x
    limit; any other string than "bilinear" or "bicubic" raises ValueError before anything is created.  orientations, libjpeg, draft: as in
    decode_resized_batch_tensor.  letterbox, fill: as there; the border is normalised like every other sample (fill=(124, 116, 104) is
    about the ImageNet mean colour), unless pad_value -- one number or three -- is given: the border elements are then exactly that
    (Batch.set_pad_value; pad_value=0 is "zeros after normalisation": DETR, SAM).  pad_value without letterbox raises ValueError.
    gray=True: [N, 1, H, W] of `dtype` (OUT_GRAY8): fma(v, scale[0], bias[0]) of the luma plane; mean and std may be one number or a
    sequence of length 1, fill and pad_value one number; it takes channels_last=False (one plane has no interleaved form).
    views: as in decode_resized_batch_tensor -- [V, C, H, W] of `dtype` (channels_last: the permuted view of [V, H, W, 3]), per-view crops,
    flips and orientations, per-picture statuses, every picture decoded once.
    affines, with fill: as in decode_resized_batch_tensor; the fill is a sample like any other and is normalised with the rest (there is
    no pad_value beside it: that needs a letterbox).
    colours: as in decode_resized_batch_tensor; the map comes BEFORE the normalisation, which reads its 8-bit result -- the order of
    ColorJitter, RandomGrayscale, ToTensor, Normalize.
    blurs: as in decode_resized_batch_tensor; the normalisation reads the blurred byte -- ColorJitter, RandomGrayscale, GaussianBlur,
    ToTensor, Normalize, the order of the SimCLR family."""
    _gray_layout(gray, not channels_last)
    if gray:
        mean, std = _gray3(mean, "mean"), _gray3(std, "std")
        pad_value = None if pad_value is None else _gray3(pad_value, "pad_value")
    scale, bias = normalize_constants(mean, std)
    pad_value = _pad_value(pad_value)
    if pad_value is not None and letterbox is None:
        raise ValueError("pad_value needs letterbox: without it there is no border")
    req = _resize_request("decode_normalized_batch_tensor", descs, size, pjd_amd.OUT_GRAY8 if gray else pjd_amd.OUT_RGB8 if channels_last else pjd_amd.OUT_RGB8_PLANAR,
                          prescale, antialias, crops, flips, resize_short, interpolation, orientations, libjpeg, letterbox, fill, draft, views, affines, colours, blurs)
    torch = _torch()
    dtype = torch.float16 if dtype is None else dtype
    dts = {torch.float16: (pjd_amd.DT_F16, 2), torch.bfloat16: (pjd_amd.DT_BF16, 2), torch.float32: (pjd_amd.DT_F32, 4)}
    if dtype not in dts:
        raise ValueError("decode_normalized_batch_tensor: dtype must be torch.float16, torch.bfloat16 or torch.float32")
    dt, es = dts[dtype]
    req = req._replace(capacity=req.capacity * es, offsets=[o * es for o in req.offsets], normalize=(dt, scale, bias), pad_value=pad_value)
    buf, _, st = _run(ctx, req, device)
    n, (th, tw) = len(req.sizes), req.sizes[0]
    t = buf.view(dtype)
    return (t.view(n, th, tw, 3).permute(0, 3, 1, 2) if channels_last else t.view(n, 1 if gray else 3, th, tw)), st
