"""The cases of test_gpu_giant.py, each run in a process of its own:

    python giant_torch_cases.py <case> [arguments]

As tests/libjpeg_corpus_torch_cases.py: torch is imported, and touches the device, before anything of pjd_amd, so that torch and
libpjd.so use ONE HIP runtime.  Prints "CASE OK <case>" at the end; any failed assertion ends the process with a traceback.

Every case compares EVERY byte, on the device: the output is bound to a torch uint8 buffer filled with 0xA5 with 4096 guard bytes on
either side, at base + 1 where the elements are bytes; a giant's rows are compared, a thousand at a time, with the rows gathered from
the two period expectations of tests/giant_corpus.py (and the rows of the marked segments once more on the host against
giant_corpus.expected_rows), and the guard bytes must still be 0xA5.  Nothing expected is something this library delivered, but for the
small pictures behind a giant, which are held to their own decode in a batch of their own (what other suites hold to the oracle).  A
line "MEASURE ..." per decode records what profiles/size_limits.md holds."""
import torch                                                      # first: see above

assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

import ctypes as C                                                # noqa: E402
import os                                                         # noqa: E402
import sys                                                        # noqa: E402
import time                                                       # noqa: E402

import numpy as np                                                # noqa: E402

T_START = time.time()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "pim-jpeg-decoder_amd", "python"))

import giant_corpus as GC                                         # noqa: E402
import oracle_lib                                                 # noqa: E402
import pjd_amd                                                    # noqa: E402

GUARD = 4096
FILL = 0xA5
TWO32 = 1 << 32
DEV = "cuda:0"
FMT = {"rgb8": pjd_amd.OUT_RGB8, "bmp": pjd_amd.OUT_BMP, "planar": pjd_amd.OUT_RGB8_PLANAR, "gray": pjd_amd.OUT_GRAY8}
CHUNK = 1024      # rows compared at a time


def golden_bytes(name):
    with open(os.path.join(HERE, "golden", name + ".jpg"), "rb") as f:
        return f.read()


def scan(data, flags=0):
    s = pjd_amd.Scanned(data)
    assert s.valid, s.log
    s.desc.flags = int(s.desc.flags) | flags
    return s


def measure(what, **kw):
    print("MEASURE", what, " ".join(f"{k}={v}" for k, v in kw.items()), f"wall_s={time.time() - T_START:.1f}", flush=True)


# ---- a guarded buffer --------------------------------------------------------------------------------------------------------------------
class Guarded:
    """`size` bytes of 0xA5 between two guards of 4096 bytes, the payload at base + 1 (`align` 1) or at the aligned base + 4096"""

    def __init__(self, size, align=1):
        self.off = GUARD + (1 if align == 1 else 0)
        self.size = size
        self.buf = torch.full((self.off + size + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 256 == 0

    def refill(self):
        self.buf.fill_(FILL)
        torch.cuda.synchronize()

    @property
    def payload(self):
        return self.buf[self.off:self.off + self.size]

    def bind(self, b, offsets=(0,)):
        b.bind_output(self.buf.data_ptr(), self.buf.numel(), [self.off + o for o in offsets])

    def guards_intact(self, what):
        for part in (self.buf[:self.off], self.buf[self.off + self.size:]):
            assert bool((part == FILL).all()), (what, "a guard byte was written")


def same_on_device(got, want, what):
    """two device tensors of one shape, first dimension rows"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want).flatten(1).any(1).nonzero().flatten()
    row = int(bad[0])
    col = int((got[row] != want[row]).flatten().nonzero()[0])
    raise AssertionError((what, "rows differing", int(bad.numel()), "first", row, "at element", col,
                          "got", got[row].flatten()[col].item(), "want", want[row].flatten()[col].item()))


# ---- the expected rows of a giant, gathered on the device --------------------------------------------------------------------------------
class Expect:
    def __init__(self, name, flags, gray=False):
        self.name, self.flags, self.gray = name, flags, gray
        self.w, self.h = GC.spec(name)[0], GC.height(name)
        per = GC.seg_rows(GC.spec(name)[2])
        main, alt = GC.period_expected(GC._base(name), flags, gray)
        parts = [main, alt]
        y = np.arange(self.h, dtype=np.int64)
        r = y // per
        index = (r % 8) * per + y % per + np.where(np.isin(r, GC.marks(name)), main.shape[0], 0)
        self.status = 0
        if name == GC.FULL_ERR:
            self.status, last = GC.full_err_expected()
            parts.append(last)
            index = np.where(r == GC.n_segments(name) - 1, 2 * main.shape[0] + y % per, index)
        self.src = torch.from_numpy(np.concatenate(parts)).to(DEV)
        self.index = torch.from_numpy(index).to(DEV)
        self.planes = None

    def rows(self, y0, y1):
        """[y1 - y0, W, 3], or [y1 - y0, W] for grey"""
        return self.src[self.index[y0:y1]]

    def plane_rows(self, c, y0, y1):
        if self.planes is None:
            self.planes = self.src.permute(2, 0, 1).contiguous()
        return self.planes[c][self.index[y0:y1]]

    def check(self, payload, fmt, what):
        """every byte of the picture in `payload` (a device tensor of the picture's bytes)"""
        w, h = self.w, self.h
        assert payload.numel() == GC.out_bytes(w, h, fmt)
        for y0 in range(0, h, CHUNK):
            y1 = min(h, y0 + CHUNK)
            if fmt == "rgb8":
                same_on_device(payload.view(h, w, 3)[y0:y1], self.rows(y0, y1), (what, fmt, "rows from", y0))
            elif fmt == "gray":
                same_on_device(payload.view(h, w)[y0:y1], self.rows(y0, y1), (what, fmt, "rows from", y0))
            else:
                for c in range(3):
                    same_on_device(payload.view(3, h, w)[c, y0:y1], self.plane_rows(c, y0, y1), (what, fmt, "plane", c, "rows from", y0))

    def check_marked_on_host(self, payload, fmt, what):
        """the rows of the marked segments against giant_corpus.expected_rows: ties the gather above to the corpus's own definition"""
        w, h = self.w, self.h
        per = GC.seg_rows(GC.spec(self.name)[2])
        for r in GC.marks(self.name):
            y0, y1 = r * per, min(h, (r + 1) * per)
            want = GC.expected_rows(self.name, y0, y1, self.flags, self.gray)
            if fmt == "rgb8":
                got = payload.view(h, w, 3)[y0:y1].cpu().numpy()
            elif fmt == "gray":
                got = payload.view(h, w)[y0:y1].cpu().numpy()
            else:
                got = payload.view(3, h, w)[:, y0:y1].cpu().numpy().transpose(1, 2, 0)
            assert np.array_equal(got, want), (what, fmt, "marked segment", r)


def assert_lane_path(info, what):
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0 and sum(info["flag_waves"]) == 0, (what, info)


# ---- 1: the back ends ----------------------------------------------------------------------------------------------------------------------
def largest_offset(w, h, fmt):
    return max(int(first.max()) + n for first, n in GC.row_offsets(w, h, fmt)) - 1


def run_bound(c, s, name, flags, fmt, exp=None, status=0, lane_path=True):
    """decode twice, then replay a captured graph once; every byte compared after each"""
    exp = exp or Expect(name, flags, fmt == "gray")
    w, h = exp.w, exp.h
    with c.batch([s.desc], FMT[fmt]) as b:
        size = b.output_size(0)
        assert size == GC.out_bytes(w, h, fmt)
        g = Guarded(size)
        g.bind(b)
        b.upload()
        info = None
        for rep in ("first", "second", "replay"):
            what = (name, flags, fmt, rep)
            if rep == "first":
                timings, total_ms = b.decode_timed()
            else:
                if rep == "replay":
                    b.capture()
                g.refill()
                b.decode()
            b.sync()
            got_status = b.statuses()
            assert got_status == [status], (what, got_status, status)
            exp.check(g.payload, fmt, what)
            g.guards_intact(what)
            if rep == "first":
                exp.check_marked_on_host(g.payload, fmt, what)
                info = b.info()
                measure(f"{name}:{flags}:{fmt}", first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"] + g.buf.numel(),
                        largest_offset=largest_offset(w, h, fmt))
        info = b.info()
        if lane_path:
            assert_lane_path(info, (name, flags, fmt))
    del g
    torch.cuda.empty_cache()
    return info


def bmp_header(w, h):
    """the reference's 26 bytes (src/bmp_writer.cpp): a BITMAPCOREHEADER, the file size taken mod 2^32"""
    size = (26 + h * (3 * w + w % 4)) % TWO32
    head = np.zeros(26, np.uint8)
    head[0], head[1] = ord("B"), ord("M")
    head[2:6] = np.frombuffer(size.to_bytes(4, "little"), np.uint8)
    head[10], head[14] = 0x1A, 12
    head[18:20] = np.frombuffer(w.to_bytes(2, "little"), np.uint8)
    head[20:22] = np.frombuffer(h.to_bytes(2, "little"), np.uint8)
    head[22], head[24] = 1, 24
    return head


def run_bmp(c, s, name, flags):
    """BMP cannot be bound: the picture comes through download_packed into page-locked memory (one copy: 4.8 GB of host memory), and
    goes back to the device a thousand rows at a time for the comparison"""
    exp = Expect(name, flags)
    w, h = exp.w, exp.h
    stride = 3 * w + w % 4
    L = c.L
    with c.batch([s.desc], pjd_amd.OUT_BMP) as b:
        size, pic = b.packed_size(), GC.out_bytes(w, h, "bmp")
        assert b.output_size(0) == pic > TWO32 and b.output_offset(0) == 0
        assert size >= pic and size - pic < 256                   # the packed size is rounded up to 256 bytes
        b.upload()
        host = L.pjd_host_alloc(size)
        assert host
        try:
            whole = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint8)), shape=(size,))
            for rep in ("first", "second", "replay"):
                what = (name, flags, "bmp", rep)
                if rep == "first":
                    timings, total_ms = b.decode_timed()
                else:
                    if rep == "replay":
                        b.capture()
                    b.decode()
                b.sync()
                whole[:] = FILL
                st = (C.c_int32 * 1)()
                c._check(L.pjd_batch_download_packed(b._h, host, size, st), "pjd_batch_download_packed")
                assert int(st[0]) == 0, what
                assert np.array_equal(whole[:26], bmp_header(w, h)), (what, whole[:26].tolist())
                body = whole[26:pic].reshape(h, stride)
                assert not whole[pic:].any(), (what, "bytes behind the picture: the batch's own buffer is zeroed")
                for k0 in range(0, h, CHUNK):                       # file rows: bottom-up
                    k1 = min(h, k0 + CHUNK)
                    got = torch.from_numpy(body[k0:k1]).to(DEV)
                    want = exp.rows(h - k1, h - k0).flip(0).flip(2)      # picture rows h-1-k, B G R
                    same_on_device(got[:, :3 * w].reshape(k1 - k0, w, 3), want, (what, "file rows from", k0))
                    assert bool((got[:, 3 * w:] == 0).all()), (what, "row padding", k0)
                if rep == "first":
                    info = b.info()
                    measure(f"{name}:{flags}:bmp", first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"],
                            largest_offset=largest_offset(w, h, "bmp"))
            assert_lane_path(b.info(), (name, flags, "bmp"))
        finally:
            L.pjd_host_free(host)


def case_backend(member, flags, fmts):
    """One member under one flag set in the listed formats."""
    flags = int(flags)
    assert flags in GC.spec(member)[6]
    s = scan(GC.jpeg(member), flags)
    measure(f"{member}:built")
    c = pjd_amd.Context(0)
    for fmt in fmts.split(","):
        assert fmt in GC.spec(member)[7]
        if fmt == "bmp":
            run_bmp(c, s, member, flags)
        else:
            run_bound(c, s, member, flags, fmt)
    c.close()


# ---- 3: the stream limit -------------------------------------------------------------------------------------------------------------------
def case_stream_limit():
    """g444_full in rgb8: ecs_len == 2^29 - 1, the last segment's base_bit above 2^32 - 2^22, the last unit above 2^32 - 2^21."""
    s = scan(GC.jpeg(GC.FULL))
    assert int(s.desc.ecs_len) == GC.ECS_CAP
    measure("g444_full:built")
    c = pjd_amd.Context(0)
    info = run_bound(c, s, GC.FULL, 0, "rgb8", lane_path=False)
    c.close()
    # the zero bytes behind the last MCU never self-synchronise: their waves end flagged (PJD_FLAG_STITCH), behind the picture's last
    # unit, where a flag does not count (PjdDevImState::end_pos) -- every other reason stays 0 and nothing goes to the exact kernel
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0, info
    assert [n for r, n in enumerate(info["flag_waves"]) if r != 3] == [0] * 7, info


def case_padded_tail():
    """What sent g444_full to the exact kernel before end_pos, at a size where that costs nothing: 203 x 213 with 180 000 zero bytes
    between the last MCU and the EOI (22 waves of lanes that never synchronise: PJD_FLAG_STITCH, measured in 18 of them) decodes on
    the lane path, to the port's picture and coefficients."""
    port = oracle_lib.Port()
    w, h, per = 203, 213, 8
    main = GC.synth.make(w, 64, 7301, 85, GC.S444, 26, 1.0)
    alt = GC.synth.make(w, 64, 7351, 85, GC.S444, 26, 1.0)
    n = -(-h // per)
    plain = GC.splice(main, h, (0, n - 1), alt)
    data_len = int(pjd_amd.Scanned(plain).desc.ecs_len)
    c = pjd_amd.Context(0)
    for pad in (0, 2000, 180000):
        j = GC.splice(main, h, (0, n - 1), alt, pad_to=data_len + pad)
        want = port.decode(j)
        assert want["huff_rc"] == 0 and np.array_equal(want["rgb"], port.decode(plain)["rgb"])
        s = scan(j)
        assert int(s.desc.ecs_len) == data_len + pad
        with c.batch([s.desc], pjd_amd.OUT_RGB8) as b:
            b.upload()
            b.decode(); b.sync()
            outs, st = b.download()
            info = b.info()
            assert st == [0] and np.array_equal(outs[0], want["rgb"]), pad
            assert info["n_sequential"] == 0 and info["n_fallback"] == 0, (pad, info)
            assert [k for r, k in enumerate(info["flag_waves"]) if r != 3] == [0] * 7, (pad, info)
            assert pad == 180000 or info["flag_waves"][3] == 0, (pad, info)
            assert np.array_equal(b.coefficients(0), want["coef"]), pad
    c.close()


def case_stream_limit_error():
    """g444_full_err: one erring symbol in the last segment's last MCU, at a bit position above 2^32 - 2^21.  The status and the last
    segment's rows are the port's for the period picture carrying the same damage; every earlier row is the tiling."""
    s = scan(GC.jpeg(GC.FULL_ERR))
    assert int(s.desc.ecs_len) == GC.ECS_CAP
    status, _ = GC.full_err_expected()
    assert status != 0
    measure("g444_full_err:built")
    c = pjd_amd.Context(0)
    info = run_bound(c, s, GC.FULL_ERR, 0, "rgb8", status=status, lane_path=False)
    assert info["n_sequential"] == 0 and info["n_fallback"] == 0 and info["n_entropy_errors"] == 1, info
    c.close()


def case_stream_limit_coefficients():
    """b.coefficients(0) of g444_full: the rows of the last 16 DPUs against the port's coefficients of the period pictures."""
    name = GC.FULL
    s = scan(GC.jpeg(name))
    port = oracle_lib.Port()
    coef = [port.decode(GC.period_jpeg(name, alt))["coef"].reshape(-1) for alt in (False, True)]
    n_seg, w8 = GC.n_segments(name), 8192
    c = pjd_amd.Context(0)
    with c.batch([s.desc], pjd_amd.OUT_RGB8) as b:
        b.upload()
        b.decode(); b.sync()
        assert b.statuses() == [0]
        got = b.coefficients(0)
        info = b.info()
        assert info["n_sequential"] == 0 and info["n_fallback"] == 0, info      # as case_stream_limit: the padding's waves may be flagged
    c.close()
    n_dpus = got.shape[0]
    assert n_dpus == (w8 * (n_seg + n_seg % 2) + 99) // 100             # 100 unit positions (25 blocks of 2 x 2 units) per DPU
    tail = (n_dpus - 16) * 19200
    want = np.zeros(16 * 19200, np.int16)
    x = np.arange(w8, dtype=np.int64)
    n_units = 0
    for y in range(max(0, n_seg - 4), n_seg):                         # the unit rows that can reach into the last 1600 positions
        src = coef[1 if y in GC.marks(name) else 0]
        yp = y % 8
        for comp in range(3):
            og = ((y // 2) * (w8 // 2) + x // 2) * 768 + comp * 256 + ((y % 2) * 2 + x % 2) * 64
            op = ((yp // 2) * (w8 // 2) + x // 2) * 768 + comp * 256 + ((yp % 2) * 2 + x % 2) * 64
            keep = og >= tail
            n_units += int(keep.sum())
            want[(og[keep] - tail)[:, None] + np.arange(64)] = src[op[keep][:, None] + np.arange(64)]
    assert n_units >= 3 * 2 * 350                                     # the 15 full DPUs: 375 blocks, two units of a unit row each
    bad = np.flatnonzero(got.reshape(-1)[tail:] != want)
    assert bad.size == 0, ("coefficients of the last 16 DPUs", "first differing", int(bad[0]), "differing", int(bad.size))
    measure("g444_full:coefficients", coefficient_bytes=got.nbytes)


# ---- shared by the batch cases -------------------------------------------------------------------------------------------------------------
def bind_packed(b, align=1):
    """the packed layout of the batch inside a guarded buffer -> (buffer, offsets of the outputs in its payload)"""
    offs = [b.output_offset(i) for i in range(b.n_out)]
    g = Guarded(offs[-1] + b.output_size(b.n_out - 1), align)
    g.bind(b, offs)
    return g, offs


def gaps_intact(g, offs, sizes, what):
    """the bytes of the payload between two outputs of the packed layout (it aligns every output) are still 0xA5"""
    for i in range(len(offs) - 1):
        gap = g.payload[offs[i] + sizes[i]:offs[i + 1]]
        assert gap.numel() < 4096 and bool((gap == FILL).all()), (what, "gap behind output", i)


def equal_stack(stack, want, what):
    """stack [n, ...] against one expected [...] on the device"""
    want = want.to(DEV)
    ok = (stack == want).flatten(1).all(1)
    assert bool(ok.all()), (what, "outputs differing", int((~ok).sum()), "first", int((~ok).nonzero()[0]))


def square_sources(n=4, size=1024):
    import synth
    return [synth.make(size, size, 7400 + k, 85, synth.SUB_444) for k in range(n)]


# ---- 4: the dense scratch, the component planes and out_off past 2^32 at batch level -------------------------------------------------------
def run_many(flags, n_desc, expected_of, check_coefficients, what):
    src = square_sources()
    sc = [scan(j, flags) for j in src]
    want = [expected_of(j) for j in src]
    measure(f"{what}:built")
    c = pjd_amd.Context(0)
    with c.batch([sc[i % 4].desc for i in range(n_desc)], pjd_amd.OUT_RGB8_PLANAR) as b:
        one = 3 * 1024 * 1024
        g, offs = bind_packed(b)
        assert offs == [i * one for i in range(n_desc)] and g.size == n_desc * one
        b.upload()
        timings, total_ms = b.decode_timed()
        b.sync()
        info = b.info()
        measure(what, first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"] + g.buf.numel(), coef_bytes=info["coef_bytes"],
                largest_offset=offs[-1] + one - 1)
        assert b.statuses() == [0] * n_desc
        stack = g.payload.view(n_desc, 3, 1024, 1024)
        for k in range(4):
            equal_stack(stack[k::4], torch.from_numpy(np.ascontiguousarray(want[k][1].transpose(2, 0, 1))), (what, "source", k))
        g.guards_intact(what)
        for i in check_coefficients:
            assert np.array_equal(b.coefficients(i), want[i % 4][2]), (what, "coefficients of picture", i)
    c.close()
    return info


def case_dense_scratch():
    """720 descriptors of four 1024 x 1024 4:4:4 pictures under PJD_F_FORCE_SEQUENTIAL, planar: the exact kernel's dense scratch is
    720 x 6 MiB = 4 529 848 320 bytes, so the byte offset of a picture's scratch (dense_base x 64 coefficients) passes 2^32 from picture
    683 on.  Every output is the port's picture of its source; coefficients() of the first and the last picture are the port's."""
    port = oracle_lib.Port()

    def expected_of(j):
        d = port.decode(j)
        assert d["huff_rc"] == 0
        return 0, d["rgb"], d["coef"]
    info = run_many(pjd_amd.F_FORCE_SEQUENTIAL, 720, expected_of, (0, 719), "dense_scratch")
    assert info["n_sequential"] == 720 and info["n_fallback"] == 0, info
    assert info["coef_bytes"] >= 720 * 1024 * 1024 * 3 * 2 > TWO32, info


def case_libjpeg_planes():
    """1440 descriptors of the same pictures under PJD_F_LIBJPEG, planar: the component planes (plane_off256 x 256) and the output are
    4 529 848 320 bytes each."""
    import libjpeg_corpus as LC
    port = oracle_lib.Port()

    def expected_of(j):
        st, rgb = LC.expected(port, j)
        assert st == 0
        return 0, rgb, None
    info = run_many(pjd_amd.F_LIBJPEG, 1440, expected_of, (), "libjpeg_planes")
    assert_lane_path(info, "libjpeg_planes")
    assert info["out_bytes"] == 1440 * 3 * 1024 * 1024 > TWO32, info


# ---- 7: dst_off past 2^32 across views ---------------------------------------------------------------------------------------------------
VIEW_SOURCES = ["env_200x150_444_q85_opt", "env_128x96_422_q30", "noise_96x80_420_q95", "h1v2_104x72"]
VIEW_SPECS = [None, dict(flags=1), dict(x=3, y=5, w=60, h=40), dict(x=3, y=5, w=60, h=40, flags=1),
              dict(x=10, y=0, w=80, h=64), dict(x=0, y=7, w=33, h=41, flags=1),
              dict(x=8, y=4, w=64, h=50, vw=1100, vh=1050, ox=40, oy=20), dict(x=1, y=2, w=30, h=60)]


def case_view_offsets():
    """1408 views of 1024 x 1024, planar u8, of four small pictures, cycling through eight (window, flip) specs: dst_off of a view passes
    2^32 from view 1366 on.  View v is picture v % 4 under spec v % 8: eight different expectations, each the window model's."""
    import orientation_model as om
    port = oracle_lib.Port()
    n_views, side = 1408, 1024
    datas = [golden_bytes(n) for n in VIEW_SOURCES]
    sc = [scan(j) for j in datas]
    rgb = [port.decode(j)["rgb"] for j in datas]
    want = [om.window(rgb[k % 4], VIEW_SPECS[k], side, side, "bilinear") for k in range(8)]
    measure("view_offsets:built")
    c = pjd_amd.Context(0)
    with c.batch([s.desc for s in sc], pjd_amd.OUT_RGB8_PLANAR) as b:
        b.set_views([v % 4 for v in range(n_views)])
        b.set_resize([(side, side)] * n_views)
        b.set_resize_window([VIEW_SPECS[v % 8] for v in range(n_views)])
        g, offs = bind_packed(b)
        one = 3 * side * side
        assert offs == [v * one for v in range(n_views)] and b.output_offset(n_views - 1) > TWO32
        b.upload()
        timings, total_ms = b.decode_timed()
        b.sync()
        info = b.info()
        measure("view_offsets", first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"] + g.buf.numel(), largest_offset=offs[-1] + one - 1)
        assert b.statuses() == [0] * 4
        stack = g.payload.view(n_views, 3, side, side)
        for k in range(8):
            equal_stack(stack[k::8], torch.from_numpy(np.ascontiguousarray(want[k].transpose(2, 0, 1))), ("view_offsets", "spec", k))
        g.guards_intact("view_offsets")
    c.close()


# ---- 2: small pictures behind a giant ----------------------------------------------------------------------------------------------------
S2, S4, S8 = pjd_amd.F_SCALE_1_2, pjd_amd.F_SCALE_1_4, pjd_amd.F_SCALE_1_8
SEQ, LJ2 = pjd_amd.F_FORCE_SEQUENTIAL, pjd_amd.F_LIBJPEG | pjd_amd.F_LIBJPEG_SCALE_1_2
SMALL = [("env_200x150_444_q85_opt", S2), ("env_61x45_444_q85_opt", SEQ), ("rst4_128x96_444", LJ2),
         ("env_200x150_422_q30", S4), ("noise_80x96_422_q50_opt", SEQ), ("env_61x45_422_q30", LJ2),
         ("big_640x480_420_q85", S8), ("env_61x45_420_q100_opt", SEQ), ("noise_96x80_420_q95", LJ2),
         ("h1v2_104x72", S2), ("h1v2_45x61", SEQ), ("h1v2_48x64", S4),            # 4:4:0 is outside PJD_F_LIBJPEG's envelope
         ("gray_33x70", 0)]


def case_small_behind_giant(fmt):
    """[g444] and thirteen committed fixtures -- three per sampling: one at a reduced scale (1/2, 1/4, 1/8), one under
    PJD_F_FORCE_SEQUENTIAL, one under PJD_F_LIBJPEG at libjpeg's 1/2 scale (4:4:0: a second reduced scale), and a grey one -- in ONE
    batch, planar or grey.  Every small picture is bound behind 2^32 (the planar giant alone reaches there; for grey the offsets are
    the caller's) and equals what it decodes to in a batch of its own; the giant is compared whole."""
    small = [scan(golden_bytes(n), fl) for n, fl in SMALL]
    giant = scan(GC.jpeg("g444"))
    exp = Expect("g444", 0, fmt == "gray")
    measure(f"small_behind_giant:{fmt}:built")
    c = pjd_amd.Context(0)
    alone = []
    for s in small:
        outs, st = c.decode([s.desc], FMT[fmt])
        alone.append((st[0], outs[0]))
    with c.batch([giant.desc] + [s.desc for s in small], FMT[fmt]) as b:
        sizes = [b.output_size(i) for i in range(b.n)]
        assert sizes[0] == GC.out_bytes(exp.w, exp.h, fmt) and sizes[1:] == [a[1].size for a in alone]
        offs, pos = [0], max(sizes[0], TWO32) + 3
        for n in sizes[1:]:
            offs.append(pos)
            pos += n + 5
        g = Guarded(pos)
        g.bind(b, offs)
        assert all(o + g.off > TWO32 for o in offs[1:])
        b.upload()
        timings, total_ms = b.decode_timed()
        b.sync()
        info = b.info()
        measure(f"small_behind_giant:{fmt}", first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"] + g.buf.numel(), largest_offset=pos - 6)
        assert b.statuses() == [0] + [a[0] for a in alone]
        assert info["n_sequential"] == 4 and info["n_fallback"] == 0, info
        exp.check(g.payload[:sizes[0]], fmt, ("small_behind_giant", fmt))
        covered = [(0, sizes[0])]
        for i, (st, pic) in enumerate(alone, start=1):
            got = g.payload[offs[i]:offs[i] + sizes[i]].cpu().numpy()
            bad = np.flatnonzero(got != pic.reshape(-1))
            assert bad.size == 0, (fmt, SMALL[i - 1], "first differing byte", int(bad[0]), "differing", int(bad.size))
            covered.append((offs[i], offs[i] + sizes[i]))
        g.guards_intact(fmt)
        for (a0, a1), (b0, b1) in zip(covered, covered[1:]):         # between the pictures: still 0xA5, in pieces of 256 MiB
            for lo in range(a1, b0, 1 << 28):
                assert bool((g.payload[lo:min(b0, lo + (1 << 28))] == FILL).all()), (fmt, "bytes between pictures written", lo)
    c.close()


# ---- 5: the resample's source past 2^32 --------------------------------------------------------------------------------------------------
def crossing_windows():
    """six windows of 512 x 384 in g444: the two far corners and two around each point where the planar and the interleaved
    intermediate pass 2^32 (the window holds the row and the column of that byte); the second is mirrored"""
    w, h = GC.spec("g444")[0], GC.height("g444")
    yb = GC.crossings("g444")["planar"][0]
    xb = TWO32 - 2 * w * h - yb * w
    yi = GC.crossings("g444")["rgb8"][0]
    xi = (TWO32 - yi * 3 * w) // 3
    assert 0 <= xb < w and 0 <= xi < w

    def win(x, y, flip=0):
        x, y = min(max(x, 0), w - 512), min(max(y, 0), h - 384)
        return dict(x=x, y=y, w=512, h=384, flags=flip)
    wins = [win(0, 0), win(w, h, 1), win(xb - 100, yb - 50), win(xb - 400, yb - 300), win(xi - 100, yi - 50), win(xi - 400, yi - 300)]
    for k, (x, y) in ((2, (xb, yb)), (3, (xb, yb)), (4, (xi, yi)), (5, (xi, yi))):
        assert wins[k]["x"] <= x < wins[k]["x"] + 512 and wins[k]["y"] <= y < wins[k]["y"] + 384
    return wins


def case_resample_source(fmt, filt, dtype="u8"):
    """g444 decoded once into the resample's intermediate (planar, interleaved or grey: as the output) and six views of it resized to
    224 x 224.  Expected: the window models over giant_corpus.expected_rows of the crop -- a window's taps read only the window."""
    import normalize_model as nm
    import orientation_model as om
    from pjd_amd import tensors
    gray = fmt == "gray"
    wins = crossing_windows()
    want = []
    for wd in wins:
        crop = GC.expected_rows("g444", wd["y"], wd["y"] + 384, 0, gray)[:, wd["x"]:wd["x"] + 512]
        crop = np.repeat(crop[:, :, None], 3, axis=2) if gray else crop
        want.append(om.window(np.ascontiguousarray(crop), dict(flags=wd["flags"]), 224, 224, filt))
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    s = scan(GC.jpeg("g444"))
    measure(f"resample_source:{fmt}:{filt}:{dtype}:built")
    c = pjd_amd.Context(0)
    with c.batch([s.desc], FMT[fmt]) as b:
        b.set_views([0] * 6)
        b.set_resize([(224, 224)] * 6)
        b.set_resize_window(wins)
        if filt != "bilinear":
            b.set_resize_filter({"antialias": pjd_amd.RESIZE_ANTIALIAS, "bicubic": pjd_amd.RESIZE_BICUBIC}[filt])
        esize = 1
        if dtype == "f16":
            b.set_normalize(pjd_amd.DT_F16, scale, bias)
            esize = 2
        g, offs = bind_packed(b, esize)
        sizes = [b.output_size(v) for v in range(6)]
        assert sizes == [224 * 224 * (1 if gray else 3) * esize] * 6
        b.upload()
        timings, total_ms = b.decode_timed()
        b.sync()
        info = b.info()
        measure(f"resample_source:{fmt}:{filt}:{dtype}", first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"] + g.buf.numel(),
                largest_offset=GC.out_bytes(GC.spec("g444")[0], GC.height("g444"), fmt) - 1)
        assert b.statuses() == [0]
        assert_lane_path(info, ("resample_source", fmt, filt))
        host = g.payload.cpu().numpy()
        for v in range(6):
            wv = want[v] if dtype == "u8" else nm.bits(nm.normalize(want[v], nm.DT_F16, scale, bias))
            wv = wv[..., 0] if gray else (wv.transpose(2, 0, 1) if fmt == "planar" else wv)
            raw = host[offs[v]:offs[v] + sizes[v]].view(wv.dtype)
            assert np.array_equal(raw, np.ascontiguousarray(wv).reshape(-1)), (fmt, filt, dtype, "view", v, wins[v])
        g.guards_intact((fmt, filt))
        gaps_intact(g, offs, sizes, (fmt, filt))
    c.close()


# ---- 6: the resample's destination past 2^32 inside one canvas -----------------------------------------------------------------------------
CANVAS_SOURCE = "env_200x150_444_q85_opt"
CONTENT = (301, 203)              # (cw, ch): the content rectangle, in the canvas's bottom-right corner
CANVAS_FILL = (17, 99, 203)
PAD_VALUE = (0.5, -1.0, 3e-6)


def case_canvas(fmt, dtype, runs):
    """One picture letterboxed onto a canvas of 65535 x 32768 (u8: 6.4 GB planar or interleaved) or 65535 x 21846 (interleaved fp16:
    8.6 GB): the content rectangle, at the far end of the canvas, equals the model, and EVERY other element is the fill -- what
    pjd_k_resize_border delivers.  runs: comma-separated filter[:orientation]."""
    import normalize_model as nm
    import orientation_model as om
    import resize_pad_model as pm
    from pjd_amd import tensors
    port = oracle_lib.Port()
    data = golden_bytes(CANVAS_SOURCE)
    rgb = port.decode(data)["rgb"]
    s = scan(data)
    cw, ch = CONTENT
    wc, hc = 65535, (32768 if dtype == "u8" else 21846)
    esize = 1 if dtype == "u8" else 2
    assert wc * hc * 3 * esize > TWO32 + (1 << 30)
    pad = (wc - cw, hc - ch, 0, 0)
    scale, bias = tensors.normalize_constants(nm.IMAGENET_MEAN, nm.IMAGENET_STD)
    c = pjd_amd.Context(0)
    for run in runs.split(","):
        filt, _, o = run.partition(":")
        o = int(o or 1)
        D = om.oriented(rgb, None, cw, ch, o, filt)
        if dtype == "u8":
            content = torch.from_numpy(D).to(DEV)
            border = torch.tensor(CANVAS_FILL, dtype=torch.uint8, device=DEV)
        else:
            content = torch.from_numpy(nm.bits(nm.normalize(D, nm.DT_F16, scale, bias)).view(np.int16)).to(DEV)
            border = torch.from_numpy(np.array([pm.convert(v, nm.DT_F16) for v in PAD_VALUE], np.float16).view(np.int16)).to(DEV)
        with c.batch([s.desc], FMT[fmt]) as b:
            b.set_resize([(hc, wc)])
            b.set_resize_pad([pad], CANVAS_FILL)
            if o != 1:
                b.set_orientation([o])
            if filt != "bilinear":
                b.set_resize_filter({"antialias": pjd_amd.RESIZE_ANTIALIAS, "bicubic": pjd_amd.RESIZE_BICUBIC}[filt])
            if dtype != "u8":
                b.set_normalize(pjd_amd.DT_F16, scale, bias)
                b.set_pad_value(PAD_VALUE)
            size = b.output_size(0)
            assert size == wc * hc * 3 * esize
            g = Guarded(size, esize)
            g.bind(b)
            b.upload()
            timings, total_ms = b.decode_timed()
            b.sync()
            info = b.info()
            what = ("canvas", fmt, dtype, run)
            measure(f"canvas:{fmt}:{dtype}:{run}", first_decode_ms=f"{total_ms:.1f}", device_bytes=info["device_bytes"] + g.buf.numel(), largest_offset=size - 1)
            assert b.statuses() == [0]
            elems = g.payload if dtype == "u8" else g.payload.view(torch.int16)
            if fmt == "planar":
                canvas = elems.view(3, hc, wc)
                for ch_i in range(3):
                    plane = canvas[ch_i]
                    for y0 in range(0, hc - ch, 4096):
                        assert bool((plane[y0:min(hc - ch, y0 + 4096)] == border[ch_i]).all()), (what, "border of plane", ch_i, "rows from", y0)
                    assert bool((plane[hc - ch:, :wc - cw] == border[ch_i]).all()), (what, "border left of the content, plane", ch_i)
                    same_on_device(plane[hc - ch:, wc - cw:], content[..., ch_i], (what, "content, plane", ch_i))
            else:
                canvas = elems.view(hc, wc, 3)
                for y0 in range(0, hc - ch, 2048):
                    assert bool((canvas[y0:min(hc - ch, y0 + 2048)] == border).all()), (what, "border rows from", y0)
                assert bool((canvas[hc - ch:, :wc - cw] == border).all()), (what, "border left of the content")
                same_on_device(canvas[hc - ch:, wc - cw:], content, (what, "content"))
            g.guards_intact(what)
        del g, canvas, elems
        torch.cuda.empty_cache()
    c.close()


CASES = {}
for _n, _f in list(globals().items()):
    if _n.startswith("case_"):
        CASES[_n[5:]] = _f

if __name__ == "__main__":
    case = sys.argv[1]
    CASES[case](*sys.argv[2:])
    print(f"CASE OK {case}", flush=True)
