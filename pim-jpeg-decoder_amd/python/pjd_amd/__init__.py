"""pjd_amd -- thin ctypes binding of the C ABI in include/pjd.h and include/pjd_host.h.

Python is plumbing here (tests, bench harness); the product is lib/libpjd.so (HIP kernels for
gfx950 behind the C ABI) and lib/libpjdhost.so (scanner + BMP helpers).  There is no CPU decode
path in this package: without a gfx950 device `Context()` raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_DIR = os.path.join(_PKG, "lib")
LIBPJD = os.path.join(LIB_DIR, "libpjd.so")
LIBHOST = os.path.join(LIB_DIR, "libpjdhost.so")
LIBPIPE = os.path.join(LIB_DIR, "libpjdpipe.so")

OUT_RGB8, OUT_BMP = 0, 1
OUT_RGB8_PLANAR = 2      # uint8[3][H][W]: the R, G and B planes one after the other (pjd.h)
OUT_GRAY8 = 4            # uint8[H][W]: one plane, the luma as libjpeg's JCS_GRAYSCALE delivers it (pjd.h, "grey output"); 3 stays no format
PLAN_LATENCY, PLAN_THROUGHPUT = 0, 1      # pjd_set_plan_mode
F_STANDARD_RESTART, F_FORCE_SEQUENTIAL, F_STANDARD_ZIGZAG, F_PROGRESSIVE = 1, 2, 4, 8
F_SCALE_1_2, F_SCALE_1_4, F_SCALE_1_8, F_SCALE_MASK = 16, 32, 48, 48      # output scale s = 1 << ((flags >> 4) & 3) (pjd.h)
F_LIBJPEG_SCALE_1_2, F_LIBJPEG_SCALE_1_4, F_LIBJPEG_SCALE_1_8, F_LIBJPEG_SCALE_MASK = 128, 256, 384, 384   # with F_LIBJPEG: libjpeg's reduced decode (its scaled IDCTs), s = 1 << ((flags >> 7) & 3) (pjd.h)
F_LIBJPEG = 64           # the picture libjpeg decodes, bit for bit (islow IDCT, fancy upsampling, JFIF colour); implies the two F_STANDARD_* (pjd.h)
RESIZE_BILINEAR, RESIZE_ANTIALIAS = 0, 1   # pjd_batch_set_resize_filter (pjd.h)
RW_HFLIP = 1                               # pjd_resize_window.flags: the delivered picture mirrored left-right
AA_MAX_TAPS = 32                           # PJD_AA_MAX_TAPS: the most taps per axis pjd_resize_aa_taps returns
RESIZE_BICUBIC = 3                         # PJD_RESIZE_BICUBIC: Keys' cubic (a = -0.5), widened where an axis shrinks
BICUBIC_MAX_TAPS = 64                      # PJD_BICUBIC_MAX_TAPS: the most taps per axis pjd_resize_bicubic_taps returns
BICUBIC_MAX_GAIN = 92681                   # PJD_BICUBIC_MAX_GAIN: the largest sum |q_j| of an axis set_resize_filter accepts
DT_F16, DT_BF16, DT_F32 = 1, 2, 3         # pjd_batch_set_normalize: IEEE binary16, bfloat16, IEEE binary32 (pjd.h)
SCAN_PROGRESSIVE = 1
MAX_KERNELS = 16
ABI_VERSION = 6          # PJD_VERSION of include/pjd.h these ctypes structs mirror


class HuffTable(C.Structure):
    _fields_ = [("offsets", C.c_uint8 * 17), ("symbols", C.c_uint8 * 162), ("set", C.c_uint8)]


class ScanDesc(C.Structure):
    _fields_ = [("n_comp", C.c_uint8), ("comp", C.c_uint8 * 3), ("ss", C.c_uint8), ("se", C.c_uint8), ("ah", C.c_uint8), ("al", C.c_uint8),
                ("restart_interval", C.c_uint32), ("table", HuffTable * 3), ("ecs", C.c_void_p), ("ecs_len", C.c_uint64)]


class ImageDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("num_components", C.c_uint8), ("h_samp", C.c_uint8), ("v_samp", C.c_uint8),
        ("comp_h", C.c_uint8 * 3), ("comp_v", C.c_uint8 * 3),
        ("comp_qt", C.c_uint8 * 3), ("comp_dc", C.c_uint8 * 3), ("comp_ac", C.c_uint8 * 3),
        ("qt_set", C.c_uint8 * 4),
        ("qt", (C.c_uint32 * 64) * 4),
        ("dc", HuffTable * 4), ("ac", HuffTable * 4),
        ("restart_interval", C.c_uint32),
        ("ecs", C.c_void_p), ("ecs_len", C.c_uint64),
        ("seg_offsets", C.c_void_p), ("n_segments", C.c_uint32),
        ("flags", C.c_uint32),
        ("shard_first_seg", C.c_uint32), ("shard_n_segs", C.c_uint32),
        ("qt_slot48", C.c_uint32 * 4),
        ("scans", C.POINTER(ScanDesc)), ("n_scans", C.c_uint32), ("reserved_", C.c_uint32),
    ]


class Timings(C.Structure):
    _fields_ = [("n", C.c_int32), ("ms", C.c_float * MAX_KERNELS),
                ("name", (C.c_char * 32) * MAX_KERNELS), ("total_ms", C.c_float)]

    def as_dict(self):
        return {self.name[i].value.decode(): float(self.ms[i]) for i in range(self.n)}


class ResizeWindow(C.Structure):
    """pjd_resize_window (pjd.h): the source window (x, y, w, h; w == h == 0: the whole picture), the virtual target it is resampled to
    (vw, vh; 0: the picture's target), the part of it that is delivered (from ox, oy) and RW_HFLIP in flags.  All zero: the identity."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("vw", C.c_uint32), ("vh", C.c_uint32),
                ("ox", C.c_uint32), ("oy", C.c_uint32), ("flags", C.c_uint32), ("reserved_", C.c_uint32)]


class ResizePad(C.Structure):
    """pjd_resize_pad (pjd.h): how many columns and rows of the delivered canvas lie left of, above, right of and below the content
    rectangle.  All zero: the picture fills its canvas."""
    _fields_ = [("left", C.c_uint32), ("top", C.c_uint32), ("right", C.c_uint32), ("bottom", C.c_uint32)]


BLUR_MAX_TAPS = 63                         # PJD_BLUR_MAX_TAPS


class Blur(C.Structure):
    """pjd_blur (pjd.h): one output's Gaussian -- sigma and the odd tap count ksize; ksize == 0 with sigma == 0: no blur."""
    _fields_ = [("sigma", C.c_double), ("ksize", C.c_uint32), ("reserved_", C.c_uint32)]


class BatchInfo(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("pixels", C.c_uint64), ("ecs_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("coef_bytes", C.c_uint64), ("n_data_units", C.c_uint64),
                ("n_subsequences", C.c_uint64), ("device_bytes", C.c_uint64),
                ("n_sequential", C.c_int32), ("n_fallback", C.c_int32),
                ("n_huff_workgroups", C.c_uint64), ("sync_rounds", C.c_uint64), ("sync_lane_passes", C.c_uint64),
                ("fix_rounds", C.c_uint64), ("fix_lane_passes", C.c_uint64),
                ("sub_bytes", C.c_uint32), ("n_table_sets", C.c_uint32), ("n_huff_waves", C.c_uint64),
                ("n_entries", C.c_uint64), ("exact_fallback_ms", C.c_float), ("n_entropy_errors", C.c_uint32),
                ("flag_waves", C.c_uint64 * 8), ("huff_lds_bytes", C.c_uint32), ("plan_mode", C.c_uint32), ("walks", C.c_uint64), ("walk_lanes", C.c_uint64), ("n_steps", C.c_uint64),
                ("lane_fill_x1024", C.c_uint32), ("dc_plan", C.c_uint32)]       # bits 0..7: 0 three-launch DC scan, 1 a workgroup per picture; bits 8..15: picture groups planned (pjd.h)


SPLIT_MAX_DEVICES = 16


class SplitStats(C.Structure):
    _fields_ = [("wall_s", C.c_double), ("broadcast_s", C.c_double), ("upload_s", C.c_double), ("exec_s", C.c_double), ("download_s", C.c_double),
                ("blob_bytes", C.c_uint64), ("ecs_bytes", C.c_uint64 * SPLIT_MAX_DEVICES),
                ("n_segments", C.c_uint32), ("n_ranks", C.c_uint32), ("n_exact", C.c_uint32),
                ("rccl_used", C.c_int32), ("redone_whole", C.c_int32)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "ecs_bytes" else getattr(self, k)) for k, _ in self._fields_}


class PjdError(RuntimeError):
    pass


_host = None
_dev = None


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(LIBHOST):
            raise PjdError(f"{LIBHOST} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIBHOST)
        L.pjd_scan_memory.restype = C.c_int
        L.pjd_scan_memory.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.POINTER(C.c_void_p)]
        L.pjd_scan_file.restype = C.c_int
        L.pjd_scan_file.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.pjd_scan_memory_ex.restype = C.c_int
        L.pjd_scan_memory_ex.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.pjd_scan_file_ex.restype = C.c_int
        L.pjd_scan_file_ex.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.pjd_scanned_desc.restype = C.POINTER(ImageDesc)
        L.pjd_scanned_desc.argtypes = [C.c_void_p]
        L.pjd_scanned_log.restype = C.c_char_p
        L.pjd_scanned_log.argtypes = [C.c_void_p]
        L.pjd_scanned_valid.restype = C.c_int
        L.pjd_scanned_valid.argtypes = [C.c_void_p]
        L.pjd_scanned_orientation.restype = C.c_int
        L.pjd_scanned_orientation.argtypes = [C.c_void_p]
        L.pjd_scanned_free.argtypes = [C.c_void_p]
        L.pjd_scanned_metadata.argtypes = [C.c_void_p, C.c_void_p]
        L.pjd_rgb_to_bmp.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.pjd_write_file.restype = C.c_int
        L.pjd_write_file.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64]
        _host = L
    return _host


def dev_lib():
    """Load libpjd.so.  Fails loudly when the HIP extension has not been built."""
    global _dev
    if _dev is None:
        if not os.path.exists(LIBPJD):
            raise PjdError(f"{LIBPJD} missing: the HIP extension is not built (no CPU fallback exists)")
        L = C.CDLL(LIBPJD)
        vp, i32 = C.c_void_p, C.c_int
        L.pjd_version.restype = i32
        if L.pjd_version() != ABI_VERSION:
            raise PjdError(f"{LIBPJD} has ABI version {L.pjd_version()}, these bindings mirror version {ABI_VERSION}: rebuild")
        L.pjd_open.restype = i32
        L.pjd_open.argtypes = [i32, C.POINTER(vp)]
        L.pjd_close.argtypes = [vp]
        L.pjd_set_plan_mode.restype = i32
        L.pjd_set_plan_mode.argtypes = [vp, i32]
        L.pjd_last_error.restype = C.c_char_p
        L.pjd_last_error.argtypes = [vp]
        L.pjd_status_string.restype = C.c_char_p
        L.pjd_status_string.argtypes = [i32]
        L.pjd_stream.restype = vp
        L.pjd_stream.argtypes = [vp]
        L.pjd_batch_create.restype = i32
        L.pjd_batch_create.argtypes = [vp, C.POINTER(ImageDesc), i32, i32, C.POINTER(vp)]
        for fn in ("pjd_batch_upload", "pjd_batch_decode", "pjd_batch_capture", "pjd_batch_sync"):
            getattr(L, fn).restype = i32
            getattr(L, fn).argtypes = [vp]
        L.pjd_batch_decode_timed.restype = i32
        L.pjd_batch_decode_timed.argtypes = [vp, C.POINTER(Timings)]
        L.pjd_batch_download.restype = i32
        L.pjd_batch_download.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32)]
        L.pjd_batch_get_info.restype = i32
        L.pjd_batch_get_info.argtypes = [vp, C.POINTER(BatchInfo)]
        L.pjd_batch_download_packed.restype = i32
        L.pjd_batch_download_packed.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_int32)]
        L.pjd_batch_packed_size.restype = C.c_uint64
        L.pjd_batch_packed_size.argtypes = [vp]
        L.pjd_batch_output_offset.restype = C.c_uint64
        L.pjd_batch_output_offset.argtypes = [vp, i32]
        L.pjd_batch_bind_output.restype = i32
        L.pjd_batch_bind_output.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.pjd_batch_set_views.restype = i32
        L.pjd_batch_set_views.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint32]
        L.pjd_batch_n_outputs.restype = C.c_uint32
        L.pjd_batch_n_outputs.argtypes = [vp]
        L.pjd_batch_set_resize.restype = i32
        L.pjd_batch_set_resize.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pjd_resize_tap.restype = i32
        L.pjd_resize_tap.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pjd_batch_set_resize_filter.restype = i32
        L.pjd_batch_set_resize_filter.argtypes = [vp, i32]
        L.pjd_resize_aa_taps.restype = i32
        L.pjd_resize_aa_taps.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pjd_resize_bicubic_taps.restype = i32
        L.pjd_resize_bicubic_taps.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        L.pjd_batch_set_resize_window.restype = i32
        L.pjd_batch_set_resize_window.argtypes = [vp, C.POINTER(ResizeWindow)]
        L.pjd_batch_set_orientation.restype = i32
        L.pjd_batch_set_orientation.argtypes = [vp, C.POINTER(C.c_uint8)]
        L.pjd_batch_set_resize_pad.restype = i32
        L.pjd_batch_set_resize_pad.argtypes = [vp, C.POINTER(ResizePad), C.POINTER(C.c_uint8)]
        L.pjd_batch_set_pad_value.restype = i32
        L.pjd_batch_set_pad_value.argtypes = [vp, C.POINTER(C.c_float)]
        L.pjd_batch_set_resize_affine.restype = i32
        L.pjd_batch_set_resize_affine.argtypes = [vp, C.POINTER(C.c_double * 6), C.POINTER(C.c_uint8)]
        L.pjd_warp_tap.restype = i32
        L.pjd_warp_tap.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pjd_resize_affine_check.restype = i32
        L.pjd_resize_affine_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        L.pjd_batch_set_colour.restype = i32
        L.pjd_batch_set_colour.argtypes = [vp, C.POINTER(C.c_double * 12)]
        L.pjd_colour_value.restype = i32
        L.pjd_colour_value.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
        L.pjd_colour_check.restype = i32
        L.pjd_colour_check.argtypes = [C.POINTER(C.c_double)]
        L.pjd_batch_set_blur.restype = i32
        L.pjd_batch_set_blur.argtypes = [vp, C.POINTER(Blur)]
        L.pjd_blur_taps.restype = i32
        L.pjd_blur_taps.argtypes = [C.c_uint32, C.c_double, C.POINTER(C.c_uint32)]
        L.pjd_blur_index.restype = i32
        L.pjd_blur_index.argtypes = [C.c_uint32, C.c_int64, C.POINTER(C.c_uint32)]
        L.pjd_blur_check.restype = i32
        L.pjd_blur_check.argtypes = [C.POINTER(Blur)]
        L.pjd_resize_pad_check.restype = i32
        L.pjd_resize_pad_check.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(ResizePad)]
        L.pjd_resize_window_check.restype = i32
        L.pjd_resize_window_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ResizeWindow), i32]
        L.pjd_batch_set_normalize.restype = i32
        L.pjd_batch_set_normalize.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.pjd_libjpeg_idct.restype = i32
        L.pjd_libjpeg_idct.argtypes = [C.POINTER(C.c_int16), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]
        L.pjd_libjpeg_idct_scaled.restype = i32
        L.pjd_libjpeg_idct_scaled.argtypes = [C.POINTER(C.c_int16), C.POINTER(C.c_uint16), C.c_uint32, C.POINTER(C.c_uint8)]
        L.pjd_libjpeg_ycc_to_rgb.restype = i32
        L.pjd_libjpeg_ycc_to_rgb.argtypes = [C.c_uint8, C.c_uint8, C.c_uint8, C.POINTER(C.c_uint8)]
        L.pjd_libjpeg_upsample_row.restype = i32
        L.pjd_libjpeg_upsample_row.argtypes = [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), i32, C.c_uint32, C.POINTER(C.c_uint8)]
        L.pjd_normalize_value.restype = i32
        L.pjd_normalize_value.argtypes = [i32, C.c_uint32, C.c_float, C.c_float, vp]
        L.pjd_host_alloc.restype = vp
        L.pjd_host_alloc.argtypes = [C.c_uint64]
        L.pjd_host_free.argtypes = [vp]
        L.pjd_batch_output_size.restype = C.c_uint64
        L.pjd_batch_output_size.argtypes = [vp, i32]
        L.pjd_batch_device_output.restype = vp
        L.pjd_batch_device_output.argtypes = [vp, i32]
        L.pjd_batch_device_status.restype = vp
        L.pjd_batch_device_status.argtypes = [vp]
        L.pjd_batch_destroy.argtypes = [vp]
        L.pjd_decode_batch.restype = i32
        L.pjd_decode_batch.argtypes = [vp, C.POINTER(ImageDesc), i32, i32, C.POINTER(vp), C.POINTER(C.c_int32)]
        L.pjd_exec_dpu_payload.restype = i32
        L.pjd_exec_dpu_payload.argtypes = [vp, vp, vp, i32]
        L.pjd_output_size.restype = C.c_uint64
        L.pjd_output_size.argtypes = [C.c_uint32, C.c_uint32, i32]
        L.pjd_output_channels.restype = i32
        L.pjd_output_channels.argtypes = [i32]
        L.pjd_scaled_dims.restype = i32
        L.pjd_scaled_dims.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pjd_image_output_size.restype = C.c_uint64
        L.pjd_image_output_size.argtypes = [C.POINTER(ImageDesc), i32]
        L.pjd_coefficients_size.restype = C.c_uint64
        L.pjd_coefficients_size.argtypes = [C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8]
        L.pjd_batch_download_coefficients.restype = i32
        L.pjd_batch_download_coefficients.argtypes = [vp, i32, vp, C.c_uint64]
        L.pjd_split_decode.restype = i32
        L.pjd_split_decode.argtypes = [C.POINTER(ImageDesc), C.POINTER(C.c_int32), i32, i32, vp, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(SplitStats)]
        L.pjd_split_plan.restype = i32
        L.pjd_split_plan.argtypes = [C.POINTER(ImageDesc), i32, i32, C.POINTER(ImageDesc), vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.pjd_split_release.restype = None
        L.pjd_plan_info.restype = i32
        L.pjd_plan_info.argtypes = [C.POINTER(ImageDesc), i32, i32, C.POINTER(BatchInfo)]
        L.pjd_plan_check.restype = i32
        L.pjd_plan_check.argtypes = [C.POINTER(ImageDesc), i32, i32, C.c_char_p, C.c_uint64]
        _dev = L
    return _dev


class Scanned:
    """A parsed JPEG (host side).  Mirrors the reference's `Header` for the decode path."""

    def __init__(self, data: bytes = None, name: str = "x.jpg", path: str = None, options: int = 0):
        """options: SCAN_PROGRESSIVE parses a progressive file scan by scan (not reference behaviour: the reference rejects it)."""
        L = host_lib()
        h = C.c_void_p()
        if path is not None:
            rc = L.pjd_scan_file_ex(path.encode(), options, C.byref(h))
            if rc == 2:
                raise FileNotFoundError(path)
        else:
            self._data = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
            rc = L.pjd_scan_memory_ex(self._data.ctypes.data, len(data), name.encode(), options, C.byref(h))
        self._h = h
        self.rc = rc
        self.valid = bool(L.pjd_scanned_valid(h))
        self.log = L.pjd_scanned_log(h).decode()
        self.desc = L.pjd_scanned_desc(h).contents
        self.orientation = int(L.pjd_scanned_orientation(h))    # the EXIF orientation tag, 1..8; 1 without a valid one (include/pjd_host.h)

    def metadata(self):
        m = np.zeros(276, np.uint32)
        host_lib().pjd_scanned_metadata(self._h, m.ctypes.data)
        return m

    def ecs(self):
        n = int(self.desc.ecs_len)
        if n == 0:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(self.desc.ecs, C.POINTER(C.c_uint8)), (n,)).copy()

    def seg_offsets(self):
        n = int(self.desc.n_segments)
        return np.ctypeslib.as_array(C.cast(self.desc.seg_offsets, C.POINTER(C.c_uint64)), (n,)).copy()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                host_lib().pjd_scanned_free(self._h)
                self._h = None
        except Exception:
            pass


def rgb_to_bmp(rgb: np.ndarray) -> bytes:
    h, w, _ = rgb.shape
    rgb = np.ascontiguousarray(rgb, np.uint8)
    out = np.zeros(26 + h * (3 * w + w % 4), np.uint8)
    host_lib().pjd_rgb_to_bmp(rgb.ctypes.data, w, h, out.ctypes.data)
    return out.tobytes()


class Context:
    """One GPU (replaces DpuSet::allocate + load of the reference)."""

    def __init__(self, device: int = 0, plan_mode: int = None):
        L = dev_lib()
        h = C.c_void_p()
        rc = L.pjd_open(device, C.byref(h))
        if rc != 0:
            raise PjdError(f"pjd_open({device}) failed with {rc}: no usable gfx950 device")
        self._h = h
        self.L = L
        self.device = int(device)
        if plan_mode is not None:
            self.set_plan_mode(plan_mode)

    def set_plan_mode(self, mode: int):
        """PLAN_LATENCY (a batch decoded alone finishes sooner) or PLAN_THROUGHPUT (batches kept in flight: more pictures per second);
        applies to batches created afterwards (include/pjd.h, pjd_set_plan_mode)."""
        self._check(self.L.pjd_set_plan_mode(self._h, int(mode)), "pjd_set_plan_mode")

    def close(self):
        if self._h:
            self.L.pjd_close(self._h)
            self._h = None

    def _check(self, rc, what):
        if rc != 0:
            raise PjdError(f"{what} failed ({rc}): {self.L.pjd_last_error(self._h).decode()}")

    @property
    def stream(self):
        return self.L.pjd_stream(self._h)

    def batch(self, descs, out_format=OUT_RGB8):
        return Batch(self, descs, out_format)

    def decode(self, descs, out_format=OUT_RGB8):
        """One-shot decode -> (list of np.uint8 arrays, list of status ints)."""
        with self.batch(descs, out_format) as b:
            b.upload()
            b.decode()
            return b.download()

    def exec_dpu_payload(self, metadata: np.ndarray, mcus: np.ndarray):
        """The literal DPU contract: metadata (n,276) uint32, mcus (n,19200) int16 in/out."""
        metadata = np.ascontiguousarray(metadata, np.uint32).reshape(-1, 276)
        assert mcus.dtype == np.int16 and mcus.flags.c_contiguous
        n = metadata.shape[0]
        assert mcus.size == n * 19200
        self._check(self.L.pjd_exec_dpu_payload(self._h, metadata.ctypes.data, mcus.ctypes.data, n), "pjd_exec_dpu_payload")
        return mcus


class Batch:
    def __init__(self, ctx: Context, descs, out_format):
        self.ctx, self.L = ctx, ctx.L
        self.n = len(descs)
        self.out_format = out_format
        arr = (ImageDesc * max(self.n, 1))()
        for i, d in enumerate(descs):
            C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(ImageDesc))
        self._descs = arr
        self._keep = descs
        h = C.c_void_p()
        ctx._check(self.L.pjd_batch_create(ctx._h, arr, self.n, out_format, C.byref(h)), "pjd_batch_create")
        self._h = h
        self._resize = None                        # set_resize: the (h, w) of every output
        self.views = None                          # set_views: the picture of every view
        self._dtype = None                         # set_normalize: DT_*

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.destroy()

    def destroy(self):
        if self._h:
            self.L.pjd_batch_destroy(self._h)
            self._h = None

    @property
    def n_out(self):
        """The outputs of the batch (pjd_batch_n_outputs): its views once set_views() was called, else its pictures.  Status words stay
        per picture (`n`)."""
        return self.n if self.views is None else len(self.views)

    def set_views(self, picture_of_view):
        """pjd_batch_set_views: the batch delivers len(picture_of_view) outputs, view v a resample of picture picture_of_view[v] (any
        order, any number of views per picture, none included); every picture is decoded once.  From then on every per-picture argument
        of set_resize(), set_resize_pad(), set_orientation(), set_resize_window() and bind_output(), and the index of output_size(),
        output_offset(), output_shape() and device_output(), is per VIEW (n_out entries); download() returns n_out arrays and n statuses.
        Once, first: before set_resize() / set_normalize() / bind_output() / upload(), one of the first two must follow; not for OUT_BMP."""
        views = [int(p) for p in picture_of_view]
        if any(not 0 <= p < 2 ** 32 for p in views):
            raise ValueError("set_views: picture indices must fit 32 bits")
        if len(views) >= 2 ** 32:
            raise ValueError("set_views: too many views")
        arr = (C.c_uint32 * max(len(views), 1))(*views)
        self.ctx._check(self.L.pjd_batch_set_views(self._h, arr, len(views)), "pjd_batch_set_views")
        self.views = views

    def upload(self):
        self.ctx._check(self.L.pjd_batch_upload(self._h), "pjd_batch_upload")

    def decode(self):
        self.ctx._check(self.L.pjd_batch_decode(self._h), "pjd_batch_decode")

    def decode_timed(self):
        t = Timings()
        self.ctx._check(self.L.pjd_batch_decode_timed(self._h, C.byref(t)), "pjd_batch_decode_timed")
        return t.as_dict(), float(t.total_ms)

    def capture(self):
        self.ctx._check(self.L.pjd_batch_capture(self._h), "pjd_batch_capture")

    def sync(self):
        self.ctx._check(self.L.pjd_batch_sync(self._h), "pjd_batch_sync")

    def decode_chains(self):
        """pjd_batch_decode_chains: the form the last decode was issued in -- 0 before the first, 1 for one chain of launches, g >= 2 for
        the chains of g picture groups (a replay: the form of the graph that was launched; decode_timed: always 1)."""
        self.L.pjd_batch_decode_chains.restype = C.c_int32
        self.L.pjd_batch_decode_chains.argtypes = [C.c_void_p]
        n = int(self.L.pjd_batch_decode_chains(self._h))
        if n < 0:
            self.ctx._check(n, "pjd_batch_decode_chains")
        return n

    def info(self):
        bi = BatchInfo()
        self.ctx._check(self.L.pjd_batch_get_info(self._h, C.byref(bi)), "pjd_batch_get_info")
        return {k: (list(getattr(bi, k)) if k == "flag_waves" else (float(getattr(bi, k)) if k == "exact_fallback_ms" else int(getattr(bi, k)))) for k, _ in bi._fields_}

    def huff_occupancy(self):
        """pjd_batch_huff_occupancy: (workgroups of the entropy decoder one CU holds, as the runtime computes it; the dynamic LDS it asked with)."""
        self.L.pjd_batch_huff_occupancy.restype = C.c_int32
        self.L.pjd_batch_huff_occupancy.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        n, lds = C.c_int32(), C.c_uint32()
        self.ctx._check(self.L.pjd_batch_huff_occupancy(self._h, C.byref(n), C.byref(lds)), "pjd_batch_huff_occupancy")
        return int(n.value), int(lds.value)

    def output_size(self, i):
        return int(self.L.pjd_batch_output_size(self._h, i))

    def device_output(self, i):
        return self.L.pjd_batch_device_output(self._h, i)

    def output_offset(self, i):
        return int(self.L.pjd_batch_output_offset(self._h, i))

    def packed_size(self):
        return int(self.L.pjd_batch_packed_size(self._h))

    def output_shape(self, i):
        """Shape of picture i as download() returns it: (h, w, 3) for OUT_RGB8, (3, h, w) for OUT_RGB8_PLANAR, (h, w) for OUT_GRAY8,
        flat for OUT_BMP."""
        d = self._descs[i if self.views is None else self.views[i]]
        if self._resize is not None:
            h, w = self._resize[i]
        else:
            w, h = scaled_dims(d.width, d.height, d.flags)
        if self.out_format == OUT_RGB8:
            return (h, w, 3)
        if self.out_format == OUT_RGB8_PLANAR:
            return (3, h, w)
        if self.out_format == OUT_GRAY8:
            return (h, w)
        return (self.output_size(i),)

    def set_resize(self, sizes):
        """pjd_batch_set_resize: picture i leaves the decode resampled to sizes[i] = (h, w), with the bilinear filter include/pjd.h
        specifies bit for bit.  Once, before bind_output() / upload(); not for OUT_BMP, not for shards.  output_size, output_shape,
        output_offset, packed_size, download and bind_output speak about the resized pictures from then on."""
        if len(sizes) != self.n_out:
            raise ValueError("set_resize: one (h, w) per picture (per view after set_views)")
        sizes = [(int(h), int(w)) for h, w in sizes]
        for h, w in sizes:
            if not (0 <= h < 2 ** 32 and 0 <= w < 2 ** 32):
                raise ValueError("set_resize: sizes must fit 32 bits")
        ws = (C.c_uint32 * max(self.n_out, 1))(*[w for _, w in sizes])
        hs = (C.c_uint32 * max(self.n_out, 1))(*[h for h, _ in sizes])
        self.ctx._check(self.L.pjd_batch_set_resize(self._h, ws, hs), "pjd_batch_set_resize")
        self._resize = sizes

    def set_resize_pad(self, pads, fill=(0, 0, 0)):
        """pjd_batch_set_resize_pad: picture i fills only the rectangle of its canvas (the size of set_resize()) that pads[i] leaves, and
        the rest is `fill` (three bytes, R G B) -- C = paste(D, left, top) of include/pjd.h, inside the resample launch and the border
        launch behind it.  pads[i]: a ResizePad, None (the all-zero record), or a dict / tuple of its fields (left, top, right, bottom).
        From then on "the target" of every later call is the content, canvas less pad.  Once, after set_resize() and before
        set_orientation() / set_resize_window() / set_resize_filter() / set_normalize() / bind_output() / upload()."""
        if len(pads) != self.n_out:
            raise ValueError("set_resize_pad: one pad (or None) per picture (per view after set_views)")
        if len(fill) != 3 or any(not 0 <= int(v) <= 255 or int(v) != v for v in fill):
            raise ValueError("set_resize_pad: the fill is three bytes (R, G, B)")
        arr = (ResizePad * max(self.n_out, 1))()
        for i, p in enumerate(pads):
            if p is not None:
                arr[i] = resize_pad(p)
        fl = (C.c_uint8 * 3)(*[int(v) for v in fill])
        self.ctx._check(self.L.pjd_batch_set_resize_pad(self._h, arr, fl), "pjd_batch_set_resize_pad")

    def set_pad_value(self, values):
        """pjd_batch_set_pad_value: the border elements of a padded, normalised batch are values[c], converted once to the batch's
        dtype, instead of the normalised fill ((0, 0, 0): zeros after normalisation).  Once, after set_normalize() on a batch that took
        set_resize_pad(), before bind_output() / upload()."""
        if len(values) != 3:
            raise ValueError("set_pad_value: three values (R, G, B)")
        va = (C.c_float * 3)(*[float(v) for v in values])
        self.ctx._check(self.L.pjd_batch_set_pad_value(self._h, va), "pjd_batch_set_pad_value")

    def set_orientation(self, orientations):
        """pjd_batch_set_orientation: picture i is delivered in EXIF orientation orientations[i] (1..8; Scanned.orientation, or a value of
        the caller's: 4 is a vertical flip, 6 and 8 the quarter turns) -- D = H^h(V^v(T^t(Q))) of include/pjd.h, inside the resample
        launch.  The sizes of set_resize() are those of the DELIVERED pictures; for 5..8 the resample's own target is (w, h), and that
        is what later windows speak about.  Once, after set_resize() and before set_resize_window() / set_resize_filter() /
        set_normalize() / bind_output() / upload()."""
        if len(orientations) != self.n_out:
            raise ValueError("set_orientation: one orientation per picture (per view after set_views)")
        vals = [int(o) for o in orientations]
        if any(not 0 <= o <= 255 for o in vals):
            raise ValueError("set_orientation: orientations are 1..8")
        arr = (C.c_uint8 * max(self.n_out, 1))(*vals)
        self.ctx._check(self.L.pjd_batch_set_orientation(self._h, arr), "pjd_batch_set_orientation")

    def set_resize_window(self, windows):
        """pjd_batch_set_resize_window: picture i is resampled from a window of the decoded picture to a window of a virtual target,
        mirrored where asked -- flip(resize(P[y:y+h, x:x+w], vw, vh)[oy:oy+th, ox:ox+tw]), the arithmetic include/pjd.h specifies.
        windows[i]: a ResizeWindow, None (the whole picture: the all-zero record), or a dict / tuple of its fields (x, y, w, h, vw, vh,
        ox, oy, flags).  Once, after set_resize() and before set_resize_filter() / set_normalize() / bind_output() / upload()."""
        if len(windows) != self.n_out:
            raise ValueError("set_resize_window: one window (or None) per picture (per view after set_views)")
        arr = (ResizeWindow * max(self.n_out, 1))()
        for i, w in enumerate(windows):
            if w is not None:
                arr[i] = resize_window(w)
        self.ctx._check(self.L.pjd_batch_set_resize_window(self._h, arr), "pjd_batch_set_resize_window")

    def set_resize_affine(self, matrices, fill=(0, 0, 0)):
        """pjd_batch_set_resize_affine: output i is read from its picture under matrices[i] = (m00, m01, m02, m10, m11, m12), the INVERSE
        map from the centres of its target pixels (the size of set_resize()) to source pixel centres at the decode size, bilinear in the
        fixed point include/pjd.h specifies bit for bit, with `fill` (three bytes, R G B; grey reads the first) where a tap lies outside
        the picture: rotation, scale, shear and translation in one launch.  An alternative to set_resize_pad() / set_orientation() /
        set_resize_window() / set_resize_filter(), which it excludes and which exclude it.  Once, after set_resize() (and set_views()),
        before set_normalize() / bind_output() / upload()."""
        if len(matrices) != self.n_out:
            raise ValueError("set_resize_affine: one matrix of six values per picture (per view after set_views)")
        if len(fill) != 3 or any(not 0 <= int(v) <= 255 or int(v) != v for v in fill):
            raise ValueError("set_resize_affine: the fill is three bytes (R, G, B)")
        arr = ((C.c_double * 6) * max(self.n_out, 1))()
        for i, m in enumerate(matrices):
            arr[i] = _affine6(m, "set_resize_affine")
        fl = (C.c_uint8 * 3)(*[int(v) for v in fill])
        self.ctx._check(self.L.pjd_batch_set_resize_affine(self._h, arr, fl), "pjd_batch_set_resize_affine")

    def set_colour(self, matrices):
        """pjd_batch_set_colour: output i's resampled 8-bit triple goes through the 3 x 4 map matrices[i] -- twelve values, row-major,
        out[c] = m[4c] * R + m[4c + 1] * G + m[4c + 2] * B + m[4c + 3] with the last column in 8-bit levels (or three rows of four; None:
        the identity) -- in the Q16 fixed point include/pjd.h specifies bit for bit, inside the resample or warp launch, before the
        normalisation and the store: ColorJitter, RandomGrayscale, BGR, DALI's color_twist (tensors.colour_matrix builds the numbers).
        The border of set_resize_pad() keeps its fill; the fill of set_resize_affine() passes through the map.  Once, after set_resize()
        (and whatever shapes the resample), before set_normalize() / bind_output() / upload(); not on a grey batch."""
        if len(matrices) != self.n_out:
            raise ValueError("set_colour: one matrix of twelve values (or None) per picture (per view after set_views)")
        arr = ((C.c_double * 12) * max(self.n_out, 1))()
        for i, m in enumerate(matrices):
            arr[i] = _colour12(COLOUR_IDENTITY if m is None else m, "set_colour")
        self.ctx._check(self.L.pjd_batch_set_colour(self._h, arr), "pjd_batch_set_colour")

    def set_blur(self, blurs):
        """pjd_batch_set_blur: output i leaves as the separable Gaussian of what the batch would deliver without the call -- blurs[i] =
        (ksize, sigma), ksize odd and at most BLUR_MAX_TAPS, or None for no blur -- with the taps, the reflect border and the unsigned
        fixed point include/pjd.h specifies bit for bit (blur_taps, blur_index), in one launch behind the resample or warp and before the
        normalisation: torchvision's GaussianBlur to within 1 level, not Pillow's.  Once, after set_resize() (and whatever shapes the
        resample, set_colour() included), before set_normalize() / bind_output() / upload(); not on a batch with set_resize_pad()."""
        if len(blurs) != self.n_out:
            raise ValueError("set_blur: one (ksize, sigma) (or None) per picture (per view after set_views)")
        arr = (Blur * max(self.n_out, 1))()
        for i, e in enumerate(blurs):
            arr[i] = Blur(0.0, 0, 0) if e is None else Blur(float(e[1]), int(e[0]), 0)
        self.ctx._check(self.L.pjd_batch_set_blur(self._h, arr), "pjd_batch_set_blur")

    def set_resize_filter(self, filter):
        """pjd_batch_set_resize_filter: RESIZE_ANTIALIAS makes the resize the widened triangle filter include/pjd.h specifies bit for
        bit (torch's antialias=True, Pillow's BILINEAR), RESIZE_BICUBIC the bicubic one (Keys, a = -0.5, widened where an axis shrinks:
        Pillow's BICUBIC, torch's mode="bicubic" with antialias=True); RESIZE_BILINEAR is what a batch has without the call.  Once, after
        set_resize() and before set_normalize() / bind_output() / upload(); a picture more than 16x its target on an axis at its
        decode size is refused."""
        self.ctx._check(self.L.pjd_batch_set_resize_filter(self._h, int(filter)), "pjd_batch_set_resize_filter")

    def set_normalize(self, dtype, scale, bias):
        """pjd_batch_set_normalize: every sample v of channel c leaves the decode as fma(v, scale[c], bias[c]) in `dtype` (DT_F16,
        DT_BF16, DT_F32), the arithmetic include/pjd.h specifies bit for bit; scale[c] = 1 / (255 * std[c]), bias[c] = -mean[c] / std[c]
        (tensors.normalize_constants).  Once, after set_resize() if that is used, before bind_output() / upload(); not for OUT_BMP,
        not for shards.  Sizes, offsets and bind_output speak about elements of 2 or 4 bytes from then on; download() returns
        np.float16 / np.float32 arrays, and np.uint16 (the raw bits) for DT_BF16."""
        if len(scale) != 3 or len(bias) != 3:
            raise ValueError("set_normalize: three scales and three biases (R, G, B)")
        sc = (C.c_float * 3)(*[float(v) for v in scale])
        bi = (C.c_float * 3)(*[float(v) for v in bias])
        self.ctx._check(self.L.pjd_batch_set_normalize(self._h, int(dtype), sc, bi), "pjd_batch_set_normalize")
        self._dtype = int(dtype)

    def bind_output(self, device_ptr, capacity, offsets=None):
        """pjd_batch_bind_output: pictures go into caller-owned device memory (`device_ptr`: a plain integer address, e.g. a
        torch tensor's data_ptr(); `capacity` bytes) instead of a buffer of the batch.  `offsets`: byte offset of every picture,
        or None for the packed layout (output_offset(i)).  Before upload(); not for OUT_BMP.  The caller keeps the memory alive
        for as long as the batch decodes, and orders its own streams against the context's (sync())."""
        arr = None
        if offsets is not None:
            if len(offsets) != self.n_out:
                raise ValueError("bind_output: one offset per picture (per view after set_views)")
            arr = (C.c_uint64 * max(self.n_out, 1))(*[int(o) for o in offsets])
        self.ctx._check(self.L.pjd_batch_bind_output(self._h, C.c_void_p(int(device_ptr)), int(capacity), arr), "pjd_batch_bind_output")

    def statuses(self):
        """The status words of the last decode, without the pictures (synchronises)."""
        st = (C.c_int32 * max(self.n, 1))()
        self.ctx._check(self.L.pjd_batch_download(self._h, None, st), "pjd_batch_download")
        return [int(st[i]) for i in range(self.n)]

    def download(self):
        outs = [np.zeros(self.output_size(i), np.uint8) for i in range(self.n_out)]
        ptrs = (C.c_void_p * max(self.n_out, 1))(*[o.ctypes.data for o in outs])
        st = (C.c_int32 * max(self.n, 1))()
        self.ctx._check(self.L.pjd_batch_download(self._h, ptrs, st), "pjd_batch_download")
        if self._dtype is not None:                # normalised: elements of 2 or 4 bytes (bf16 as its raw bits: numpy has no such type)
            outs = [o.view({DT_F16: np.float16, DT_BF16: np.uint16, DT_F32: np.float32}[self._dtype]) for o in outs]
        outs = [o.reshape(self.output_shape(i)) for i, o in enumerate(outs)]
        return outs, [int(st[i]) for i in range(self.n)]


    def coefficients(self, i):
        """Stage-level parity: image i's coefficients after entropy decoding, in the reference's MCU_buffer layout
        (n_dpus x 19200 int16, reference src/jpeg_scanner.cpp:733-741)."""
        d = self._descs[i]
        n = int(self.L.pjd_coefficients_size(d.width, d.height, d.h_samp, d.v_samp))
        out = np.zeros(n, np.int16)
        self.ctx._check(self.L.pjd_batch_download_coefficients(self._h, i, out.ctypes.data, n), "pjd_batch_download_coefficients")
        return out.reshape(-1, 19200)

    def download_packed(self):
        """All pictures in one D2H copy into page-locked memory; returns (list of arrays, statuses)."""
        size = int(self.L.pjd_batch_packed_size(self._h))
        host = self.L.pjd_host_alloc(size)
        if not host:
            raise PjdError("pjd_host_alloc failed")
        try:
            st = (C.c_int32 * max(self.n, 1))()
            self.ctx._check(self.L.pjd_batch_download_packed(self._h, host, size, st), "pjd_batch_download_packed")
            whole = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint8)), shape=(size,))
            outs = []
            for i in range(self.n_out):
                off, n = int(self.L.pjd_batch_output_offset(self._h, i)), self.output_size(i)
                outs.append(whole[off:off + n].copy())
        finally:
            self.L.pjd_host_free(host)
        return outs, [int(st[i]) for i in range(self.n)]


# ---- pipelined batcher (include/pjd_pipeline.h) ---------------------------------------------
SINK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint8), C.c_uint64)


class PipeOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("out_format", C.c_int32), ("batch_images", C.c_int32),
                ("scan_threads", C.c_int32), ("slots", C.c_int32), ("sink_threads", C.c_int32),
                ("sink", SINK_FN), ("sink_user", C.c_void_p),
                ("devices", C.POINTER(C.c_int32)), ("n_devices", C.c_int32), ("scan_options", C.c_uint32),
                ("image_flags", C.c_uint32)]


PIPE_MAX_DEVICES = 16


class PipeStats(C.Structure):
    _fields_ = [("wall_s", C.c_double), ("scan_s", C.c_double), ("create_s", C.c_double), ("upload_s", C.c_double),
                ("exec_s", C.c_double), ("download_s", C.c_double), ("sink_s", C.c_double),
                ("n_inputs", C.c_uint64), ("n_decoded", C.c_uint64), ("n_rejected", C.c_uint64),
                ("n_batches", C.c_uint64), ("n_batch_failures", C.c_uint64),
                ("pixels", C.c_uint64), ("in_bytes", C.c_uint64), ("ecs_bytes", C.c_uint64), ("out_bytes", C.c_uint64),
                ("n_devices", C.c_uint64), ("n_stolen", C.c_uint64),
                ("device_batches", C.c_uint64 * PIPE_MAX_DEVICES), ("device_in_bytes", C.c_uint64 * PIPE_MAX_DEVICES),
                ("n_exact_images", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.startswith("device_") else getattr(self, k)) for k, _ in self._fields_}


_pipe = None


def pipe_lib():
    global _pipe
    if _pipe is None:
        if not os.path.exists(LIBPIPE):
            raise PjdError(f"{LIBPIPE} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        dev_lib(), host_lib()
        L = C.CDLL(LIBPIPE)
        L.pjd_pipe_run_files.restype = C.c_int
        L.pjd_pipe_run_files.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(PipeOpts), C.POINTER(PipeStats)]
        L.pjd_pipe_run_memory.restype = C.c_int
        L.pjd_pipe_run_memory.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_char_p), C.c_int,
                                          C.POINTER(PipeOpts), C.POINTER(PipeStats)]
        L.pjd_pipe_release.restype = None
        L.pjd_pipe_assign.restype = C.c_int
        L.pjd_pipe_assign.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_int32)]
        _pipe = L
    return _pipe


def pipe_release():
    if _pipe is not None:
        _pipe.pjd_pipe_release()


def pipe_assign(costs, n_devices):
    """The batcher's dealing rule (pjd_pipe_assign): device index per item, longest first onto the least loaded."""
    L = pipe_lib()
    n = len(costs)
    c = (C.c_uint64 * max(n, 1))(*[int(x) for x in costs])
    out = (C.c_int32 * max(n, 1))()
    rc = L.pjd_pipe_assign(c, n, n_devices, out)
    if rc != 0:
        raise PjdError(f"pjd_pipe_assign failed ({rc})")
    return [int(out[k]) for k in range(n)]


def pipe_run(jpegs=None, names=None, paths=None, out_format=OUT_BMP, batch_images=1024, scan_threads=0, slots=0,
             sink_threads=0, sink=None, device=0, devices=None, scan_options=0, image_flags=0):
    """Run the pipelined batcher over in-memory JPEGs (`jpegs`: list of bytes) or files (`paths`).
    `devices`: HIP ordinals to spread the batches over (default: `device` alone).
    `image_flags`: PJD_F_* ORed into every descriptor (F_SCALE_*: the sink receives reduced-size pictures; F_LIBJPEG: libjpeg's
    pictures -- a picture outside that mode's envelope reaches the sink with status -2, no data and the planner's reason as the last
    line of its log, and the rest of its batch decodes).

    `sink(index, name, log, status, data)` is called from worker threads with `data` a numpy copy of the
    picture (or None).  Returns the statistics as a dict."""
    L = pipe_lib()
    o = PipeOpts()
    o.device, o.out_format, o.batch_images = device, out_format, batch_images
    o.scan_threads, o.slots, o.sink_threads = scan_threads, slots, sink_threads
    o.scan_options = scan_options
    o.image_flags = image_flags
    if devices is not None:
        dv = (C.c_int32 * max(len(devices), 1))(*[int(d) for d in devices])
        o.devices, o.n_devices = C.cast(dv, C.POINTER(C.c_int32)), len(devices)

    def _tramp(user, index, name, log, status, data, length):
        pic = np.ctypeslib.as_array(data, shape=(length,)).copy() if data and length else None
        sink(index, name.decode(), log.decode(), status, pic)

    cb = SINK_FN(_tramp) if sink else SINK_FN()
    o.sink = cb
    st = PipeStats()
    if paths is not None:
        arr = (C.c_char_p * max(len(paths), 1))(*[p.encode() for p in paths])
        rc = L.pjd_pipe_run_files(arr, len(paths), C.byref(o), C.byref(st))
    else:
        n = len(jpegs)
        keep = [np.frombuffer(j, np.uint8) for j in jpegs]
        ptrs = (C.c_void_p * max(n, 1))(*[k.ctypes.data for k in keep])
        lens = (C.c_uint64 * max(n, 1))(*[len(j) for j in jpegs])
        nm = (C.c_char_p * max(n, 1))(*[(names[i] if names else f"mem{i}.jpg").encode() for i in range(n)])
        rc = L.pjd_pipe_run_memory(ptrs, lens, nm, n, C.byref(o), C.byref(st))
    if rc != 0:
        raise PjdError(f"pipeline failed ({rc})")
    return st.as_dict()


def split_decode(desc, devices, out_format=OUT_RGB8):
    """pjd_split_decode: ONE picture over several devices (restart-segment ranges, RCCL broadcast of the descriptor).
    -> (picture as np.uint8 array, status, stats dict)."""
    L = dev_lib()
    n = int(L.pjd_image_output_size(C.byref(desc), out_format))
    out = np.zeros(n, np.uint8)
    dv = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    st, status = SplitStats(), C.c_int32(0)
    rc = L.pjd_split_decode(C.byref(desc), dv, len(devices), out_format, out.ctypes.data, n, C.byref(status), C.byref(st))
    if rc != 0:
        raise PjdError(f"pjd_split_decode failed ({rc})")
    if out_format == OUT_RGB8:
        out = out.reshape(*reversed(scaled_dims(desc.width, desc.height, desc.flags)), 3)
    elif out_format == OUT_RGB8_PLANAR:
        out = out.reshape(3, *reversed(scaled_dims(desc.width, desc.height, desc.flags)))
    return out, int(status.value), st.as_dict()


def split_plan(desc, world, rank):
    """pjd_split_plan (host only) -> None if the rank has no segment, else dict(first_seg, n_segs, byte_lo, byte_hi, first_mcu, last_mcu,
    seg_offsets of the shard descriptor, ecs_len of the shard)."""
    L = dev_lib()
    shard = ImageDesc()
    scratch = np.zeros(max(int(desc.n_segments), 1), np.uint64)
    lo, hi, m0, m1 = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
    rc = L.pjd_split_plan(C.byref(desc), world, rank, C.byref(shard), scratch.ctypes.data, C.byref(lo), C.byref(hi), C.byref(m0), C.byref(m1))
    if rc == 1:
        return None
    if rc != 0:
        raise PjdError(f"pjd_split_plan failed ({rc})")
    return {"first_seg": int(shard.shard_first_seg), "n_segs": int(shard.shard_n_segs), "byte_lo": lo.value, "byte_hi": hi.value,
            "first_mcu": m0.value, "last_mcu": m1.value, "seg_offsets": scratch.copy(), "ecs_len": int(shard.ecs_len),
            "ecs_delta": (int(shard.ecs or 0) - int(desc.ecs or 0))}


def plan_step_bits(desc):
    """Host-only, debug: fewest bits of stream per write-pass step the picture's tables can be made to sustain (a float; pjd.h)."""
    L = dev_lib()
    L.pjd_plan_step_bits.restype = C.c_int32
    L.pjd_plan_step_bits.argtypes = [C.POINTER(ImageDesc), C.POINTER(C.c_uint32)]
    v = C.c_uint32()
    rc = L.pjd_plan_step_bits(C.byref(desc), C.byref(v))
    if rc != 0:
        raise PjdError(f"pjd_plan_step_bits failed ({rc})")
    return v.value / 256.0


def plan_luts(desc):
    """Host-only, debug (pjd_plan_luts): the decode tables of the picture's table set as the entropy decoder holds them in LDS ->
    (blob as np.uint8 of the real size, nominal size -- the one that routes the set --, slots as a [3][2] list: [component][DC, AC] ->
    first-level table).  An empty blob: the set takes the exact kernel."""
    L = dev_lib()
    L.pjd_plan_luts.restype = C.c_int32
    L.pjd_plan_luts.argtypes = [C.POINTER(ImageDesc), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
    real, nominal = C.c_uint32(), C.c_uint32()
    slots = np.zeros(6, np.uint8)
    blob = np.zeros(6 * 2048 + 8192 + 16, np.uint8)          # PJD_LUT_LDS_MAX: no blob is larger
    rc = L.pjd_plan_luts(C.byref(desc), blob.ctypes.data, blob.size, C.byref(real), C.byref(nominal), slots.ctypes.data)
    if rc != 0:
        raise PjdError(f"pjd_plan_luts failed ({rc})")
    return blob[: real.value].copy(), int(nominal.value), slots.reshape(3, 2).tolist()


def plan_info(descs, out_format=OUT_RGB8):
    """Host-only: what a batch of these images would occupy (no GPU needed)."""
    L = dev_lib()
    arr = (ImageDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(ImageDesc))
    bi = BatchInfo()
    rc = L.pjd_plan_info(arr, len(descs), out_format, C.byref(bi))
    if rc != 0:
        raise PjdError(f"pjd_plan_info failed ({rc})")
    return {k: (list(getattr(bi, k)) if k == "flag_waves" else (float(getattr(bi, k)) if k == "exact_fallback_ms" else int(getattr(bi, k)))) for k, _ in bi._fields_}


def plan_check(descs, out_format=OUT_RGB8):
    """Host-only (pjd_plan_check): would a batch take these images?  -> (code, reason): (0, "") or the planner's refusal, which names
    the picture -- what the batcher and the CLI ask, picture by picture, before they OR image_flags into a whole batch."""
    L = dev_lib()
    arr = (ImageDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(ImageDesc))
    text = C.create_string_buffer(256)
    rc = L.pjd_plan_check(arr, len(descs), out_format, text, len(text))
    return int(rc), text.value.decode()


def resize_tap(src_n, dst_n, i):
    """pjd_resize_tap (host only): (i0, i1, w) -- the two source samples target sample i of dst_n reads over src_n source samples,
    and the weight of i1 in 1/256; the code the resize kernel runs.  ValueError outside 1..65535 / i >= dst_n."""
    a, b, w = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if not all(0 <= int(v) < 2 ** 32 for v in (src_n, dst_n, i)) or dev_lib().pjd_resize_tap(int(src_n), int(dst_n), int(i), C.byref(a), C.byref(b), C.byref(w)) != 0:
        raise ValueError(f"resize_tap({src_n}, {dst_n}, {i}): sizes must be 1..65535 and i < dst_n")
    return a.value, b.value, w.value


def resize_aa_taps(src_n, dst_n, i):
    """pjd_resize_aa_taps (host only): (first, [q ...]) -- the first source sample target sample i of dst_n reads over src_n source
    samples with the antialiased filter, and the weights of that sample and the following ones in 1/65536 (they sum to 65536); the
    code the batch's weight table is built with.  ValueError outside 1..65535, for i >= dst_n and for src_n > 16 * dst_n."""
    first, count, q = C.c_uint32(), C.c_uint32(), (C.c_uint32 * AA_MAX_TAPS)()
    if not all(0 <= int(v) < 2 ** 32 for v in (src_n, dst_n, i)) or dev_lib().pjd_resize_aa_taps(int(src_n), int(dst_n), int(i), C.byref(first), C.byref(count), q) != 0:
        raise ValueError(f"resize_aa_taps({src_n}, {dst_n}, {i}): sizes must be 1..65535, i < dst_n and src_n <= 16 * dst_n")
    return first.value, list(q[:count.value])


def resize_bicubic_taps(src_n, dst_n, i):
    """pjd_resize_bicubic_taps (host only): (first, [q ...]) -- the first source sample in the support of target sample i of dst_n over
    src_n source samples with the bicubic filter, and the SIGNED weights of that sample and the following ones in 1/65536 (they sum to
    65536; a weight inside the support may be 0); the code the batch's weight table is built with.  ValueError outside 1..65535, for
    i >= dst_n and for src_n > 16 * dst_n."""
    first, count, q = C.c_uint32(), C.c_uint32(), (C.c_int32 * BICUBIC_MAX_TAPS)()
    if not all(0 <= int(v) < 2 ** 32 for v in (src_n, dst_n, i)) or dev_lib().pjd_resize_bicubic_taps(int(src_n), int(dst_n), int(i), C.byref(first), C.byref(count), q) != 0:
        raise ValueError(f"resize_bicubic_taps({src_n}, {dst_n}, {i}): sizes must be 1..65535, i < dst_n and src_n <= 16 * dst_n")
    return first.value, list(q[:count.value])


def _affine6(m, who):
    """six doubles from a flat sequence of six or from two rows of three"""
    vals = [float(v) for row in m for v in (row if hasattr(row, "__len__") else (row,))]
    if len(vals) != 6:
        raise ValueError(f"{who}: a matrix is six values (m00, m01, m02, m10, m11, m12), or two rows of three")
    return (C.c_double * 6)(*vals)


def warp_tap(m, i, j):
    """pjd_warp_tap (host only): (x0, y0, wx, wy) -- the top-left source sample (either may be negative) target pixel (i, j), column i and
    row j, reads under the inverse map m of six values, and the weights of x0 + 1 and y0 + 1 in 1/256; the code the warp kernel runs.
    ValueError for a matrix that is not finite or beyond the limits, and for i or j at or above 65535."""
    x0, y0, wx, wy = C.c_int64(), C.c_int64(), C.c_uint32(), C.c_uint32()
    if not all(0 <= int(v) < 2 ** 32 for v in (i, j)) or dev_lib().pjd_warp_tap(_affine6(m, "warp_tap"), int(i), int(j), C.byref(x0), C.byref(y0), C.byref(wx), C.byref(wy)) != 0:
        raise ValueError(f"warp_tap({list(m)}, {i}, {j}): the matrix must be finite and within the limits, i and j below 65535")
    return x0.value, y0.value, wx.value, wy.value


def resize_affine_check(sw, sh, tw, th, m):
    """pjd_resize_affine_check (host only): True where pjd_batch_set_resize_affine would accept the inverse map m (six values) for a
    picture of sw x sh at its decode size and a target of tw x th."""
    if not all(0 <= int(v) < 2 ** 32 for v in (sw, sh, tw, th)):
        return False
    return dev_lib().pjd_resize_affine_check(int(sw), int(sh), int(tw), int(th), _affine6(m, "resize_affine_check")) == 0


COLOUR_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _colour12(m, who):
    """twelve doubles from a flat sequence of twelve or from three rows of four"""
    vals = [float(v) for row in m for v in (row if hasattr(row, "__len__") else (row,))]
    if len(vals) != 12:
        raise ValueError(f"{who}: a colour map is twelve values (row-major 3 x 4), or three rows of four")
    return (C.c_double * 12)(*vals)


def colour_value(m, rgb):
    """pjd_colour_value (host only): the triple (R', G', B') the 3 x 4 colour map m makes of the 8-bit triple rgb; the code the coloured
    kernels run.  ValueError for a map that is not finite or beyond the limits (|weight| <= 16, |offset| <= 4096 levels)."""
    if len(rgb) != 3 or any(not 0 <= int(v) <= 255 for v in rgb):
        raise ValueError(f"colour_value: rgb is three bytes, not {list(rgb)}")
    out = (C.c_uint8 * 3)()
    if dev_lib().pjd_colour_value(_colour12(m, "colour_value"), (C.c_uint8 * 3)(*[int(v) for v in rgb]), out) != 0:
        raise ValueError(f"colour_value({list(m)}): the map must be finite and within the limits")
    return out[0], out[1], out[2]


def blur_taps(ksize, sigma):
    """pjd_blur_taps (host only): the ksize taps, in 1/65536, of the Gaussian of Batch.set_blur -- symmetric, non-negative, summing to
    65536 exactly; the table the blur kernel reads."""
    ksize = int(ksize)
    q = (C.c_uint32 * max(ksize, 1))()
    if not 0 < ksize < 2 ** 32 or dev_lib().pjd_blur_taps(ksize, float(sigma), q) != 0:
        raise ValueError(f"blur_taps({ksize}, {sigma}): ksize is odd and at most {BLUR_MAX_TAPS}, sigma finite and greater than 0")
    return list(q)


def blur_index(n, i):
    """pjd_blur_index (host only): the sample that index i of an axis of n samples reads under the border rule of Batch.set_blur
    (torchvision's reflect, folded as often as it takes)."""
    src = C.c_uint32()
    if not 0 < int(n) < 2 ** 32 or not -2 ** 63 <= int(i) < 2 ** 63 or dev_lib().pjd_blur_index(int(n), int(i), C.byref(src)) != 0:
        raise ValueError(f"blur_index({n}, {i}): n is 1..65535")
    return src.value


def blur_check(ksize, sigma, reserved=0):
    """pjd_blur_check (host only): True where pjd_batch_set_blur would accept the entry (ksize, sigma); (0, 0.0) is no blur."""
    return dev_lib().pjd_blur_check(C.byref(Blur(float(sigma), int(ksize) & 0xffffffff, int(reserved)))) == 1


def colour_check(m):
    """pjd_colour_check (host only): True where pjd_batch_set_colour would accept the 3 x 4 colour map m (twelve values)."""
    return dev_lib().pjd_colour_check(_colour12(m, "colour_check")) == 1


def resize_window(w):
    """A ResizeWindow from a ResizeWindow (copied), a dict of its fields, or a tuple (x, y, w, h[, vw, vh, ox, oy, flags]).  ValueError
    for a field outside 32 bits."""
    if isinstance(w, ResizeWindow):
        vals = [getattr(w, k) for k, _ in ResizeWindow._fields_]
    elif isinstance(w, dict):
        if set(w) - {k for k, _ in ResizeWindow._fields_}:
            raise ValueError(f"resize_window: unknown fields {sorted(set(w) - {k for k, _ in ResizeWindow._fields_})}")
        vals = [w.get(k, 0) for k, _ in ResizeWindow._fields_]
    else:
        vals = list(w) + [0] * (10 - len(w))
        if not 4 <= len(w) <= 10 or vals[9] != 0:
            raise ValueError("resize_window: (x, y, w, h[, vw, vh, ox, oy, flags])")
    if not all(0 <= int(v) < 2 ** 32 for v in vals):
        raise ValueError("resize_window: every field must fit 32 bits")
    return ResizeWindow(*[int(v) for v in vals])


def resize_pad(p):
    """A ResizePad from a ResizePad (copied), a dict of its fields, or a tuple (left, top, right, bottom).  ValueError for anything else."""
    names = [k for k, _ in ResizePad._fields_]
    if isinstance(p, ResizePad):
        vals = [getattr(p, k) for k in names]
    elif isinstance(p, dict):
        if set(p) - set(names):
            raise ValueError(f"resize_pad: unknown fields {sorted(set(p) - set(names))}")
        vals = [p.get(k, 0) for k in names]
    else:
        vals = list(p)
        if len(vals) != 4:
            raise ValueError("resize_pad: (left, top, right, bottom)")
    if any(not 0 <= int(v) < 2 ** 32 for v in vals):
        raise ValueError("resize_pad: every field must fit 32 bits")
    return ResizePad(*[int(v) for v in vals])


def resize_pad_check(out_w, out_h, pad):
    """pjd_resize_pad_check (host only): True where pjd_batch_set_resize_pad would accept `pad` (anything resize_pad() takes; None: the
    null record, which it refuses) for a canvas of out_w x out_h."""
    if not (0 <= int(out_w) < 2 ** 32 and 0 <= int(out_h) < 2 ** 32):
        return False
    ref = None if pad is None else C.byref(resize_pad(pad))
    return dev_lib().pjd_resize_pad_check(int(out_w), int(out_h), ref) == 0


def resize_window_check(sw, sh, tw, th, window, filter=RESIZE_BILINEAR):
    """pjd_resize_window_check (host only): True where pjd_batch_set_resize_window (and, with RESIZE_ANTIALIAS or RESIZE_BICUBIC, set_resize_filter) would
    accept `window` (anything resize_window() takes; None: the all-zero record) for a picture of sw x sh at its decode size and a target
    of tw x th; the one implementation of the rules of include/pjd.h."""
    if not all(0 <= int(v) < 2 ** 32 for v in (sw, sh, tw, th)):
        return False
    rec = ResizeWindow() if window is None else resize_window(window)
    return dev_lib().pjd_resize_window_check(int(sw), int(sh), int(tw), int(th), C.byref(rec), int(filter)) == 0


def normalize_value(dtype, v, scale, bias):
    """pjd_normalize_value (host only): the bits of one normalised sample, as an int of 16 (DT_F16, DT_BF16) or 32 (DT_F32) bits -- the
    fma the kernel runs, then the conversion include/pjd.h specifies.  ValueError for what the library refuses."""
    out = (C.c_uint8 * 4)()
    if not 0 <= int(v) < 2 ** 32 or dev_lib().pjd_normalize_value(int(dtype), int(v), float(scale), float(bias), out) != 0:
        raise ValueError(f"normalize_value({dtype}, {v}, {scale}, {bias}): dtype DT_F16 / DT_BF16 / DT_F32, v <= 255, finite constants")
    return int.from_bytes(bytes(out[:4 if int(dtype) == DT_F32 else 2]), "little")


def libjpeg_idct(coef, q):
    """pjd_libjpeg_idct (host only): the 64 samples (uint8, natural order) of one unit under F_LIBJPEG -- coef (int16) times q (uint16), both
    64 values in natural order, through libjpeg's islow IDCT; the inlines the kernel runs."""
    c = np.ascontiguousarray(np.asarray(coef).reshape(64), np.int16)
    qq = np.ascontiguousarray(np.asarray(q).reshape(64), np.uint16)
    out = np.empty(64, np.uint8)
    if dev_lib().pjd_libjpeg_idct(c.ctypes.data_as(C.POINTER(C.c_int16)), qq.ctypes.data_as(C.POINTER(C.c_uint16)), out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise ValueError("libjpeg_idct: 64 coefficients and 64 quantisers")
    return out


def libjpeg_idct_scaled(coef, q, n):
    """pjd_libjpeg_idct_scaled (host only): the n x n samples (uint8, row by row) of one unit under F_LIBJPEG_SCALE_* -- n = 8 (full size), 4,
    2 or 1: libjpeg's reduced IDCTs; the inlines the kernels run.  ValueError for any other n."""
    c = np.ascontiguousarray(np.asarray(coef).reshape(64), np.int16)
    qq = np.ascontiguousarray(np.asarray(q).reshape(64), np.uint16)
    out = np.empty(64, np.uint8)
    if dev_lib().pjd_libjpeg_idct_scaled(c.ctypes.data_as(C.POINTER(C.c_int16)), qq.ctypes.data_as(C.POINTER(C.c_uint16)), int(n) & 0xffffffff,
                                         out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise ValueError("libjpeg_idct_scaled: n is 8, 4, 2 or 1")
    return out[:int(n) * int(n)].copy()


def libjpeg_ycc_to_rgb(y, cb, cr):
    """pjd_libjpeg_ycc_to_rgb (host only): (R, G, B) of one pixel under F_LIBJPEG; y, cb, cr in 0..255."""
    if not all(0 <= int(v) <= 255 for v in (y, cb, cr)):
        raise ValueError("libjpeg_ycc_to_rgb: samples are 0..255")
    out = (C.c_uint8 * 3)()
    if dev_lib().pjd_libjpeg_ycc_to_rgb(int(y), int(cb), int(cr), out) != 0:
        raise ValueError("libjpeg_ycc_to_rgb refused")
    return out[0], out[1], out[2]


def libjpeg_upsample_row(cur, nb=None, v=0):
    """pjd_libjpeg_upsample_row (host only): the 2n samples of one output row of fancy upsampling under F_LIBJPEG from the chroma row `cur`
    (n samples) and, for 4:2:0, its neighbour row `nb` (the row above for v = 0, below for v = 1; None: 4:2:2)."""
    c = np.ascontiguousarray(np.asarray(cur).reshape(-1), np.uint8)
    nbp = None
    if nb is not None:
        nba = np.ascontiguousarray(np.asarray(nb).reshape(-1), np.uint8)
        if nba.size != c.size:
            raise ValueError("libjpeg_upsample_row: the two rows have one length")
        nbp = nba.ctypes.data_as(C.POINTER(C.c_uint8))
    out = np.empty(2 * c.size, np.uint8)
    if dev_lib().pjd_libjpeg_upsample_row(c.ctypes.data_as(C.POINTER(C.c_uint8)), nbp, int(v), c.size, out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise ValueError("libjpeg_upsample_row: at least one sample")
    return out


def scaled_dims(width, height, flags=0):
    """pjd_scaled_dims: (width, height) of the output picture at the scale the descriptor flags ask for (F_SCALE_*, F_LIBJPEG_SCALE_*)."""
    L = dev_lib()
    w, h = C.c_uint32(), C.c_uint32()
    L.pjd_scaled_dims(int(width), int(height), int(flags), C.byref(w), C.byref(h))
    return w.value, h.value


def output_channels(out_format):
    """pjd_output_channels (host only): 3 for OUT_RGB8, OUT_BMP and OUT_RGB8_PLANAR, 1 for OUT_GRAY8, 0 for a value that is no format."""
    return int(dev_lib().pjd_output_channels(int(out_format)))


def image_output_size(desc, out_format=OUT_RGB8):
    """pjd_image_output_size: bytes of the picture of one descriptor in `out_format`, at its output scale."""
    return int(dev_lib().pjd_image_output_size(C.byref(desc), out_format))
