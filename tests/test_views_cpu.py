"""Views on decode (pjd_batch_set_views), what needs no device: the exported symbols, the pure helpers of pjd_amd.tensors on
hand-computed cases, and the resolver of the resample work list under requests that repeat and permute their sources
(tools/resize_views_host.cpp, built with csrc/pjd_resize_plan.cpp under AddressSanitizer + UndefinedBehaviorSanitizer and run as a
process of its own, the way tests/test_resize_plan_cpu.py runs tools/resize_plan_host.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_symbols_are_exported():
    import pjd_amd
    L = pjd_amd.dev_lib()
    assert L.pjd_version() == 6
    for name in ("pjd_batch_set_views", "pjd_batch_n_outputs"):
        assert hasattr(L, name), name
    assert L.pjd_batch_n_outputs(None) == 0
    assert L.pjd_batch_set_views(None, (C.c_uint32 * 2)(0, 0), 2) == -3
    assert hasattr(pjd_amd.Batch, "set_views") and isinstance(pjd_amd.Batch.n_out, property)
    text = open(os.path.join(ROOT, "include", "pjd.h")).read()
    assert "#define PJD_MAX_VIEWS 65536u" in text and "#define PJD_VERSION 6" in text


def test_tile_views_on_hand_computed_cases():
    from pjd_amd import tensors
    # 10 rows x 7 columns in tiles of at most 4 x 4: columns 4 + 3, rows 4 + 4 + 2, row-major
    windows, sizes = tensors.tile_views(10, 7, 4, 4)
    assert sizes == [(4, 4), (4, 3), (4, 4), (4, 3), (2, 4), (2, 3)]
    assert windows == [dict(x=0, y=0, w=4, h=4), dict(x=4, y=0, w=3, h=4), dict(x=0, y=4, w=4, h=4), dict(x=4, y=4, w=3, h=4),
                       dict(x=0, y=8, w=4, h=2), dict(x=4, y=8, w=3, h=2)]
    # a picture that is one tile, one that divides evenly, one pixel, tiles larger than the picture on one axis
    assert tensors.tile_views(5, 9, 5, 9) == ([dict(x=0, y=0, w=9, h=5)], [(5, 9)])
    assert tensors.tile_views(4, 6, 2, 3)[1] == [(2, 3)] * 4
    assert tensors.tile_views(1, 1, 64, 64) == ([dict(x=0, y=0, w=1, h=1)], [(1, 1)])
    assert tensors.tile_views(3, 10, 64, 4) == ([dict(x=0, y=0, w=4, h=3), dict(x=4, y=0, w=4, h=3), dict(x=8, y=0, w=2, h=3)], [(3, 4), (3, 4), (3, 2)])
    # 400 rows x 264 columns in 64 x 64: 7 x 5 tiles, the last column 8 wide, the last row 16 high; they cover every pixel once
    windows, sizes = tensors.tile_views(400, 264, 64, 64)
    assert len(sizes) == 35 and sizes[0] == (64, 64) and sizes[4] == (64, 8) and sizes[30] == (16, 64) and sizes[34] == (16, 8)
    assert sum(h * w for h, w in sizes) == 400 * 264 and all((w["h"], w["w"]) == s for w, s in zip(windows, sizes))
    for bad in ((0, 5, 4, 4), (5, 0, 4, 4), (5, 5, 0, 4), (5, 5, 4, 0)):
        with pytest.raises(ValueError):
            tensors.tile_views(*bad)


def test_the_pre_scale_of_a_picture_is_the_least_reduced_of_its_views():
    import pjd_amd
    from pjd_amd import tensors
    F = pjd_amd
    assert tensors.least_reduced_scale_flags([F.F_SCALE_1_8, F.F_SCALE_1_2, F.F_SCALE_1_4]) == F.F_SCALE_1_2
    assert tensors.least_reduced_scale_flags([F.F_SCALE_1_8, 0]) == 0
    assert tensors.least_reduced_scale_flags([F.F_SCALE_1_4 | F.F_LIBJPEG]) == F.F_SCALE_1_4
    assert tensors.least_reduced_scale_flags([]) == F.F_SCALE_1_8
    assert tensors.least_reduced_scale_flags([F.F_LIBJPEG_SCALE_1_8, F.F_LIBJPEG_SCALE_1_4], draft=True) == F.F_LIBJPEG_SCALE_1_4
    assert tensors.least_reduced_scale_flags([], draft=True) == F.F_LIBJPEG_SCALE_1_8

    def desc(w, h, flags=0):
        d = pjd_amd.ImageDesc()
        d.width, d.height, d.flags = w, h, flags
        return d

    # 640 x 480 to 224 x 224 is 1/2 on its own (320 x 240; 1/4 is 160 x 120), a 300 x 300 crop of it is full size (1/2 is 150 x 150):
    # the picture is decoded at full size.  1000 x 800 is 1/2 (500 x 400; 1/4 is 250 x 200, too low); 64 x 64 has no view: 1/8.
    descs = [desc(640, 480), desc(1000, 800, F.F_SCALE_1_8 | F.F_STANDARD_RESTART), desc(64, 64)]
    run, windows, oris, pads = tensors.plan_views(descs, [0, 0, 1], (224, 224), True, [(0, 0, 640, 480), (10, 10, 300, 300), None], [0, 1, 0])
    assert [int(d.flags) for d in run] == [0, F.F_SCALE_1_2 | F.F_STANDARD_RESTART, F.F_SCALE_1_8]
    assert windows == [dict(x=0, y=0, w=640, h=480), dict(x=10, y=10, w=300, h=300, flags=F.RW_HFLIP), None] and oris is None and pads is None
    assert [int(d.flags) for d in descs] == [0, F.F_SCALE_1_8 | F.F_STANDARD_RESTART, 0], "the caller's descriptors are not touched"
    # two views of one picture that differ in scale: both windows are taken at the scale the picture is decoded at (1/2 of 640 x 480)
    run, windows, _, _ = tensors.plan_views([desc(640, 480)], [0, 0], (96, 96), True, [None, (101, 51, 201, 199)], None)
    assert int(run[0].flags) == F.F_SCALE_1_2                  # the whole picture alone: 1/4 (160 x 120); the crop: 1/2 (101 x 100)
    assert windows == [None, dict(x=50, y=25, w=101, h=100)]    # [101 >> 1, ceil(302 / 2)) x [51 >> 1, ceil(250 / 2))
    # prescale off: the descriptors' own flags hold, windows at those
    run, windows, _, _ = tensors.plan_views([desc(640, 480, F.F_SCALE_1_4)], [0, 0], (96, 96), False, [None, (100, 60, 200, 200)], None)
    assert run[0].flags == F.F_SCALE_1_4 and windows == [None, dict(x=25, y=15, w=50, h=50)]
    # libjpeg's own reduced decode
    run, _, _, _ = tensors.plan_views([desc(640, 480, F.F_LIBJPEG)], [0, 0], (96, 96), "draft", [None, (101, 51, 201, 199)], None)
    assert int(run[0].flags) == F.F_LIBJPEG | F.F_LIBJPEG_SCALE_1_2
    # per-view arguments have one entry per view, and a view names a picture
    with pytest.raises(ValueError):
        tensors.plan_views(descs, [0, 0, 1], (224, 224), True, [None, None], None)
    with pytest.raises(ValueError):
        tensors.plan_views(descs, [0, 3], (224, 224))
    with pytest.raises(ValueError):
        tensors.plan_views(descs, [], (224, 224))


def test_resolver_with_repeated_sources_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "resize_views_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__host__=", "-D__device__=",
           os.path.join(ROOT, "tools", "resize_views_host.cpp"), os.path.join(ROOT, "pim-jpeg-decoder_amd", "csrc", "pjd_resize_plan.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("this toolchain has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout and " 0 checks failed" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
