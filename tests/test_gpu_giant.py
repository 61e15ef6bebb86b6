"""Decode at the size limits (run with -m gpu on an MI355X): pictures of 1.6 GPix whose output passes 4 GiB inside ONE picture, plane or
canvas, in every back end and format; a stream of 2^29 - 1 entropy-coded bytes, whose last unit starts above bit 2^32 - 2^21; the
exact kernel's dense scratch, the libjpeg component planes, the resample's source, its destination and the views' offsets past 2^32.

Every case is one child process of tests/giant_torch_cases.py (torch first, one HIP runtime), which compares every byte on the
device against the period expectations of tests/giant_corpus.py -- the oracle port, the libjpeg model and the resize models, never
this library -- and keeps 4096 guard bytes of 0xA5 on either side of the bound output.  Nothing retries; a child that does not end
in 300 s fails its test.  What the cases measured on an MI355X is in profiles/size_limits.md."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "giant_torch_cases.py")


def run_case(*args):
    p = subprocess.run([sys.executable, CASES, *args], capture_output=True, text=True, timeout=300, cwd=HERE)
    assert p.returncode == 0 and f"CASE OK {args[0]}" in p.stdout, (args, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


# ---- 1: the back ends.  One member under one flag set a child, its formats one after the other ----------------------------------------
@pytest.mark.parametrize("member,flags,formats", [
    ("g444", 0, "rgb8,planar,gray"),
    ("g444", 0, "bmp"),
    ("g420_std", 1, "rgb8,planar"),                      # PJD_F_STANDARD_RESTART
    ("g422_tall", 1, "rgb8"),
    ("g422_tall", 64, "rgb8,planar,gray"),               # PJD_F_LIBJPEG
])
def test_back_ends_write_past_4_gib_inside_one_picture(member, flags, formats):
    out = run_case("backend", member, str(flags), formats)
    assert out.count("MEASURE") == 1 + len(formats.split(","))


# ---- 2: small pictures behind a giant ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["planar", "gray"])
def test_small_pictures_behind_a_giant(fmt):
    run_case("small_behind_giant", fmt)


# ---- 3: the stream limit ------------------------------------------------------------------------------------------------------------------
def test_stream_of_2_29_less_one_bytes():
    run_case("stream_limit")


def test_padding_behind_the_last_mcu_stays_on_the_lane_path():
    """The finding of the case above: its 180 KB of zero padding never self-synchronises, and before PjdDevImState::end_pos the flags
    of those waves sent the whole 1.6 GPix picture to the one-lane exact kernel (minutes).  The same padding behind a 203 x 213 picture."""
    run_case("padded_tail")


def test_coefficients_of_the_last_dpus_of_the_longest_stream():
    run_case("stream_limit_coefficients")


def test_erring_symbol_at_the_end_of_the_longest_stream():
    run_case("stream_limit_error")


# ---- 4: the dense scratch and the component planes past 2^32 --------------------------------------------------------------------------
def test_dense_scratch_past_4_gib():
    run_case("dense_scratch")


def test_libjpeg_planes_and_output_past_4_gib():
    run_case("libjpeg_planes")


# ---- 5: the resample's source past 2^32 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,filt,dtype", [
    ("planar", "bilinear", "u8"), ("planar", "antialias", "u8"), ("planar", "bicubic", "u8"),
    ("rgb8", "bilinear", "u8"), ("rgb8", "antialias", "u8"), ("rgb8", "bicubic", "u8"),
    ("planar", "bilinear", "f16"), ("gray", "bilinear", "u8"),
])
def test_resample_reads_a_source_past_4_gib(fmt, filt, dtype):
    run_case("resample_source", fmt, filt, dtype)


# ---- 6: the resample's destination past 2^32 inside one canvas ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dtype,runs", [
    ("planar", "u8", "bilinear,antialias,bicubic,bilinear:6"),      # the last: orientation 6, the transposed store
    ("rgb8", "u8", "bilinear"),
    ("rgb8", "f16", "bilinear"),
])
def test_resample_and_border_write_a_canvas_past_4_gib(fmt, dtype, runs):
    run_case("canvas", fmt, dtype, runs)


# ---- 7: dst_off past 2^32 across views ----------------------------------------------------------------------------------------------------
def test_views_past_4_gib():
    run_case("view_offsets")
