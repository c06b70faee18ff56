"""CPU: the checked inflate call (hdlz_inflate_checked) is exported, names its two statuses, checks its parameters before it looks
for a device, and asks for almost no scratch of its own."""
import ctypes

import pytest

E_BAD_PARAM, E_HIP = 8, 9
FLAGS_OK = (0, 1, 2, 4, 64, 128, 1 | 2, 1 | 128)


def _lib():
    from hdl_deflate_amd import _lib
    return _lib.load()


def test_symbols_status_strings_and_constants():
    import hdl_deflate_amd
    from hdl_deflate_amd import _lib, constants
    L = _lib.load()
    assert hasattr(L, "hdlz_inflate_checked") and hasattr(L, "hdlz_inflate_checked_work_bytes")
    assert "hdlz_inflate_checked" in _lib.EXPORTS and "hdlz_inflate_checked_work_bytes" in _lib.EXPORTS
    assert L.hdlz_status_string(11) == b"BAD_HEADER" and L.hdlz_status_string(12) == b"BAD_CHECKSUM"
    assert hdl_deflate_amd.E_BAD_HEADER == constants.E_BAD_HEADER == 11
    assert hdl_deflate_amd.E_BAD_CHECKSUM == constants.E_BAD_CHECKSUM == 12
    assert constants.STATUS_NAMES[11] == "BAD_HEADER" and constants.STATUS_NAMES[12] == "BAD_CHECKSUM"
    assert L.hdlz_version() == 0x000600          # the call is additive: the new symbols are the feature test


def test_parameter_errors_come_before_the_device():
    L = _lib()
    buf = (ctypes.c_uint8 * 256)()

    def call(flags=0, in_used=buf, adler=buf, work=None, work_bytes=0, nstreams=1, out_pitch=64):
        return L.hdlz_inflate_checked(buf, None, 64, 64, nstreams, flags, 0, buf, out_pitch, buf, buf, in_used, adler,
                                      work, work_bytes, None)
    assert call(in_used=None) == E_BAD_PARAM and b"d_in_used" in L.hdlz_last_error()
    assert call(flags=8) == E_BAD_PARAM and b"ONEBLOCK" in L.hdlz_last_error()
    for f in (16, 32, 256, 1 << 31):
        assert call(flags=f) == E_BAD_PARAM, f
    assert call(flags=2 | 4) == E_BAD_PARAM                                  # contradictory hints, as in hdlz_inflate_batch_ws
    assert call(out_pitch=66) == E_BAD_PARAM
    # the judging pass's own share of the scratch (rows of 64 KiB and more): required
    share = L.hdlz_inflate_checked_work_bytes(4, 64, 1 << 20, 2, 0) - L.hdlz_inflate_work_bytes(4, 64, 1 << 20, 2, 0)
    assert share > 0
    assert call(flags=2, nstreams=4, out_pitch=1 << 20) == E_BAD_PARAM and b"share" in L.hdlz_last_error()
    assert call(flags=2, nstreams=4, out_pitch=1 << 20, work=buf, work_bytes=share - 1) == E_BAD_PARAM
    import torch
    if torch.cuda.is_available():
        return                       # (with a device the good calls below would run kernels on these host buffers)
    for f in FLAGS_OK:
        assert call(flags=f) == E_HIP, f
    assert call(adler=None) == E_HIP                                          # d_adler is optional
    assert call(nstreams=0, in_used=buf) == E_HIP


SHAPES = [(1 << 20, 0, 2048, 0, 1), (1, 1 << 24, 1 << 26, 0, 0), (1, 1 << 24, 1 << 26, 2, 0), (4096, 1 << 20, 1 << 22, 0, 0),
          (1 << 20, 2048, 2048, 0, 0)]


@pytest.mark.parametrize("shape", SHAPES)
def test_scratch_query(shape):
    L = _lib()
    nstreams, in_len, out_pitch, flags, ragged = shape
    checked = L.hdlz_inflate_checked_work_bytes(*shape)
    plain = L.hdlz_inflate_work_bytes(*shape)
    assert checked >= plain
    # per-tile partial sums, not per-byte anything: at most a tenth of a percent of the output capacity
    assert checked - plain <= nstreams * out_pitch // 1024 + 4096
    assert (checked - plain) % 256 == 0                                       # what is left for the decode stays 256-byte aligned
    if out_pitch < 65536:
        assert checked == plain                                               # short rows need no scratch at all


def test_scratch_query_of_nothing():
    L = _lib()
    assert L.hdlz_inflate_checked_work_bytes(0, 0, 0, 0, 0) == 0
    assert L.hdlz_inflate_checked_work_bytes(0, 1 << 20, 1 << 22, 0, 0) == 0
