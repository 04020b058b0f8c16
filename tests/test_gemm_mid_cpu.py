"""CPU: llark_gemm16_mid (csrc/gemm_mid.hip) checks every shape rule before any launch, names the offending argument in
llark_last_error, and llark_gemm16_mid_scratch_bytes documents its own size (include/llark_hip.h).  No GPU call is made: the pointers
handed over are host buffers the library never dereferences."""
import ctypes

import pytest

from llark_amd import _lib

BF16, F16 = 1, 0
EPI_F32, EPI_RESID, EPI_QGELU_SPLIT, EPI_SWIGLU16, EPI_SWIGLU_SPLIT = 0, 1, 2, 4, 6
_BUF = ctypes.create_string_buffer(4096 + 64)
PTR = (ctypes.addressof(_BUF) + 63) // 64 * 64          # a 64-byte aligned non-null address (never read)


def _bn(split):
    return 256 if split else 128


def _documented(m, n, kp, split, splits):
    """splits x m x (n rounded up to the column tile) x 4 bytes (include/llark_hip.h)"""
    bn = _bn(split)
    return splits * m * ((n + bn - 1) // bn * bn) * 4


def _call(L, *, dtype=BF16, split=1, epi=EPI_F32, a_hi=PTR, a_lo=PTR, lda=None, wt=PTR, ldw=None, bias=None, m=32, n=256, kp=512, c=PTR,
          ldc=None, resid=PTR, ldr=None, out_hi=PTR, out_lo=PTR, ldo=None, scratch=PTR, scratch_bytes=1 << 40):
    lda = kp if lda is None else lda
    ldw = kp if ldw is None else ldw
    ldc = n if ldc is None else ldc
    ldr = n if ldr is None else ldr
    ldo = n if ldo is None else ldo
    return L.llark_gemm16_mid(dtype, split, epi, a_hi, a_lo, lda, wt, ldw, bias, m, n, kp, c, ldc, resid, ldr, out_hi, out_lo, ldo, scratch,
                              scratch_bytes, None)


def test_scratch_bytes_is_zero_for_refused_shapes_and_at_least_the_documented_size():
    L = _lib.lib()
    for m, n, kp, split, epi in [(0, 256, 512, 1, EPI_F32), (16, 256, 512, 1, EPI_F32), (65, 256, 512, 0, EPI_F32), (32, 256, 40, 1, EPI_F32),
                                 (32, 0, 512, 1, EPI_F32), (32, 256, 0, 1, EPI_F32), (32, 96, 512, 1, EPI_SWIGLU_SPLIT),
                                 (32, 96, 512, 0, EPI_SWIGLU16), (32, 256, 512, 1, EPI_QGELU_SPLIT), (32, 256, 512, 1, 99)]:
        assert L.llark_gemm16_mid_scratch_bytes(m, n, kp, split, epi) == 0, (m, n, kp, split, epi)
    for m in (17, 20, 33, 64):
        for n, kp in [(80, 32), (100, 96), (4096, 4096), (4096, 11008), (12288, 4096), (22016, 4096), (32004, 4096)]:
            for split in (0, 1):
                for epi in (EPI_F32, EPI_RESID) + ((EPI_SWIGLU_SPLIT if split else EPI_SWIGLU16,) if n % 64 == 0 else ()):
                    got = L.llark_gemm16_mid_scratch_bytes(m, n, kp, split, epi)
                    assert got >= _documented(m, n, kp, split, 1) and got % 16 == 0, (m, n, kp, split, epi, got)
                    assert got <= _documented(m, n, kp, split, 8), (m, n, kp, split, epi, got)         # splits is 1 .. 8
                    # the K split -- and with it the summation order of a row -- must not depend on the row count
                    assert got * 17 == L.llark_gemm16_mid_scratch_bytes(17, n, kp, split, epi) * m
    # o_proj / down_proj of a 7B model fill the chip: (n / column tile) x splits is 0.5 .. 1 x 256 workgroups
    for n, kp, split in [(4096, 4096, 0), (4096, 4096, 1), (4096, 11008, 0), (4096, 11008, 1)]:
        splits = L.llark_gemm16_mid_scratch_bytes(64, n, kp, split, EPI_RESID) // _documented(64, n, kp, split, 1)
        assert 128 <= (n // _bn(split)) * splits <= 256, (n, kp, split, splits)


@pytest.mark.parametrize("kwargs,code,names", [
    (dict(m=0), -2, b"m=0"),
    (dict(m=16), -2, b"m=16"),
    (dict(m=65), -2, b"m=65"),
    (dict(kp=40), -1, b"kp=40"),
    (dict(a_hi=None), -1, b"a_hi"),
    (dict(a_lo=None), -1, b"a_lo"),
    (dict(wt=None), -1, b"wt"),
    (dict(epi=EPI_SWIGLU_SPLIT, n=96), -1, b"n=96"),
    (dict(epi=EPI_SWIGLU16, split=0, n=160), -1, b"n=160"),
    (dict(epi=EPI_SWIGLU_SPLIT, n=128, out_lo=None), -1, b"out_lo"),
    (dict(scratch_bytes=1024), -1, b"scratch_bytes=1024"),
    (dict(scratch=None), -1, b"scratch"),
    (dict(epi=99), -1, b"epilogue=99"),
    (dict(epi=EPI_QGELU_SPLIT), -1, b"epilogue=2"),
    (dict(dtype=F16), -2, b"dtype=0"),
    (dict(lda=504), -1, b"lda=504"),
    (dict(ldw=516), -1, b"ldw=516"),
    (dict(c=None), -1, b"c is null"),
    (dict(ldc=255), -1, b"ldc=255"),
    (dict(epi=EPI_RESID, resid=None), -1, b"resid"),
    (dict(a_hi=PTR + 2), -1, b"aligned"),
])
def test_bad_arguments_are_refused_before_any_launch_and_named(kwargs, code, names):
    L = _lib.lib()
    assert _call(L, **kwargs) == code, kwargs
    msg = L.llark_last_error()
    assert msg.startswith(b"gemm16_mid: ") and names in msg, (kwargs, msg)


def test_scratch_one_byte_short_is_refused():
    L = _lib.lib()
    need = L.llark_gemm16_mid_scratch_bytes(32, 256, 512, 1, EPI_F32)
    assert need > 0
    assert _call(L, scratch_bytes=need - 1) == -1
    assert b"scratch_bytes" in L.llark_last_error()
