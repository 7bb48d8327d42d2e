"""CPU: the sample-rate additions of the C ABI exist and follow its contract where no handle or GPU is needed (NULL handle or NULL
pointers: -1, nothing written), and whisper_srv's X-Sample-Rate header parses as documented (csrc/http_request.hpp, exercised as a
stand-alone host program: tests/cpp/http_sample_rate_test.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("AX_WHISPER_ResampledLength", "AX_WHISPER_ResampleFilter", "AX_WHISPER_ResampleBatch", "AX_WHISPER_ComputeMelRate",
       "AX_WHISPER_RunPCMBatchRate", "AX_WHISPER_StreamAdmitBatchRate", "AX_WHISPER_RunFileResampled", "AX_WHISPER_LoadAudioFile16k")


def test_new_symbols_are_declared_exported_and_bound(built_lib):
    header = open(built_lib.HEADER_PATH).read()
    lib = C.CDLL(built_lib.LIB_PATH)
    for n in NEW:
        assert n + "(" in header and hasattr(lib, n) and n in built_lib.SYMBOLS, n


def test_null_handle_and_null_pointers_return_minus_one(built_lib):
    L = built_lib.load_library()
    fp, ip = built_lib.fp, C.POINTER(C.c_int)
    x = np.zeros(16, dtype=np.float32)
    out = np.full(16, 7.0, dtype=np.float32)
    ptr = (fp * 1)(x.ctypes.data_as(fp))
    optr = (fp * 1)(out.ctypes.data_as(fp))
    one = (C.c_int * 1)(16)
    rate = (C.c_int * 1)(8000)
    n = (C.c_int * 1)(-5)
    ids = np.zeros(448, dtype=np.int32)
    text = C.c_void_p(123)
    assert L.AX_WHISPER_ResampleBatch(None, ptr, one, rate, 1, optr, one, n) == -1
    assert L.AX_WHISPER_ComputeMelRate(None, x.ctypes.data_as(fp), 16, 8000, out.ctypes.data_as(fp)) == -1
    assert L.AX_WHISPER_RunPCMBatchRate(None, 0, ptr, one, rate, 1, 4, ids.ctypes.data_as(built_lib.ip), n) == -1
    assert L.AX_WHISPER_StreamAdmitBatchRate(None, one, ptr, one, rate, None, 1) == -1
    assert L.AX_WHISPER_RunFileResampled(None, b"x.wav", C.byref(text)) == -1
    assert L.AX_WHISPER_LoadAudioFile16k(None, b"x.wav", C.byref(text), n, None) == -1
    assert (out == 7.0).all() and n[0] == -5 and not ids.any()
    # host only: NULL outputs
    l = C.c_int()
    assert L.AX_WHISPER_ResampleFilter(48000, None, C.byref(l), C.byref(l), None, 0) == -1
    assert L.AX_WHISPER_ResampleFilter(48000, C.byref(l), C.byref(l), C.byref(l), out.ctypes.data_as(fp), 16) == -1  # cap below L * 2 K
    assert (out == 7.0).all()


def test_x_sample_rate_header(tmp_path):
    exe = tmp_path / "http_sample_rate_test"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "whisper.axera_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "http_sample_rate_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    bad = 'rate=16000 rate_ok=0 error={"error": "X-Sample-Rate must be a positive integer in Hz"}'
    assert got == {"absent": "rate=16000 rate_ok=1 error=-", "8000": "rate=8000 rate_ok=1 error=-", "spaces": "rate=48000 rate_ok=1 error=-",
                   "non-numeric": bad, "zero": bad, "negative": bad, "empty": bad, "long": bad,
                   "other-header": "rate=16000 rate_ok=1 error=-"}
