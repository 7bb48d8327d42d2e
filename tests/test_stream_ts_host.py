"""CPU: the slot stream's timestamp-mode additions (DESIGN.md "Slot stream in timestamp mode") where no GPU is needed: the C ABI's new
symbols exist and follow its contract on a NULL handle or NULL pointers (-1, nothing written); whisper_srv's X-Timestamps, X-Language
and X-Task headers parse as documented (csrc/http_request.hpp, exercised by a stand-alone host program under AddressSanitizer and
UBSan: tests/cpp/http_request_fields_test.cpp); the two new kernels and the new advance instantiation compile for gfx950 in both
builds without scratch memory or register spills, within the registers and LDS DESIGN.md states for them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.axera_amd", "csrc")

NEW = ("AX_WHISPER_StreamOpenMode", "AX_WHISPER_StreamAdmitBatchLang", "AX_WHISPER_StreamCollectScored", "AX_WHISPER_StreamRulesStage")


@pytest.fixture(scope="module")
def L(built_lib):
    return built_lib.load_library()


def test_exports_exist_and_are_declared(L, built_lib):
    header = open(os.path.join(ROOT, "include", "ax_whisper_api.h")).read()
    for name in NEW:
        assert getattr(L, name) is not None and name in built_lib.SYMBOLS
        assert re.search(r"AX_WHISPER_API int %s\(" % name, header), name


def test_null_arguments_return_minus_one_and_write_nothing(L):
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert L.AX_WHISPER_StreamOpenMode(None, 4, 1) == -1 and L.AX_WHISPER_StreamOpenMode(None, 4, 0) == -1
    pcm = np.zeros(16, dtype=np.float32)
    ptrs = (fp * 1)(pcm.ctypes.data_as(fp))
    one, n16, zero = (C.c_int * 1)(0), (C.c_int * 1)(16), (C.c_int * 1)(0)
    assert L.AX_WHISPER_StreamAdmitBatchLang(None, one, ptrs, n16, None, None, zero, zero, 1) == -1
    fake = C.c_void_p(1)  # never dereferenced: the pointer checks come first
    assert L.AX_WHISPER_StreamAdmitBatchLang(fake, None, ptrs, n16, None, None, zero, zero, 1) == -1
    assert L.AX_WHISPER_StreamAdmitBatchLang(fake, one, None, n16, None, None, zero, zero, 1) == -1
    assert L.AX_WHISPER_StreamAdmitBatchLang(fake, one, ptrs, None, None, None, zero, zero, 1) == -1
    assert L.AX_WHISPER_StreamAdmitBatchLang(fake, one, ptrs, n16, None, None, zero, zero, 0) == -1
    assert L.AX_WHISPER_StreamAdmitBatchLang(fake, one, (fp * 1)(), n16, None, None, zero, zero, 1) == -1  # a NULL clip
    ids = np.full(8, 7, dtype=np.int32)
    f = np.full(8, 7.0, dtype=np.float32)
    n = C.c_int(7)
    i32 = C.POINTER(C.c_int32)
    assert L.AX_WHISPER_StreamCollectScored(None, 0, ids.ctypes.data_as(i32), C.byref(n), f.ctypes.data_as(fp), None, None, None, None, None) == -1
    assert L.AX_WHISPER_StreamCollectScored(fake, 0, None, C.byref(n), None, None, None, None, None, None) == -1
    assert L.AX_WHISPER_StreamCollectScored(fake, 0, ids.ctypes.data_as(i32), None, None, None, None, None, None, None) == -1
    assert (ids == 7).all() and (f == 7.0).all() and n.value == 7
    rows = np.zeros(8, dtype=np.float32)
    ctx = np.full(4, 7, dtype=np.int32)
    args = [rows.ctypes.data_as(fp), one, one, one, ids.ctypes.data_as(i32), one, ctx.ctypes.data_as(ip), ids.ctypes.data_as(i32),
            f.ctypes.data_as(fp), f.ctypes.data_as(fp), ctx.ctypes.data_as(ip), f.ctypes.data_as(fp)]
    assert L.AX_WHISPER_StreamRulesStage(None, 1, *args) == -1
    assert L.AX_WHISPER_StreamRulesStage(fake, 0, *args) == -1
    for k in range(len(args)):
        assert L.AX_WHISPER_StreamRulesStage(fake, 1, *[None if j == k else a for j, a in enumerate(args)]) == -1, k
    assert (ids == 7).all() and (f == 7.0).all() and (ctx == 7).all()


def test_request_field_headers_under_sanitizers(tmp_path):
    exe = tmp_path / "http_request_fields_test"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(ROOT, "tests", "cpp", "http_request_fields_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    need = '{"error": "X-Timestamps, X-Language and X-Task need a server started with --timestamps"}'
    bad_ts = 'ts=-1 lang=- task=-1 plain={0} slots={0}'.format('{"error": "X-Timestamps must be 0 or 1"}')
    bad_lang = 'ts=-1 lang=- task=-1 plain={0} slots={0}'.format('{"error": "X-Language must be a language code or auto"}')
    bad_task = 'ts=-1 lang=- task=-1 plain={0} slots={0}'.format('{"error": "X-Task must be transcribe or translate"}')
    none = "ts=-1 lang=- task=-1 plain=- slots=-"
    assert got == {"absent": none, "all": f"ts=1 lang=en task=1 plain={need} slots=-",
                   "case-and-blanks": f"ts=0 lang=auto task=0 plain={need} slots=-", "other-headers": none,
                   "language-only": f"ts=-1 lang=yue task=-1 plain={need} slots=-",
                   "ts-2": bad_ts, "ts-empty": bad_ts, "ts-word": bad_ts, "ts-signed": bad_ts,
                   "lang-empty": bad_lang, "lang-digits": bad_lang, "lang-long": bad_lang, "lang-two": bad_lang,
                   "task-empty": bad_task, "task-other": bad_task, "task-prefix": bad_task}


#            VGPRs, SGPRs (steps of 8, a little above what the build takes), LDS bytes (exact)
CEILINGS = {"stream_rules_kernel": (40, 80, 688), "advance_kernelINS0_13AdvanceParams": (64, 88, 0), "slot_reset_ts_kernel": (16, 56, 0)}
FILES = {"stream_rules_kernel": "decode_timestamps.hip", "advance_kernelINS0_13AdvanceParams": "decode_gemv.hip", "slot_reset_ts_kernel": "engine_stream.cpp"}


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kernel", sorted(CEILINGS))
def test_new_kernels_no_scratch_no_spills(kernel, f16, tmp_path):
    """Reads the compiler's resource report only."""
    out = tmp_path / "k.s"
    src = os.path.join(CSRC, FILES[kernel])
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        f"-DAXW_F16={f16}", "--cuda-device-only", "-S", "-x", "hip", "-o", str(out), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, re.M)
    field = lambda k: [int(x) for x in re.findall(r"^\s+\." + k + r":\s+(\d+)", text, re.M)]
    hits = [i for i, n in enumerate(names) if kernel in n]
    assert len(hits) == 1, (kernel, names)
    i = hits[0]
    assert len(field("private_segment_fixed_size")) == len(names)
    assert field("private_segment_fixed_size")[i] == 0 and field("vgpr_spill_count")[i] == 0 and field("sgpr_spill_count")[i] == 0
    vg, sg, lds = CEILINGS[kernel]
    got = (field("vgpr_count")[i], field("sgpr_count")[i], field("group_segment_fixed_size")[i])
    assert got[0] <= vg and got[1] <= sg and got[2] == lds, (kernel, got)
    if kernel.startswith("advance"):  # the instantiation every other call runs is still there, beside the new one
        assert sum("advance_kernelINS0_11AdvanceArgs" in n for n in names) == 1
