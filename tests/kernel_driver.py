"""The process side of the stand-alone kernel tests (tests/test_gpu_decode_kernels.py, tests/test_gpu_gemv_kernels.py,
tests/test_gpu_frontend_kernels.py): building a driver of tests/cpp/ against the shipped objects, and running one driver process over a
list of groups."""
import os
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper.axera_amd")
BUILD = os.path.join(PKG, "build")
HIPCC = "/opt/rocm/bin/hipcc"
DTYPES = ("bf16", "f16")
LINKED = ("decode_gemm", "decoder", "decode_gemv")  # the kernel files whose objects the driver links


class Session:
    """What one test file keeps between its tests: whether a driver run failed, the forms that ran and the worst ratios, per build."""

    def __init__(self):
        self.state = {"dead": None, "t0": time.time()}
        self.ran = {dt: set() for dt in DTYPES}
        self.worst = {}


def driver_exe(dt, source="decode_kernels_driver.cpp", linked=LINKED, also=("common.hpp", "decode_layout.hpp")):
    """build/<source's name>.<dt> from tests/cpp/<source>, relinked whenever it is older than its source or the objects it links
    (build/<k>.<dt>.o for k in linked; `also`: further files of csrc/ the kernels are made of)."""
    exe = os.path.join(BUILD, os.path.splitext(source)[0] + "." + dt)
    src = os.path.join(ROOT, "tests", "cpp", source)
    objs = [os.path.join(BUILD, f"{k}.{dt}.o") for k in linked]
    srcs = [src] + [os.path.join(PKG, "csrc", f) for f in [k + ".hip" for k in linked] + list(also)]
    newest = max(os.path.getmtime(f) for f in srcs + [o for o in objs if os.path.exists(o)])
    if os.path.exists(exe) and os.path.getmtime(exe) >= newest:
        return exe
    r = subprocess.run(["make", "-C", PKG, "-j16"] + [os.path.relpath(o, PKG) for o in objs], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    obj = exe + ".o"
    for cmd in ([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DAXW_F16=" + ("1" if dt == "f16" else "0"),
                 "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-c", src, "-o", obj],
                [HIPCC, "--offload-arch=gfx950", obj] + objs + ["-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_groups(session, verify, form_of, grid_of, driver, tmp_path, groups, timeout=120, qall=None, keep=None):
    """One driver process for all groups; every launch checked (verify) against what its predecessors left. A group is
    (bufs, launches), a launch (cmd, id, keys, buffers to dump). Returns the notes {label: worst error / bound}."""
    dt, exe = driver
    if session.state["dead"]:
        pytest.fail("not run: an earlier driver run failed (" + session.state["dead"] + ")")
    tmp = str(tmp_path)
    lines, n = [], 0
    for gi, (bufs, launches) in enumerate(groups):
        for name, content in bufs.items():
            n += 1
            f = os.path.join(tmp, f"in{n}.bin")
            np.ascontiguousarray(content).tofile(f)
            lines.append(f"alloc {name} {np.ascontiguousarray(content).nbytes} {f}")
        for li, (cmd, ident, p, outs) in enumerate(launches):
            lines.append(f"{cmd} {ident} " + " ".join(f"{k}={v}" for k, v in p.items()))
            lines += [f"dump {o} {os.path.join(tmp, f'g{gi}.l{li}.{o}')}" for o in outs]
        lines += [f"free {name}" for name in bufs]
    mf = os.path.join(tmp, "manifest.txt")
    with open(mf, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ)
    env.pop("AX_WHISPER_ATTN_QALL", None)
    if qall is not None:
        env["AX_WHISPER_ATTN_QALL"] = qall
    try:
        r = subprocess.run([exe, mf], capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        session.state["dead"] = "timeout"
        raise
    if r.returncode != 0 or not r.stdout.rstrip().endswith("done"):
        session.state["dead"] = f"exit status {r.returncode}"
        pytest.fail(f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    grids = {ln.split()[1]: tuple(int(v) for v in ln.split()[2:5]) for ln in r.stdout.splitlines() if ln.startswith("ran ")}

    def dumps(gi, li, outs):
        got = {}
        for o in outs:
            f = os.path.join(tmp, f"g{gi}.l{li}.{o}")
            got[o] = np.fromfile(f, dtype=np.uint16)
            os.remove(f)
        return got

    return check_groups(session, verify, form_of, grid_of, dt, groups, lambda gi, li, l, state: (grids[l[1]], dumps(gi, li, l[3])), qall=qall, keep=keep)


def check_groups(session, verify, form_of, grid_of, dt, groups, result_of, qall=None, keep=None):
    """The checking half of run_groups: result_of(group index, launch index, launch, state) gives (grid, dumps) of a launch."""
    from decode_kernel_reference import strip

    notes = {}
    for gi, (bufs, launches) in enumerate(groups):
        state, prev = dict(bufs), None
        for li, l in enumerate(launches):
            cmd, ident, p, outs = l
            grid, got = result_of(gi, li, l, state)
            assert grid == grid_of(cmd, p), (ident, grid)
            for what, w in verify(cmd, ident, p, state, got, dt, prev).items():
                notes[what] = max(notes.get(what, 0.0), w)
                session.worst[dt, what] = max(session.worst.get((dt, what), 0.0), w)
            session.ran[dt].add(form_of(cmd, p, qall))
            if keep is not None:
                keep[ident] = got
            prev = got
            for o in outs:
                state[o] = strip(ident, got[o])
    for what, w in sorted(notes.items()):
        print(f"{dt} {what}: worst error / bound {w:.4f}")
    return notes
