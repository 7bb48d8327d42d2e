"""GPU: the log-mel front-end kernels (stft_mel_kernel, stft_mel_long_kernel: csrc/frontend_stft.inc; mel_normalize_kernel,
mel_window_kernel, mel_to_tm_kernel, gmax_reset_kernel: csrc/frontend.hip) alone, their WHOLE output against float64, both builds,
80 and 128 mels.

tests/cpp/frontend_kernels_driver.cpp is linked against the objects `make` produced for libax_whisper.so (build/frontend.*.o), so
what runs here is the shipped code. A case is a list of groups, a group one launch_frontend / launch_frontend_long /
launch_mel_window / launch_mel_to_tm (or two on the same buffers) with 3004-row slots as the engine has them; the Hann window, the
twiddle table and the transposed filterbank are the test's own (the engine's stay covered end to end). Every buffer a launch
names, inputs included, comes back whole with its guards: logmel / store rows are compared with the float64 reference inside the
interval derived per element, gmax, mel_ref and the time-major h16 rows bit for bit from the dumped logmel (tests/
frontend_kernel_reference.py); everything else — logmel rows of frames past a clip's end, row 0 and rows 3001..3003 of every slot,
slots and windows beyond the batch, store rows no file owns, the inputs — holds a NaN sentinel (or its input) before and the same
bits after. tests/test_frontend_kernel_reference.py shows without a GPU that float32 emulations pass every case of CASES and
eighteen seeded defects do not.

Cases (frontend_kernel_reference.CASES): one clip per launch at 1, 159, 160, 200, 201, 401, 5119 / 5120 (a second workgroup with
one frame), 10279 / 10280 (workgroup 1 on the reflecting / on the interior path) and 10441 samples (every input family); the
staging-row edge at stride 8000 with two tails in one overflow buffer; a ragged batch (401, 10441, 5120; loud, 1e-3, silent) and a
second launch on its buffers; 3000, 3001 and 3034 frames; openai mode; a filterbank without zero weights; three files through the
long kernel, bit-equal to the clip kernel; the window kernel over files of 100, 3000 and 3137 rows; mel_to_tm on rounding ties.

A driver process has its own timeout; after one that fails, nothing further is launched and the remaining cases fail at once.

Measured on an MI355X (printed by -s and by test_zz_report), worst error / bound, identical in the bf16 and the fp16 build (the STFT
does not depend on the 16-bit type), 80 | 128 mels:
  logmel   sparse 0.346 | 0.353, sparse398 0.307 | 0.331, tone 0.182 | 0.182, dc 0.182 | 0.182, zeros 0.182 | 0.182 (floor elements: log10f
           is one ulp from -10 there), speech 0.031 | 0.033, noise 0.008 | 0.009, mixed batches 0.325 | 0.353
           openai: sparse 0.343 | 0.360, speech (128 mels) 0.182
  store    (long kernel) 0.325 | 0.353, bit-equal to the clip kernel's logmel
  gmax     beyond 3000 frames 0.230 | 0.040 of the float64 maximum's interval; exact everywhere else
  mel_normalize_kernel, mel_window_kernel, mel_to_tm_kernel: every output bit-equal
  log10f   worst |logmel - log10 M| = 2.763 ulp over the elements with e_M / M < 2^-20 (frontend_kernel_reference.LOG10F_MEASURED; the
           bound takes 5.526 ulp)
The file takes 24 s (60 tests, 11 s per build; the one-off driver link aside). Not measured: another ROCm release's log10f.
"""
import subprocess
import time

import numpy as np
import pytest

import frontend_kernel_reference as R
import kernel_driver

pytestmark = pytest.mark.gpu

DTYPES = kernel_driver.DTYPES
_session = kernel_driver.Session()


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, kernel_driver.driver_exe(request.param, "frontend_kernels_driver.cpp", ("frontend",), ("common.hpp", "frontend_stft.inc"))


@pytest.mark.parametrize("name", list(R.CASES))
def test_case(driver, tmp_path, name):
    kernel_driver.run_groups(_session, R.verify, R.form_of, R.grid_of, driver, tmp_path, R.CASES[name](driver[0]), timeout=120)


REFUSED = {"a clip beyond its staging row without an overflow buffer": lambda g: g[1][0][2].update(stride=5000),
           "a clip without samples": lambda g: g[0].update(ns=np.zeros(1, dtype=np.int32)),
           "a logmel buffer below batch x 3000 x n_mels": lambda g: g[0].update(logmel=R.sentinel(2999 * 80, 4))}


@pytest.mark.parametrize("what", list(REFUSED))
def test_driver_refuses_what_a_launcher_cannot_take(driver, tmp_path, what):
    """Status 2 before anything is launched (the kernels themselves trust their parameters)."""
    group = R.clip_group(driver[0], "refused", 80, [R.family("noise", 5120, 1)], ref=False, tm=False)
    REFUSED[what](group)
    lines = []
    for name, content in group[0].items():
        np.ascontiguousarray(content).tofile(tmp_path / name)
        lines.append(f"alloc {name} {np.ascontiguousarray(content).nbytes} {tmp_path / name}")
    cmd, ident, p, _ = group[1][0]
    lines.append(f"{cmd} {ident} " + " ".join(f"{k}={v}" for k, v in p.items()))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver[1], str(tmp_path / "manifest.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "ran " not in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-300:])


def test_every_front_end_launcher_ran_every_form(driver):
    dt, _ = driver
    assert R.WANTED_FORMS <= _session.ran[dt], sorted(R.WANTED_FORMS - _session.ran[dt], key=str)


def test_zz_report(driver):
    dt, _ = driver
    for (t, what), w in sorted(_session.worst.items()):
        if t == dt:
            print(f"{dt} {what}: worst error / bound {w:.3f}")
    print(f"log10f against float64 where e_M / M < 2^-20: worst {R.log10f_seen['ulps']:.3f} ulp (the bound takes {R.LOG10F_ULPS} ulp)")
    print(f"wall time so far {time.time() - _session.state['t0']:.0f} s")
