"""GPU: the resample kernel (csrc/resample.hip) alone, its WHOLE output against float64 under the per-element bound of
tests/resample_reference.py, both builds.

tests/cpp/resample_kernel_driver.cpp is linked against the objects `make` produced for libax_whisper.so (build/resample.*.o), so
what runs here is the shipped code. A case is a list of groups, a group one launch_resample. Every buffer a launch names, inputs
included, comes back whole with its guards: a clip's outputs lie inside the bound (a unit impulse comes back as the table values,
exactly), everything else — guards, output entries at and beyond n_out, other clips' rows, rows nobody owns, the overflow buffer
past the tails, the gaps of the packed layout, the inputs, the tables, the descriptors — holds a NaN sentinel (or its input) before
and the same bits after. tests/test_resample_reference.py shows without a GPU that a float32 emulation passes every clip of CASES
and six seeded defects do not.

Cases (resample_reference.CASES): per rate in 8000, 12000, 24000 (tables in LDS), 48000 (one row, wave-uniform), 44100 and 11025 Hz
(tables through L2) eight launches, one per length n in 1, 2, K, 2 K + 1 and the smallest n with n_out >= kResampleTile - 1,
kResampleTile, kResampleTile + 1, 2 kResampleTile + 1, each over four clips (noise in [-1, 1], a unit impulse, DC 1.0, zeros);
96000 Hz with n_out = kResampleTile + 1 (the widest input span per tile among the tested rates); one launch over 44100 Hz x 1000
samples, 8000 Hz x 1 sample and 48000 Hz x (3 kResampleTile + 1) outputs; staging rows of 8000 samples with two tails in one overflow
buffer, a clip inside its row and a row nobody owns; the packed layout with 64-bit offsets and gaps between three clips.

A driver process has its own timeout; after one that fails, nothing further is launched and the remaining cases fail at once.
Measured on an MI355X (printed by -s and by test_zz_report), worst error / bound, identical in the bf16 and the fp16 build (the kernel does
not depend on the 16-bit type): 8000, 12000 and 11025 Hz 0.366, 48000 Hz 0.286, 44100 Hz 0.267, 24000 Hz 0.257, 96000 Hz 0.021. The file
takes 11 s (30 tests; the one-off driver link aside).
"""
import subprocess
import time

import numpy as np
import pytest

import kernel_driver
import resample_reference as R

pytestmark = pytest.mark.gpu

DTYPES = kernel_driver.DTYPES
_session = kernel_driver.Session()


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, kernel_driver.driver_exe(request.param, "resample_kernel_driver.cpp", ("resample",), ("common.hpp",))


@pytest.mark.parametrize("name", list(R.CASES))
def test_case(driver, tmp_path, name):
    kernel_driver.run_groups(_session, R.verify, R.form_of, R.grid_of, driver, tmp_path, R.CASES[name](driver[0]), timeout=120)


def _short_table():
    return R.launch_group("refused", [(44100, R.family("noise", 1000, 1))], tables_short=1)


def _no_room():
    return R.launch_group("refused", [(48000, R.family("noise", 3000, 1))], out_short=6)


def _no_overflow():
    return R.launch_group("refused", [(48000, R.family("noise", 3 * 8001, 1))], placement="rows", stride=8000, rows=[0], n_rows=1, overflow=False)


REFUSED = {"a table that does not hold L x 2 K entries": _short_table,
           "an output beyond its capacity": _no_room,
           "an output beyond its staging row without an overflow buffer": _no_overflow}


@pytest.mark.parametrize("what", list(REFUSED))
def test_driver_refuses_what_the_launcher_cannot_take(driver, tmp_path, what):
    """Status 2 before anything is launched (the kernel itself trusts its parameters)."""
    bufs, launches = REFUSED[what]()
    lines = []
    for name, content in bufs.items():
        np.ascontiguousarray(content).tofile(tmp_path / name)
        lines.append(f"alloc {name} {np.ascontiguousarray(content).nbytes} {tmp_path / name}")
    cmd, ident, p, _ = launches[0]
    lines.append(f"{cmd} {ident} " + " ".join(f"{k}={v}" for k, v in p.items()))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver[1], str(tmp_path / "manifest.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "ran " not in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-300:])


def test_both_placements_ran(driver):
    dt, _ = driver
    assert R.WANTED_FORMS <= _session.ran[dt], sorted(R.WANTED_FORMS - _session.ran[dt], key=str)


def test_zz_report(driver):
    dt, _ = driver
    for (t, what), w in sorted(_session.worst.items()):
        if t == dt:
            print(f"{dt} {what}: worst error / bound {w:.3f}")
    print(f"wall time so far {time.time() - _session.state['t0']:.0f} s")
