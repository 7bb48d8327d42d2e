"""GPU: the row producers' merge of the cross-attention partial records, inside the gather (co_gather_merge, the one-clip launch)
against the LDS form (merge_cross_records, the multi-clip launch) on the same records — tests/cpp/cross_merge_driver.cpp, one
workgroup with the launch's wave roles, H = 2 and H = 12 heads. The host writes every record complete, with its tag, before the
launch: nothing waits.

Both forms call the one arithmetic on values (merge_cross_values), so the attention vectors must be the same BITS. Against float64:
a = sum_s f_s o_s / sum_s f_s l_s with f_s = exp(m_s - max m). In fp32 every f_s carries the subtraction, the product with log2 e and
v_exp_f32 (u |m_s - m| each for the first two, 2 u), every product and sum u: first order, with the factor 2 for what first
order leaves out, |a - a64| <= 2 sum_s f_s (|o_s| / L + |a| l_s / L) (5 + 2 |m_s - m|) u + 2 u |a|, L = sum f l, u = 2^-24."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper.axera_amd")
BUILD = os.path.join(PKG, "build")
HIPCC = "/opt/rocm/bin/hipcc"
U = 2.0 ** -24
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver_exe():
    """build/cross_merge_driver (the merge is fp32 throughout: one dtype build), rebuilt whenever it is older than its sources."""
    exe = os.path.join(BUILD, "cross_merge_driver")
    srcs = [os.path.join(ROOT, "tests", "cpp", "cross_merge_driver.cpp")] + [os.path.join(PKG, "csrc", f) for f in
                                                                            ("decode_persistent_common.hpp", "common.hpp", "decode_layout.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(f) for f in srcs):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DAXW_F16=0", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                        srcs[0], "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def make_records(H, seed):
    """[H][3][66] float32: o[64], m, l of every (head, key range). Head 0: one range without a valid key (m = -inf, l = 0, o = 0);
    head 1: maxima more than 80 apart (the far ranges' weights underflow towards 0 in fp32); the rest: maxima a few units apart."""
    rng = np.random.default_rng(seed)
    rec = np.empty((H, 3, 66), dtype=np.float32)
    rec[:, :, 64] = rng.normal(0.0, 3.0, (H, 3))
    rec[:, :, 65] = rng.uniform(1.0, 400.0, (H, 3))
    rec[:, :, :64] = rng.standard_normal((H, 3, 64)) * rec[:, :, 65:66] * 0.3
    rec[0, int(rng.integers(3))] = np.concatenate([np.zeros(64), [-np.inf, 0.0]]).astype(np.float32)
    rec[1, :, 64] = np.array([-2.5, 83.0, -40.0], dtype=np.float32)[rng.permutation(3)]
    assert rec[1, :, 64].max() - rec[1, :, 64].min() > 80
    return rec


def expect(rec):
    """float64 attention vector [H * 64] and its bound."""
    r = rec.astype(np.float64)
    m, l, o = r[:, :, 64], r[:, :, 65], r[:, :, :64]
    mx = m.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        f = np.where(np.isfinite(m), np.exp(m - mx), 0.0)
        dm = np.where(np.isfinite(m), mx - m, 0.0)
    L = (f * l).sum(axis=1)[:, None]
    a = (f[:, :, None] * o).sum(axis=1) / L
    w = (f * (5 + 2 * dm))[:, :, None]
    bound = 2 * U * (w * (np.abs(o) / L[:, :, None] + np.abs(a)[:, None, :] * l[:, :, None] / L[:, :, None])).sum(axis=1) + 2 * U * np.abs(a) + 1e-300
    return a.reshape(-1), bound.reshape(-1)


@pytest.mark.parametrize("H", [2, 12])
def test_merge_inside_the_gather_gives_the_lds_form_s_bits(driver_exe, H, tmp_path):
    cases = [make_records(H, 40 + H + i) for i in range(3)]
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for rec in cases:
            f.write(np.int32(H).tobytes())
            f.write(rec.tobytes())
    r = subprocess.run([driver_exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
    got = np.fromfile(fout, dtype=np.float32).reshape(len(cases), 2, H * 64)
    worst = 0.0
    for ci, rec in enumerate(cases):
        new, lds = got[ci]
        same = new.view(np.uint32) == lds.view(np.uint32)
        assert same.all(), f"H {H} case {ci}: the two forms differ at elements {np.nonzero(~same)[0][:8]}: {new[~same][:4]} against {lds[~same][:4]}"
        a, bound = expect(rec)
        assert np.isfinite(new).all()
        ratio = np.abs(new.astype(np.float64) - a) / bound
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1, f"H {H} case {ci}: element {i} {new[i]} against {a[i]}, error {abs(new[i] - a[i]):.3e} = {ratio[i]:.2f} x its bound {bound[i]:.3e}"
        worst = max(worst, float(ratio[i]))
    print(f"H {H}: worst error / bound {worst:.4f}")
