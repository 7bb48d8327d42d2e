"""No GPU: float32 emulations of the front-end kernels pass every case of tests/test_gpu_frontend_kernels.py under the bounds of
tests/frontend_kernel_reference.py, and eighteen seeded defects fail at the case named beside them.

The emulations follow the kernels' text (frontend.hip, frontend_stft.inc): the staging loop with its interior and its reflecting
path per workgroup of 32 frames, the DFT in the kernel's k order, two samples per step, the mel product with the bins in pairs, a
correctly rounded log10, the ordered-int maximum per clip, the normalisation, the window kernel's groups of eight values with the
running (f, c) index of its LDS tile. What a real MFMA does inside one step is not known here; the bound holds for any order.

Defects whose effect needs explaining:
  bin201      the padded bin 201 holds its finite DFT power instead of zero. Under the kernel's zero WEIGHT for k >= 201 a finite
              value there is harmless (0 * finite), so the defect is seeded together with the weight of bin 200 for it (`k <= kBins`).
  bin200, bin201   need a filterbank with a weight on bin 200; the Slaney ones end at 8000 Hz = bin 200 (weights 0 and 2e-8), hence
              the `dense basis` case.
  filter_m1   the columns of the last, partly filled wave (mels 64..79 of 80) read filter min(m + 1, n_mels - 1).
"""
import numpy as np
import pytest

import frontend_kernel_reference as R
import kernel_driver
from encoder_kernel_reference import GUARD, SENT16, to_bits

N_FFT, HOP, BINS, FRAMES_OUT, MEL_ROWS = R.N_FFT, R.HOP, R.BINS, R.FRAMES_OUT, R.MEL_ROWS


def with_guards(a):
    g = np.full(GUARD // 2, SENT16, dtype=np.uint16)
    return np.concatenate([g, R.tv(a, np.uint16), g])


# ------------------------------------------------------------------------------------------ stft_mel_kernel / stft_mel_long_kernel
def stage(flat, base, n, n_real, n_frames, limit, win, defect, stride=None, overflow=None, oo=0):
    """The windowed frames [n_frames][400] float32 as the staging loop leaves them. flat[base + j]: the staging row / the file."""
    f = np.arange(n_frames)
    f0 = f // R.FR * R.FR
    j_first, j_last = f0 * HOP - N_FFT // 2, (f0 + R.FR - 1) * HOP + N_FFT - 1 - N_FFT // 2
    fast = (j_first >= 0) & ((j_last <= limit) if defect == "fast_at_n" else (j_last < limit)) & (f0 + R.FR <= n_frames)
    raw = f[:, None] * HOP + np.arange(N_FFT)[None, :] - N_FFT // 2
    j = np.where(raw < 0, -raw - (1 if defect == "left_reflect" else 0), raw)
    j = np.where(j >= n, 2 * n - (1 if defect == "right_reflect" else 2) - j, j)
    j = np.clip(j, 0, n - 1)
    x = np.zeros(raw.shape, dtype=np.float32)
    inside = j < n_real
    if stride is None:
        x[inside] = flat[base + j[inside]]
    else:
        row = inside & (j < stride)
        x[row] = flat[base + j[row]]
        tail = inside & (j >= stride)
        if tail.any():
            x[tail] = overflow[oo + j[tail] - stride + (1 if defect == "overflow_plus1" else 0)]
    x[fast] = flat[base + raw[fast]]
    return x * win[None, :]


_dft_cache = {}


def dft_power(v, tw, defect):
    """[F][202] float32 power: the accumulation order of the kernel's loop, two samples (one MFMA) per step."""
    key = (hash(v.tobytes()), v.shape, defect if defect in ("drop_last_k", "bin201") else None)
    if key in _dft_cache:
        return _dft_cache[key]
    nb = BINS + 1
    idx = (np.arange(N_FFT)[:, None] * np.arange(nb)[None, :]) % N_FFT
    c, s = tw.reshape(N_FFT, 2)[idx, 0], tw.reshape(N_FFT, 2)[idx, 1]
    re, im = np.zeros((v.shape[0], nb), dtype=np.float32), np.zeros((v.shape[0], nb), dtype=np.float32)
    for s2 in range(N_FFT // 2 - (1 if defect == "drop_last_k" else 0)):
        a0, a1 = v[:, 2 * s2, None], v[:, 2 * s2 + 1, None]
        re += a0 * c[2 * s2] + a1 * c[2 * s2 + 1]
        im += a0 * s[2 * s2] + a1 * s[2 * s2 + 1]
    pw = re * re + im * im
    if defect != "bin201":
        pw[:, BINS] = 0.0
    if len(_dft_cache) > 40:
        _dft_cache.clear()
    _dft_cache[key] = pw
    return pw


def logmel32(pw, basis_t, nm, defect):
    bt = basis_t.reshape(BINS, nm)
    if defect == "filter_m1" and nm % 32:
        m = np.arange(nm)
        bt = bt[:, np.where(m >= nm // 32 * 32, np.minimum(m + 1, nm - 1), m)]
    acc = np.zeros((pw.shape[0], nm), dtype=np.float32)
    zero = np.zeros(nm, dtype=np.float32)
    for s2 in range((BINS + 1) // 2 - (1 if defect == "bin200" else 0)):
        k1 = 2 * s2 + 1
        b1 = bt[k1] if k1 < BINS else (bt[BINS - 1] if defect == "bin201" else zero)
        acc += pw[:, 2 * s2, None] * bt[2 * s2] + pw[:, k1, None] * b1
    return np.log10(np.maximum(acc, np.float32(1e-10)).astype(np.float64)).astype(np.float32)


def code_of(v, defect):
    if defect == "ordered_neg":  # the sign bit flipped for both signs: among negatives the most negative wins
        return int(np.float32(v).view(np.uint32)) ^ 0x80000000
    return R.ordered(v)


def emulate_frontend(p, st, dt, defect):
    nm, B, stride, openai = p["n_mels"], p["batch"], p["stride"], bool(p.get("openai"))
    tw, win, bt = st[p["twiddle"]], st[p["window"]], st[p["basis"]]
    logmel = st[p["logmel"]].copy().reshape(-1, FRAMES_OUT, nm)
    gmax = st[p["gmax"]].copy()
    if defect != "no_reset":
        gmax[:B] = 0
    out_ref = st[p["mel_ref"]].copy().reshape(-1, nm, FRAMES_OUT) if p.get("mel_ref") else None
    out_tm = st[p["mel_tm"]].copy().reshape(-1, MEL_ROWS, nm) if p.get("mel_tm") else None
    rows = []
    for b in range(B):
        n_real = int(st[p["n_samples"]][b])
        n = FRAMES_OUT * HOP if openai else n_real
        n_frames = R.n_frames_of(n_real, openai)
        oo = int(st[p["over_off"]][0 if defect == "over_off0" else b]) if p.get("over_off") else 0
        v = stage(st[p["pcm"]], b * stride, n, n_real, n_frames, min(n_real, stride), win, defect, stride, st.get(p.get("overflow")), oo)
        lm = logmel32(dft_power(v, tw, defect), bt, nm, defect)
        nf = min(n_frames, FRAMES_OUT)
        logmel[b, :nf] = lm[:nf]
        top = (lm[:nf] if defect == "gmax_first3000" else lm).max()
        gmax[b] = max(int(gmax[b]), code_of(top, defect))
        rows.append((lm[:nf], nf))
    if defect == "gmax_batch":
        gmax[:B] = gmax[:B].max()
    for b, (lm, nf) in enumerate(rows):
        r = np.zeros((FRAMES_OUT, nm), dtype=np.float32)
        r[:nf] = R.normalise(lm, R.unordered(gmax[b]))
        keep = FRAMES_OUT if defect != "stale_rows" else nf
        if out_ref is not None:
            out_ref[b, :, :keep] = r[:keep].T
        if out_tm is not None:
            at = 0 if defect == "tm_row_f" else 1
            out_tm[b, at: at + keep] = to_bits(r[:keep], dt).reshape(keep, nm)
    return {p["logmel"]: logmel, p["gmax"]: gmax, p.get("mel_ref"): out_ref, p.get("mel_tm"): out_tm}


def emulate_frontend_long(p, st, dt, defect):
    nm, B = p["n_mels"], p["batch"]
    store = st[p["store"]].copy().reshape(-1, nm)
    gmax = st[p["gmax"]].copy()
    gmax[:B] = 0
    for b in range(B):
        n = int(st[p["n_samples"]][b])
        v = stage(st[p["pcm"]], int(st[p["pcm_off"]][b]), n, n, 1 + n // HOP, n, st[p["window"]], defect)
        lm = logmel32(dft_power(v, st[p["twiddle"]], defect), st[p["basis"]], nm, defect)
        fo = int(st[p["frame_off"]][b])
        store[fo: fo + lm.shape[0]] = lm
        gmax[b] = code_of(lm.max(), defect)
    return {p["store"]: store, p["gmax"]: gmax}


# ------------------------------------------------------------------------------------------ mel_window_kernel, mel_to_tm_kernel
def emulate_window(p, st, dt, defect):
    nm, W = p["n_mels"], p["n_windows"]
    store = st[p["store"]]
    out_tm = st[p["mel_tm"]].copy() if p.get("mel_tm") else None
    out_ref = st[p["mel_ref"]].copy() if p.get("mel_ref") else None
    cols, ld = nm // 8, nm + 1
    df, e8 = 256 // cols, np.arange(8)
    dc = 256 - df * cols
    for a in range(W):
        file, seek = int(st[p["win_file"]][a]), int(st[p["win_seek"]][a])
        floor_g = R.unordered(st[p["gmax"]][file])
        for f0 in range(0, FRAMES_OUT, R.WF):
            nf = R.WF if defect == "window_64" else min(R.WF, FRAMES_OUT - f0)
            nv = nf if defect == "window_next_file" else min(max(int(st[p["n_frames"]][file]) - seek - f0, 0), nf)
            src = (int(st[p["frame_off"]][file]) + seek + f0) * nm
            g = np.arange(nf * cols)
            vals = np.zeros((g.size, 8), dtype=np.float32)
            at = src + g[: nv * cols, None] * 8 + e8
            raw = np.where(at < store.size, store[np.minimum(at, store.size - 1)], np.float32(0.123))  # beyond the store: anything
            vals[: nv * cols] = R.normalise(raw, floor_g)
            if out_tm is not None:
                to = ((a * MEL_ROWS + 1 + f0) * nm + g[:, None] * 8 + e8).ravel()
                ok = to < out_tm.size
                out_tm[to[ok]] = to_bits(vals, dt).ravel()[ok]
            if out_ref is not None:
                tile = np.full(4 * R.WF * ld, np.nan, dtype=np.float32)  # LDS nobody wrote: anything
                tid, t = g % 256, g // 256
                if defect == "tile_no_carry":
                    f, c = tid // cols + t * df, tid % cols + t * dc
                else:
                    f, c = g // cols, g % cols
                tile[(f[:, None] * ld + c[:, None] * 8 + e8).ravel()] = vals.ravel()
                fr = np.arange(nf)
                to = ((a * nm + np.arange(nm)[None, :]) * FRAMES_OUT + f0 + fr[:, None]).ravel()
                ok = to < out_ref.size
                out_ref[to[ok]] = tile[(fr[:, None] * ld + np.arange(nm)[None, :]).ravel()][ok]
    return {p.get("mel_tm"): out_tm, p.get("mel_ref"): out_ref}


def emulate_to_tm(p, st, dt, defect):
    nm, B = p["n_mels"], p["batch"]
    out = st[p["mel_tm"]].copy().reshape(-1, MEL_ROWS, nm)
    src = st[p["mel_ref"]].reshape(-1, nm, FRAMES_OUT)
    at = 0 if defect == "tm_row_f" else 1
    for b in range(B):
        out[b, at: at + FRAMES_OUT] = to_bits(np.ascontiguousarray(src[b].T), dt).reshape(FRAMES_OUT, nm)
    return {p["mel_tm"]: out}


EMULATE = {"frontend": emulate_frontend, "frontend_long": emulate_frontend_long, "mel_window": emulate_window, "mel_to_tm": emulate_to_tm}


def result_of(dt, defect=None):
    def result(gi, li, launch, state):
        cmd, ident, p, outs = launch
        made = EMULATE[cmd](p, R.typed(p, state), dt, defect)
        return R.grid_of(cmd, p), {o: with_guards(made[o] if made.get(o) is not None else state[o]) for o in outs}
    return result


def run(name, dt, defect=None, session=None, only=None):
    groups = [g for g in R.CASES[name](dt) if only is None or only(g[1][0][1])]
    assert groups
    return kernel_driver.check_groups(session or kernel_driver.Session(), R.verify, R.form_of, R.grid_of, dt, groups, result_of(dt, defect))


# ------------------------------------------------------------------------------------------ tests
_session = kernel_driver.Session()


@pytest.mark.parametrize("name", list(R.CASES))
def test_emulation_passes(name):
    dt = "f16" if list(R.CASES).index(name) % 2 else "bf16"  # the builds differ only in the narrowing, which every case has
    notes = run(name, dt, session=_session)
    assert notes and max(notes.values()) <= 1.0


def test_emulation_ran_every_form():
    assert R.WANTED_FORMS <= _session.ran["bf16"] | _session.ran["f16"], sorted(R.WANTED_FORMS - _session.ran["bf16"] - _session.ran["f16"], key=str)
    for (dt, what), w in sorted(_session.worst.items()):
        print(f"emulation {dt} {what}: worst error / bound {w:.3f}")


DEFECTS = {
    "right_reflect": "clip n=5119", "left_reflect": "clip n=401", "fast_at_n": "clip n=10279", "overflow_plus1": "staging-row edge",
    "over_off0": "staging-row edge", "bin201": "dense basis", "bin200": "dense basis", "filter_m1": "clip n=401",
    "gmax_first3000": "long clip 3034 frames", "gmax_batch": "ragged batch", "no_reset": "ragged batch", "stale_rows": "ragged batch",
    "ordered_neg": "ragged batch", "tm_row_f": "clip n=160", "window_next_file": "window mel_tm", "window_64": "window both",
    "tile_no_carry": "window mel_ref"}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_seeded_defect_fails(defect):
    with pytest.raises(AssertionError):
        run(DEFECTS[defect], "bf16", defect)


def test_tile_carry_matters_only_at_80_mels():
    """10 column groups per frame: 256 threads do not cover whole frames, so the running index needs its carry; 16 groups do."""
    run("window mel_ref", "bf16", "tile_no_carry", only=lambda ident: ident.endswith(".128"))
    with pytest.raises(AssertionError):
        run("window mel_ref", "bf16", "tile_no_carry", only=lambda ident: ident.endswith(".80"))


def test_dropped_last_k_step_fails_on_the_sparse_family_only():
    """Samples 398 and 399 carry a Hann weight of 6e-5: on every dense family a DFT without them stays inside the any-order bound
    over 400 terms — which is why the sparse family, whose bound counts the two or three non-zero samples of a frame, is there."""
    for fam in R.FAMILIES:
        only = lambda ident, fam=fam: ident.split(".")[1] == fam
        if fam in ("sparse", "sparse398"):
            with pytest.raises(AssertionError):
                run("clip n=10441", "bf16", "drop_last_k", only=only)
        else:
            run("clip n=10441", "bf16", "drop_last_k", only=only)


def test_frame_index_rule():
    """For n >= 201 the rule is numpy's reflect padding; below, one reflection per side and then the clamp (pinned values)."""
    for n in (201, 202, 399, 401, 1000):
        x = np.arange(n, dtype=np.float32) + 1
        pad = np.pad(x, N_FFT // 2, mode="reflect")
        want = np.stack([pad[f * HOP: f * HOP + N_FFT] for f in range(1 + n // HOP)])
        assert (R.frame_samples(x) == want).all()
    assert R.frame_index(np.arange(-200, 200), 1).tolist() == [0] * 400
    assert R.frame_index([-200, -4, -3, -1, 0, 2, 3, 4, 5, 199], 3).tolist() == [0, 0, 1, 1, 0, 2, 1, 0, 0, 0]  # -200 -> 200 -> -196 -> clamp
    j = R.frame_index(np.arange(-200, 360), 200)  # the second frame of a 200-sample clip ends at position 359
    assert j[0] == 198 and j[1] == 199 and j[2] == 198 and j[200] == 0 and j[400] == 198 and j[559] == 39


def test_ordered_code():
    v = np.array([-np.inf, -10.0, -1e-30, -0.0, 0.0, 1e-30, 2.5, np.inf], dtype=np.float32)
    codes = [R.ordered(x) for x in v]
    assert codes == sorted(codes) and all(c > 0 for c in codes)
    assert all(R.unordered(c).view(np.uint32) == x.view(np.uint32) for c, x in zip(codes, v))
