"""Float64 references of the log-mel front-end kernels (whisper.axera_amd/csrc/frontend.hip, frontend_stft.inc), the checker that
compares EVERY output element of a launch under a bound computed per element (never a constant) and every element a launch must
not write bit for bit with what was there before, and the cases of tests/test_gpu_frontend_kernels.py.

Notation: u = 2^-24, gamma_n = n u / (1 - n u). x: the clip's float32 samples, w: the float32 Hann window, (cos, sin): the float32
twiddle table, B: the float32 filterbank; the references read these VALUES and compute in float64.

The frame index rule (the engine's definition; below 201 samples it is the only one there is, since the reference program and
oracle.log_mel index outside their buffers there): sample k of frame f is x[r(160 f + k - 200)],
    r(j):  j < 0 -> -j ;  then j >= n -> 2 n - 2 - j ;  then a clamp into [0, n - 1]
— one reflection per side, then the clamp. For n >= 201 no clamp happens and r is numpy's pad(mode="reflect")
(tests/test_frontend_kernel_reference.py checks that). `openai` mode: n = 480000 virtual samples, zeros behind the clip's end,
3000 frames, every one of them written (no zero fill).

stft_mel_kernel / stft_mel_long_kernel, per frame and mel:
  frame sample  v_k = fl(x w): ONE rounding, which float32 numpy reproduces exactly, so v is an input of the bound.
  DFT           a bin accumulates the z non-zero products of the frame (z = number of non-zero v_k) in the MFMA's fixed order:
                e_re = gamma_(z+1) sum_k |v_k| |cos_k|, e_im likewise (any order, fused or not).
  power         P = re^2 + im^2:  e_P = 2 |re| e_re + e_re^2 + 2 |im| e_im + e_im^2 + 3 u (P + those)  (two squares, one addition).
  mel           M = sum_k B_mk P_k:  e_M = sum_k B_mk e_P,k + gamma_(nz_m + 1) sum_k B_mk (P_k + e_P,k), nz_m = non-zero weights of m.
  log10         the interval is carried exactly: the kernel's argument lies in [max(M - e_M, c), max(M + e_M, c)], c = the float32
                nearest 1e-10 (the kernel's constant), so its result lies in [log10 of the lower end, log10 of the upper end]
                widened by the device log10f's own error E_log at the end of larger magnitude. No special case for the floor.
  E_log         LOG10F_ULPS float32 ulps of max(|lower|, |upper|) — evaluated at the interval's ends, not at the reference, so it
                stays valid near M = 1 where the reference's own ulp vanishes while the kernel's argument is still e_M away.
                The ROCm installation this was written on carries no device-library documentation that states the accuracy of
                log10f, so the figure is MEASURED (LOG10F_MEASURED below): 2.763 ulp on an MI355X against float64 log10 of the
                float64 mel sums, over the dumped elements with e_M / M < 2^-20; the bound takes 2 x that = 5.526 ulp.
  gmax          clips of <= 3000 frames and every file of the long kernel: exactly the ordered-int code of the maximum of the
                dumped logmel / store rows (max is exact). Clips with more frames: the decoded value is not below the maximum of
                the dumped rows and lies inside [max lower, max upper] over ALL frames.
mel_normalize_kernel, mel_window_kernel, mel_to_tm_kernel: bit for bit given the dumped logmel / store and gmax:
  (max(v, gmax - 8) + 4) * 0.25 in float32 (the product is exact), zero for frames past the end, round16 for the h16 rows, row f + 1
  of a slot for frame f.
What a launch must not write — the guards, logmel rows of frames >= n_frames, mel_tm row 0 and rows 3001..3003 of every slot, slots
and windows beyond the batch, store rows beyond a file's last frame and beyond the last file, every input — holds a NaN pattern
(or its input) before and the same bits after.
"""
import functools
import hashlib
import os
import sys

import numpy as np

from encoder_kernel_reference import GUARD, SENT16, sentinel, to_bits

U = 2.0 ** -24
N_FFT, HOP, BINS, FRAMES_OUT, MEL_ROWS = 400, 160, 201, 3000, 3004
FR, WF = 32, 64  # frames per workgroup of the STFT and of the window kernel
FLOOR = float(np.float32(1e-10))
# Error of the device log10f in float32 ulps of the result. Measured on an MI355X (tests/test_gpu_frontend_kernels.py,
# test_zz_report prints it): the worst |logmel - log10(M)| / ulp(log10(M)) over every dumped element whose e_M / M < 2^-20 (M: the
# float64 mel sum of the float64 reference, never another output of the kernel) was 2.763 ulp, at log10 M = -1.484. Only the sparse
# family has such elements, all of them with |log10 M| >= 1. The figure overstates log10f itself: it contains the error of the
# kernel's argument, which e_M / M < 2^-20 lets reach 2^-20 / ln 10 = 3.5 ulp at that magnitude (2.87 ulp at the worst element).
# The bound takes twice the measured figure.
LOG10F_MEASURED = 2.763
LOG10F_ULPS = 2.0 * LOG10F_MEASURED

F32 = ("pcm", "twiddle", "window", "basis", "power", "logmel", "mel_ref", "overflow", "store")
I32 = ("n_samples", "n_frames", "win_file", "win_seek")
I64 = ("over_off", "pcm_off", "frame_off")
U32 = ("gmax",)
POINTERS = F32 + I32 + I64 + U32 + ("mel_tm", "clip_logmel")
F32 = F32 + ("clip_logmel",)  # not a pointer of the launch: the buffer the launch before left the clip kernel's rows in


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def ulp32(x):
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return np.exp2(e - 23.0)


def frame_index(j, n):
    """The engine's rule: which sample of an n-sample clip stands at position j of the (virtually) padded signal."""
    j = np.asarray(j, dtype=np.int64)
    j = np.where(j < 0, -j, j)
    j = np.where(j >= n, 2 * n - 2 - j, j)
    return np.clip(j, 0, n - 1)


def n_frames_of(n_real, openai):
    return FRAMES_OUT if openai else 1 + n_real // HOP


def frame_samples(x, openai=False):
    """[n_frames][400] float32 samples of the frames of clip x (float32, the n_real real samples)."""
    n_real = len(x)
    n = FRAMES_OUT * HOP if openai else n_real
    j = frame_index(np.arange(n_frames_of(n_real, openai))[:, None] * HOP + np.arange(N_FFT)[None, :] - N_FFT // 2, n)
    ok = j < n_real
    out = np.zeros(j.shape, dtype=np.float32)
    out[ok] = x[j[ok]]
    return out


def ordered(v):
    """float32 -> the ordered-int code gmax holds."""
    u = int(np.float32(v).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def unordered(c):
    c = int(c)
    return np.uint32(c & 0x7FFFFFFF if c & 0x80000000 else ~c & 0xFFFFFFFF).view(np.float32)


def normalise(v, g):
    """mel_normalize_kernel's / mel_window_kernel's arithmetic on float32 log-mel values v under the maximum g."""
    floor_v = np.float32(g) - np.float32(8.0)
    return (np.maximum(v.astype(np.float32), floor_v) + np.float32(4.0)) * np.float32(0.25)


# ------------------------------------------------------------------------------------------ the tables a test supplies
def twiddle_table():
    i = np.arange(N_FFT)
    return np.stack([np.cos(2.0 * np.pi * i / N_FFT), np.sin(2.0 * np.pi * i / N_FFT)], axis=1).astype(np.float32)


def hann_window(openai):
    i = np.arange(N_FFT)
    if openai:  # torch.hann_window: double, then narrowed
        return (0.5 * (1.0 - np.cos(2.0 * np.pi * i / N_FFT))).astype(np.float32)
    a = i.astype(np.float32) * np.float32(2.0) * np.float32(np.pi) / np.float32(N_FFT)
    return np.float32(0.5) * (np.float32(1.0) - np.cos(a).astype(np.float32))


def librosa_basis(n_mels):
    """librosa.filters.mel as the engine builds it for feature_mode openai: ramps in float64, narrowed, times the float64 Slaney
    norm, narrowed again. [n_mels][201]."""
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    max_mel = min_log_mel + np.log(8000.0 / min_log_hz) / logstep
    mel = max_mel * np.arange(n_mels + 2) / (n_mels + 1)
    mel_f = np.where(mel >= min_log_mel, min_log_hz * np.exp(logstep * (mel - min_log_mel)), f_sp * mel)
    freq = np.arange(BINS) * 16000.0 / N_FFT
    out = np.empty((n_mels, BINS), dtype=np.float32)
    for m in range(n_mels):
        w = np.minimum(-(mel_f[m] - freq) / (mel_f[m + 1] - mel_f[m]), (mel_f[m + 2] - freq) / (mel_f[m + 2] - mel_f[m + 1]))
        out[m] = (np.maximum(w, 0.0).astype(np.float32).astype(np.float64) * (2.0 / (mel_f[m + 2] - mel_f[m]))).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def basis(n_mels, kind):
    """[n_mels][201] float32: "slaney" the oracle's filterbank, "librosa" the openai mode's, "dense" a probe with no zero weight
    (bin 200 carries none in the two real ones: their last filter ends at 8000 Hz)."""
    if kind == "librosa":
        return librosa_basis(n_mels)
    if kind == "dense":
        return np.random.default_rng(7 + n_mels).uniform(0.01, 0.05, (n_mels, BINS)).astype(np.float32)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.join(root, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle
    return oracle.mel_filterbank(n_mels)


# ------------------------------------------------------------------------------------------ the STFT + mel reference
_cache = {}


def logmel_expect(x, openai, tw, win, basis_t, n_mels):
    """-> (ref, lo, hi, eM / M), float64 [n_frames][n_mels]: float64 log-mel of clip x and the interval the kernel's float32 value must
    lie in. Cached on the inputs' bytes (both builds and several launches see the same clips)."""
    key = hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in (x, tw, win, basis_t))).hexdigest() + f"{openai}{n_mels}"
    if key in _cache:
        return _cache[key]
    v32 = frame_samples(x, openai) * win.astype(np.float32)[None, :]  # one float32 rounding, as the kernel's
    v = v32.astype(np.float64)
    z = (v32 != 0).sum(axis=1)
    idx = (np.arange(N_FFT)[:, None] * np.arange(BINS)[None, :]) % N_FFT
    t = tw.reshape(N_FFT, 2).astype(np.float64)
    c, s = t[idx, 0], t[idx, 1]
    re, im = v @ c, v @ s
    g = gamma(z + 1)[:, None]
    e_re, e_im = g * (np.abs(v) @ np.abs(c)), g * (np.abs(v) @ np.abs(s))
    P = re * re + im * im
    eP = 2 * np.abs(re) * e_re + e_re ** 2 + 2 * np.abs(im) * e_im + e_im ** 2
    eP = eP + 3 * U * (P + eP)
    Bt = basis_t.reshape(BINS, n_mels).astype(np.float64)
    nz = (Bt != 0).sum(axis=0)
    M = P @ Bt
    eM = eP @ Bt + gamma(nz + 1)[None, :] * ((P + eP) @ Bt)
    ref = np.log10(np.maximum(M, FLOOR))
    lo, hi = np.log10(np.maximum(M - eM, FLOOR)), np.log10(np.maximum(M + eM, FLOOR))
    e_log = LOG10F_ULPS * ulp32(np.maximum(np.abs(lo), np.abs(hi)))
    rel = np.where(M > FLOOR, eM / np.maximum(M, 1e-300), np.inf)
    if len(_cache) > 64:
        _cache.clear()
    _cache[key] = (ref, lo - e_log, hi + e_log, rel)
    return _cache[key]


# ------------------------------------------------------------------------------------------ checking
def tv(a, dtype):
    return np.ascontiguousarray(a).reshape(-1).view(dtype)


def strip(name, got):
    g = GUARD // 2
    got = np.ascontiguousarray(got).view(np.uint16).ravel()
    assert (got[:g] == SENT16).all() and (got[-g:] == SENT16).all(), f"{name}: store into a guard"
    return got[g:-g]


def same_bits(ident, name, got, want, what="must not change"):
    got, want = tv(got, np.uint16), tv(want, np.uint16)
    assert got.size == want.size, (ident, name, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{ident} {name}: {bad.size} 16-bit words differ ({what}), first at {bad[0]}: {got[bad[0]]:#06x} for {want[bad[0]]:#06x}"


def in_interval(ident, got, ref, lo, hi):
    """got float32 values inside [lo, hi]; -> worst (distance from ref) / (distance of that side's end from ref)."""
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), f"{ident}: {np.count_nonzero(~np.isfinite(got))} values are not finite"
    ratio = np.where(got >= ref, (got - ref) / (hi - ref), (ref - got) / (ref - lo))
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{ident}: error / bound {worst:.3g} at {i}: got {got[i]!r}, float64 {ref[i]!r}, interval [{lo[i]!r}, {hi[i]!r}]")
    return worst


log10f_seen = {"ulps": 0.0}  # the measurement behind LOG10F_MEASURED, updated by every checked STFT launch


def _measure_log10f(got, ref, rel):
    tight = rel < 2.0 ** -20
    if tight.any():
        e = np.abs(got.astype(np.float64)[tight] - ref[tight]) / ulp32(ref[tight])
        log10f_seen["ulps"] = max(log10f_seen["ulps"], float(e.max()))


def clip_samples(p, st, b):
    n, stride = int(st[p["n_samples"]][b]), p["stride"]
    x = st[p["pcm"]][b * stride: b * stride + min(n, stride)]
    if n > stride:
        o = int(st[p["over_off"]][b])
        x = np.concatenate([x, st[p["overflow"]][o: o + n - stride]])
    return x.astype(np.float32)


def typed(p, state):
    """state (name -> content before the launch, any dtype or the uint16 of an earlier dump) -> typed flat arrays by the launch's keys."""
    out = {}
    for k in POINTERS:
        name = p.get(k)
        if name and name != "-":
            out[name] = tv(state[name], np.float32 if k in F32 else np.int32 if k in I32 else np.int64 if k in I64 else np.uint32 if k in U32 else np.uint16)
    return out


def _normalised_outputs(ident, p, st, got, dt, rows_of, n_slots, notes_key):
    """mel_ref / mel_tm of a launch bit for bit: rows_of(a) -> float32 [3000][n_mels] of slot a (already normalised, zero filled)."""
    nm = p["n_mels"]
    for key in ("mel_ref", "mel_tm"):
        name = p.get(key)
        if not name or name == "-":
            continue
        want = st[name].copy()
        for a in range(n_slots):
            rows = rows_of(a)
            if key == "mel_ref":
                want.reshape(-1, nm, FRAMES_OUT)[a] = rows.T
            else:
                want.reshape(-1, MEL_ROWS, nm)[a, 1: 1 + FRAMES_OUT] = to_bits(rows, dt).reshape(FRAMES_OUT, nm)
        same_bits(ident, name, strip(f"{ident} {name}", got[name]), want, "normalised rows bit for bit, everything else untouched")
    return {notes_key: 0.0}


def verify_frontend(ident, p, st, got, dt):
    nm, B, openai = p["n_mels"], p["batch"], bool(p.get("openai"))
    tw, win, bt = st[p["twiddle"]], st[p["window"]], st[p["basis"]]
    logmel = strip(f"{ident} logmel", got[p["logmel"]]).view(np.float32).reshape(-1, FRAMES_OUT, nm)
    before = st[p["logmel"]].reshape(-1, FRAMES_OUT, nm)
    gmax = strip(f"{ident} gmax", got[p["gmax"]]).view(np.uint32)
    label = f"frontend{' openai' if openai else ''} {nm} mels {p.get('family', '')}"
    notes, rows = {}, []
    for b in range(B):
        x = clip_samples(p, st, b)
        ref, lo, hi, rel = logmel_expect(x, openai, tw, win, bt, nm)
        nf_all = ref.shape[0]
        assert p["max_frames"] >= nf_all, "a case must launch every frame of its clips"
        nf = min(nf_all, FRAMES_OUT)
        _measure_log10f(logmel[b, :nf], ref[:nf], rel[:nf])
        w = in_interval(f"{ident} clip {b} logmel", logmel[b, :nf], ref[:nf], lo[:nf], hi[:nf])
        notes[f"{label} logmel"] = max(notes.get(f"{label} logmel", 0.0), w)
        same_bits(ident, f"logmel clip {b} rows >= {nf}", logmel[b, nf:], before[b, nf:])
        g, top = unordered(gmax[b]), logmel[b, :nf].max()
        if nf_all <= FRAMES_OUT:
            assert int(gmax[b]) == ordered(top), f"{ident} clip {b}: gmax {int(gmax[b]):#x} = {g!r}, the dumped rows' maximum is {top!r} = {ordered(top):#x}"
        else:
            assert np.isfinite(g) and g >= top and lo.max() <= g <= hi.max(), f"{ident} clip {b}: gmax {g!r}, dumped rows' maximum {top!r}, float64 maximum in [{lo.max()!r}, {hi.max()!r}]"
            notes[f"{label} gmax beyond 3000 frames"] = abs(float(g) - ref.max()) / max(hi.max() - ref.max(), ref.max() - lo.max())
        r = np.zeros((FRAMES_OUT, nm), dtype=np.float32)
        r[:nf] = normalise(logmel[b, :nf], g)
        rows.append(r)
    same_bits(ident, "logmel beyond the batch", logmel[B:], before[B:])
    same_bits(ident, "gmax beyond the batch", gmax[B:], st[p["gmax"]][B:])
    notes.update(_normalised_outputs(ident, p, st, got, dt, lambda a: rows[a], B, f"{label} normalise (bits)"))
    return notes, {p["logmel"], p["gmax"], p.get("mel_ref"), p.get("mel_tm")}


def verify_frontend_long(ident, p, st, got, dt):
    nm, B = p["n_mels"], p["batch"]
    tw, win, bt = st[p["twiddle"]], st[p["window"]], st[p["basis"]]
    store = strip(f"{ident} store", got[p["store"]]).view(np.float32).reshape(-1, nm)
    want = st[p["store"]].reshape(-1, nm).copy()
    gmax = strip(f"{ident} gmax", got[p["gmax"]]).view(np.uint32)
    label, worst = f"frontend_long {nm} mels {p.get('family', '')}", 0.0
    total = 0
    for b in range(B):
        n, po, fo = int(st[p["n_samples"]][b]), int(st[p["pcm_off"]][b]), int(st[p["frame_off"]][b])
        x = st[p["pcm"]][po: po + n].astype(np.float32)
        ref, lo, hi, rel = logmel_expect(x, False, tw, win, bt, nm)
        nf = ref.shape[0]
        total += nf
        rows = store[fo: fo + nf]
        _measure_log10f(rows, ref, rel)
        worst = max(worst, in_interval(f"{ident} file {b} store", rows, ref, lo, hi))
        assert int(gmax[b]) == ordered(rows.max()), f"{ident} file {b}: gmax {int(gmax[b]):#x}, the rows' maximum is {rows.max()!r} = {ordered(rows.max()):#x}"
        want[fo: fo + nf] = rows
        if p.get("clip_logmel"):  # the clip kernel's rows for the same samples, left by the launch before: bit-equal
            clip = st[p["clip_logmel"]].reshape(-1, FRAMES_OUT, nm)[b, :nf]
            same_bits(ident, f"store rows of file {b} against the clip kernel's logmel", rows, clip, "frontend_stft.inc: one text, one arithmetic")
    same_bits(ident, "store rows no file owns", store, want)
    assert p.get("rows") is None or total == p["rows"], (total, p.get("rows"))
    same_bits(ident, "gmax beyond the files", gmax[B:], st[p["gmax"]][B:])
    return {f"{label} store": worst}, {p["store"], p["gmax"]}


def window_rows(p, st, a):
    nm = p["n_mels"]
    f, seek = int(st[p["win_file"]][a]), int(st[p["win_seek"]][a])
    nv = min(max(int(st[p["n_frames"]][f]) - seek, 0), FRAMES_OUT)
    r = np.zeros((FRAMES_OUT, nm), dtype=np.float32)
    fo = int(st[p["frame_off"]][f]) + seek
    r[:nv] = normalise(st[p["store"]].reshape(-1, nm)[fo: fo + nv], unordered(st[p["gmax"]][f]))
    return r


def verify_window(ident, p, st, got, dt):
    label = f"mel_window {p['n_mels']} mels {form_of('mel_window', p)[2]} (bits)"
    return _normalised_outputs(ident, p, st, got, dt, lambda a: window_rows(p, st, a), p["n_windows"], label), {p.get("mel_ref"), p.get("mel_tm")}


def verify_to_tm(ident, p, st, got, dt):
    nm = p["n_mels"]
    src = st[p["mel_ref"]].reshape(-1, nm, FRAMES_OUT)
    q = dict(p, mel_ref=None)
    return _normalised_outputs(ident, q, st, got, dt, lambda a: np.ascontiguousarray(src[a].T), p["batch"], f"mel_to_tm {nm} mels (bits)"), {p["mel_tm"]}


def verify(cmd, ident, p, state, got, dt, prev=None):
    """state: buffer name -> content before the launch; got: buffer name -> uint16 dump with guards after it."""
    st = typed(p, state)
    notes, written = {"frontend": verify_frontend, "frontend_long": verify_frontend_long, "mel_window": verify_window, "mel_to_tm": verify_to_tm}[cmd](ident, p, st, got, dt)
    for name in got:  # everything else the launch names: read-only
        if name not in written:
            same_bits(ident, name, strip(f"{ident} {name}", got[name]), state[name], "an input")
    return notes


def form_of(cmd, p, qall=None):
    if cmd == "frontend":
        return (cmd, p["n_mels"], "openai" if p.get("openai") else "clip")
    if cmd == "mel_window":
        has = [k for k in ("mel_tm", "mel_ref") if p.get(k) and p[k] != "-"]
        return (cmd, p["n_mels"], "both" if len(has) == 2 else has[0])
    return (cmd, p["n_mels"], "")


def grid_of(cmd, p):
    if cmd in ("frontend", "frontend_long"):
        return (p["max_frames"] + FR - 1) // FR, p["batch"], 1
    if cmd == "mel_window":
        return (FRAMES_OUT + WF - 1) // WF, p["n_windows"], 1
    return 64, p["batch"], 1


WANTED_FORMS = {("frontend", nm, mode) for nm in (80, 128) for mode in ("clip", "openai")} | \
               {(k, nm, "") for nm in (80, 128) for k in ("frontend_long", "mel_to_tm")} | \
               {("mel_window", nm, o) for nm in (80, 128) for o in ("mel_tm", "mel_ref", "both")}


# ------------------------------------------------------------------------------------------ inputs
FAMILIES = ("sparse", "sparse398", "tone", "noise", "speech", "zeros", "dc")
DENSE = ("tone", "noise", "speech", "dc")


def family(name, n, seed, amp=1.0):
    """n float32 samples. sparse: one non-zero sample every 173 (successive frames see every sample position), amplitudes 0.2 .. 1 with
    random sign; sparse398: the same with a 100 x impulse on sample 399 and a -60 x one on sample 398 of frame 5; tone: 440 Hz plus 1e-3 noise; speech: harmonics of 120 Hz under a 3 Hz envelope plus a 1e-3 noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    if name in ("sparse", "sparse398"):
        x = np.zeros(n)
        idx = np.arange(99 if n > 3600 else seed % 173, n, 173)  # from 99: impulse 20 is sample 399 of frame 21 (Hann weight 6e-5)
        x[idx] = rng.uniform(0.2, 1.0, idx.size) * rng.choice([-1.0, 1.0], idx.size)
        if name == "sparse398" and n > 5 * HOP + 199:
            x[5 * HOP + 199] = 100.0
            x[5 * HOP + 198] = -60.0
    elif name == "tone":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t) + 1e-3 * rng.standard_normal(n)
    elif name == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif name == "speech":
        x = sum(np.sin(2 * np.pi * 120.0 * k * t + k) / k for k in range(1, 21)) * 0.2 * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t)) + 1e-3 * rng.standard_normal(n)
    elif name == "zeros":
        x = np.zeros(n)
    else:
        x = np.full(n, 0.25)
    return (amp * x).astype(np.float32)


def constants(nm, openai=False, basis_kind=None):
    b = basis(nm, basis_kind or ("librosa" if openai else "slaney"))
    return {"tw": twiddle_table(), "win": hann_window(openai), "basis": np.ascontiguousarray(b.T)}


def frontend_launch(ident, nm, clips, *, stride, openai, pcm="pcm", ns="ns", tails=False, ref=True, tm=True, power=False, fam="mixed"):
    p = dict(family=fam, pcm=pcm, n_samples=ns, twiddle="tw", window="win", basis="basis", logmel="logmel", gmax="gmax", stride=stride, batch=len(clips), n_mels=nm,
             max_frames=max(n_frames_of(len(c), openai) for c in clips), openai=int(openai))
    if ref:
        p["mel_ref"] = "mel_ref"
    if tm:
        p["mel_tm"] = "mel_tm"
    names = [pcm, ns, "tw", "win", "basis", "logmel", "gmax"] + (["mel_ref"] if ref else []) + (["mel_tm"] if tm else [])
    if tails:
        p.update(overflow="overflow", over_off="over_off")
        names += ["overflow", "over_off"]
    if power:  # FrontendParams::power: read and written by no kernel
        p["power"] = "power"
        names.append("power")
    return ("frontend", ident, p, names)


def pcm_rows(clips, stride, seed):
    """[len(clips) + 1][stride]: each clip's first `stride` samples, and NOISE behind a clip's end and in the row after the last, so a
    read beyond a clip or beyond the buffer's last row does not find zeros; -> (rows, overflow, over_off) with the tails packed."""
    rng = np.random.default_rng(seed)
    rows = (0.7 * rng.standard_normal((len(clips) + 1, stride))).astype(np.float32)
    over, off = [(0.7 * rng.standard_normal(3)).astype(np.float32)], []
    for b, c in enumerate(clips):
        rows[b, :min(len(c), stride)] = c[:stride]
        at = sum(len(o) for o in over)
        if b and len(c) > stride and at % 4 == 0:  # a later clip's offset: non-zero and no multiple of 4
            over.append((0.7 * rng.standard_normal(1)).astype(np.float32))
            at += 1
        off.append(at)
        over.append(c[stride:])
        over.append((0.7 * rng.standard_normal(2)).astype(np.float32))
    return rows, np.concatenate(over), np.array(off, dtype=np.int64)


def clip_group(dt, ident, nm, clips, *, stride=None, openai=False, seed=0, second=None, basis_kind=None, ref=True, tm=True, power=False, fam="mixed"):
    """One launch_frontend over `clips` (and a second on the same output buffers over `second`); every output has one slot more than
    the batch, NaN before."""
    longest = max(len(c) for c in clips + (second or []))
    stride = stride or longest + 5
    B = len(clips)
    bufs = constants(nm, openai, basis_kind)
    rows, over, off = pcm_rows(clips, stride, seed)
    tails = longest > stride
    bufs.update(pcm=rows, ns=np.array([len(c) for c in clips], dtype=np.int32), logmel=sentinel((B + 1) * FRAMES_OUT * nm, 4), gmax=sentinel(B + 1, 4))
    if ref:
        bufs["mel_ref"] = sentinel((B + 1) * nm * FRAMES_OUT, 4)
    if tm:
        bufs["mel_tm"] = sentinel((B + 1) * MEL_ROWS * nm, 2)
    if tails:
        bufs.update(overflow=over, over_off=off)
    if power:
        bufs["power"] = sentinel(256, 4)
    launches = [frontend_launch(f"{ident}.{nm}", nm, clips, stride=stride, openai=openai, tails=tails, ref=ref, tm=tm, power=power, fam=fam)]
    if second:
        assert len(second) <= B and not tails
        bufs.update(pcm2=pcm_rows(second, stride, seed + 1)[0], ns2=np.array([len(c) for c in second], dtype=np.int32))
        launches.append(frontend_launch(f"{ident}.{nm}.second", nm, second, stride=stride, openai=openai, pcm="pcm2", ns="ns2", ref=ref, tm=tm, fam=fam))
    return bufs, launches


LENGTHS = (1, 159, 160, 200, 201, 401, 5119, 5120, 10279, 10280, 10441)
EDGE = ((8001, 12345), (8199, 8200), (8201, 8000))
LONG = {"3000 frames": 479840, "3001 frames": 480000, "3034 frames": 480000 + 33 * HOP}
OPENAI = (10441, 479900, 480500)
FILES = (10441, 160, 25761)
WINDOW_FILES = (100, 3000, 3137)
WINDOWS = ((0, 0), (0, 36), (0, 37), (0, 99), (0, 100), (0, 5000), (1, 0), (2, 137), (2, 138))


def length_case(n):
    """One clip per launch: the sparse family and one dense family per length, 10441 samples with every family."""
    fams = FAMILIES if n == 10441 else ("sparse", DENSE[LENGTHS.index(n) % len(DENSE)])
    return lambda dt: [clip_group(dt, f"n{n}.{fam}", nm, [family(fam, n, 1000 + n + i)], seed=n + i, fam=fam) for nm in (80, 128) for i, fam in enumerate(fams)]


def edge_case(dt):
    """stride 8000: two clips per launch, their tails in one overflow buffer, the neighbour's samples behind each staging row."""
    return [clip_group(dt, f"edge{a}.{fam}", nm, [family(fam, a, 2000 + a), family(fam, b, 2000 + b)], stride=8000, seed=a, fam=fam)
            for nm in (80, 128) for (a, b), fam in zip(EDGE, ("sparse", "noise", "sparse398"))]


def ragged_case(dt):
    """(401, 10441, 5120) samples, loudness 1 / 1e-3 / silent — a clip with positive maximum, one with every value negative, one at the
    floor — and a second launch on the same buffers with shorter, quieter clips: the reset, and the zero fill over stale rows."""
    gs = []
    for nm in (80, 128):
        first = [family("noise", 401, 31, 3.0), family("speech", 10441, 32, 1e-3), family("zeros", 5120, 33)]
        second = [family("sparse", 200, 34, 1e-2), family("noise", 3000, 35, 1e-4), family("tone", 401, 36, 1e-3)]
        gs.append(clip_group(dt, "ragged", nm, first, seed=30, second=second, power=True))
    return gs


def long_case(name):
    def make(dt):
        n = LONG[name]
        x = family("sparse", n, 4000 + n)
        if name == "3034 frames":  # the loudest impulse where no frame below 3000 sees it, at the centre of the last frame (3033)
            x[n - 20] = 50.0
        return [clip_group(dt, name.replace(" ", ""), nm, [x], seed=n, ref=nm == 80, tm=True, fam="sparse") for nm in (80, 128)]
    return make


def openai_case(n):
    return lambda dt: [clip_group(dt, f"openai{n}.{fam}", nm, [family(fam, n, 5000 + n)], openai=True, seed=n, ref=nm == 80, fam=fam)
                       for nm, fam in ((80, "sparse"), (128, "speech" if n < 100000 else "sparse"))]


def dense_basis_case(dt):
    """A filterbank without a zero weight (the probe the column of bin 200 needs: the real filterbanks end at 8000 Hz = bin 200)."""
    return [clip_group(dt, f"densebasis.{fam}", nm, [family(fam, 5120, 77)], seed=77, basis_kind="dense", ref=False, fam=fam) for nm in (80, 128) for fam in ("noise", "sparse")]


def files_case(dt):
    """Three files back to back: first the clip kernel over the same samples (one clip each), then ONE launch_frontend_long; the store
    has a sentinel row block behind the last file."""
    gs = []
    for nm in (80, 128):
        files = [family(fam, n, 6000 + n) for n, fam in zip(FILES, ("sparse", "noise", "sparse398"))]
        bufs, launches = clip_group(dt, "files.clip", nm, files, seed=60, ref=False, tm=False)
        nfr = [n_frames_of(len(f), False) for f in files]
        bufs.update(lpcm=np.concatenate(files), lns=np.array([len(f) for f in files], dtype=np.int32), pcm_off=np.cumsum([0] + [len(f) for f in files[:-1]]).astype(np.int64),
                    frame_off=np.cumsum([0] + nfr[:-1]).astype(np.int64), store=sentinel((sum(nfr) + 5) * nm, 4), lgmax=sentinel(len(files) + 1, 4))
        p = dict(pcm="lpcm", n_samples="lns", twiddle="tw", window="win", basis="basis", gmax="lgmax", pcm_off="pcm_off", frame_off="frame_off", store="store",
                 batch=len(files), n_mels=nm, max_frames=max(nfr), clip_logmel="logmel", rows=sum(nfr), family="mixed")
        launches.append(("frontend_long", f"files.{nm}", p, ["lpcm", "lns", "tw", "win", "basis", "lgmax", "pcm_off", "frame_off", "store"]))
        gs.append((bufs, launches))
    return gs


def window_case(outputs):
    """The store is an input: random values on both sides of each file's floor, the next file's rows directly behind each file."""
    def make(dt):
        gs = []
        for nm in (80, 128):
            rng = np.random.default_rng(700 + nm)
            nfr = np.array(WINDOW_FILES, dtype=np.int32)
            store = rng.uniform(-11.0, 1.5, (int(nfr.sum()), nm)).astype(np.float32)
            gmax = np.array([ordered(np.float32(v)) for v in (1.25, -1.5, 0.75)] + [0], dtype=np.uint32)  # floors -6.75, -9.5, -7.25
            W = len(WINDOWS)
            bufs = dict(store=store, frame_off=np.cumsum([0] + list(nfr[:-1])).astype(np.int64), n_frames=nfr, gmax=gmax,
                        win_file=np.array([w[0] for w in WINDOWS], dtype=np.int32), win_seek=np.array([w[1] for w in WINDOWS], dtype=np.int32))
            p = dict(store="store", frame_off="frame_off", n_frames="n_frames", gmax="gmax", win_file="win_file", win_seek="win_seek", n_mels=nm, n_windows=W, n_files=3)
            if outputs in ("mel_tm", "both"):
                bufs["mel_tm"] = sentinel((W + 1) * MEL_ROWS * nm, 2)
                p["mel_tm"] = "mel_tm"
            if outputs in ("mel_ref", "both"):
                bufs["mel_ref"] = sentinel((W + 1) * nm * FRAMES_OUT, 4)
                p["mel_ref"] = "mel_ref"
            gs.append((bufs, [("mel_window", f"window.{outputs}.{nm}", p, list(bufs))]))
        return gs
    return make


def to_tm_case(dt):
    """Two clips; a third of the values on rounding ties of the build's 16-bit type (both neighbours' parity), the rest random."""
    gs = []
    keep = 8 if dt == "bf16" else 11  # significand bits the type keeps
    for nm in (80, 128):
        rng = np.random.default_rng(800 + nm)
        v = rng.uniform(-1.5, 1.5, 2 * nm * FRAMES_OUT).astype(np.float32)
        bits = v.view(np.uint32)
        tie = np.arange(v.size) % 3 == 0
        cut = np.uint32(24 - keep)
        bits[tie] = (bits[tie] >> cut << cut) | (np.uint32(1) << (cut - np.uint32(1)))
        bufs = dict(mel_ref=bits.view(np.float32), mel_tm=sentinel(3 * MEL_ROWS * nm, 2))
        gs.append((bufs, [("mel_to_tm", f"to_tm.{nm}", dict(mel_ref="mel_ref", mel_tm="mel_tm", batch=2, n_mels=nm), ["mel_ref", "mel_tm"])]))
    return gs


CASES = {f"clip n={n}": length_case(n) for n in LENGTHS}
CASES["staging-row edge"] = edge_case
CASES["ragged batch"] = ragged_case
CASES.update({f"long clip {k}": long_case(k) for k in LONG})
CASES.update({f"openai n={n}": openai_case(n) for n in OPENAI})
CASES["dense basis"] = dense_basis_case
CASES["files"] = files_case
CASES.update({f"window {o}": window_case(o) for o in ("mel_tm", "mel_ref", "both")})
CASES["mel_to_tm"] = to_tm_case
