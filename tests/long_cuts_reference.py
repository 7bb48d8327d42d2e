"""Python restatement of chunked long-form (DESIGN.md "Chunked long-form"; csrc/long_cuts.hpp states the definitions, this file
restates them independently): the levels in float64, the cut rule, a window's segments in file time, and the per-element bound of the
levels kernel's fp32 sums.

    x[f][m] = (max(S[f][m], G - 8) + 4) / 4      what the encoder will see of store row f (fp32, mel_window_kernel's arithmetic)
    e[f]    = mean over m of x[f][m]
    s[f]    = 1 / (2 R + 1) * sum over j = -R .. R of e[clamp(f + j, 0, n_frames - 1)]

The cut rule is a function of the float32 array s and three integers (content, W_min, W_max)."""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32


def frame_levels(x, smooth):
    """x: [n_frames][n_mels] (what the encoder will see, any float type) -> (e, s) in float64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    e = x.mean(axis=1)
    idx = np.clip(np.arange(n)[:, None] + np.arange(-smooth, smooth + 1)[None, :], 0, n - 1)
    s = e[idx].sum(axis=1) / (2 * smooth + 1)
    return e, s


def levels_bounds(x, e_got, smooth):
    """Per-element bounds of the kernel's e and s against frame_levels of the same float32 x (csrc/long_cuts.hip states the order of
    the sums; the bound holds for ANY order, to first order in u with the second-order terms covered by the factor 1.01).
      e: n_mels terms added in fp32 in some order: each partial sum is rounded once and every term passes through at most n_mels - 1
         additions: (n_mels - 1) u sum |x|; the division by n_mels rounds once more: u |e|. In all <= n_mels u mean |x|.
      s: its 2 R + 1 terms are the kernel's own e (each within its bound), added in fp32: 2 R u sum |e|, and divided: u |s|. In all
         mean of the e bounds over the box + (2 R + 1) u mean |e| over the box.
    The float64 reference's own rounding (2^-53 per operation) is below 1e-9 of these and is not added."""
    x = np.asarray(x, dtype=np.float64)
    n, nm = x.shape
    be = 1.01 * nm * U32 * np.abs(x).mean(axis=1)
    idx = np.clip(np.arange(n)[:, None] + np.arange(-smooth, smooth + 1)[None, :], 0, n - 1)
    w = 2 * smooth + 1
    bs = be[idx].sum(axis=1) / w + 1.01 * w * U32 * np.abs(np.asarray(e_got, dtype=np.float64))[idx].sum(axis=1) / w
    return be, bs


def check_params(w_min, w_max, smooth=0):
    if not (2 <= w_min <= w_max <= 3000) or w_min % 2 or w_max % 2 or not (0 <= smooth <= 64):
        raise ValueError("bad chunk parameters")


def cut_plan(s, w_min=2000, w_max=3000, content=None):
    """The cut rule, literally -> [(seek, len)]. s: float32 levels, content: frames of audio (default len(s))."""
    check_params(w_min, w_max)
    s = np.asarray(s, dtype=np.float32)
    content = len(s) if content is None else content
    out, seek = [], 0
    if content <= 0:
        return out
    while content - seek > w_max:
        cand = np.arange(seek + w_min, seek + w_max + 1, 2)
        v = s[cand]
        f = int(cand[np.nonzero(v == v.min())[0][-1]])  # the smallest level; of equal ones the latest frame
        out.append((seek, f - seek))
        seek = f
    out.append((seek, content - seek))
    return out


def check_plan(plan, content, w_min, w_max):
    """The invariants of every plan: the windows tile [0, content) without gap or overlap, every length but the last is even and
    in [W_min, W_max], the last is in [1, W_max]."""
    assert plan and plan[0][0] == 0
    for (a, la), (b, _) in zip(plan, plan[1:]):
        assert a + la == b
    assert plan[-1][0] + plan[-1][1] == content
    for _, l in plan[:-1]:
        assert l % 2 == 0 and w_min <= l <= w_max
    assert 1 <= plan[-1][1] <= w_max
    assert len(plan) <= -(-content // w_min) + 1


def chunked_segments(ids, T, E, seek, length):
    """One window's ids (eot excluded) -> [(start, end, tok_begin, tok_end)] in file time: the single-window split (pairs of
    consecutive timestamps close segments, a single closing timestamp closes the last, a tail after the last pair is kept and runs to
    the window's end, no pairs: one segment), every time t mapped to seek / 100 + min(t, length / 100)."""
    ids = list(ids)
    n = len(ids)
    clip, base = length * 0.01, seek * 0.01
    ts = lambda i: ids[i] >= T
    time = lambda i: (ids[i] - T) * 0.02
    out = []

    def emit(lo, hi, t0, t1):
        txt = [i for i in range(lo, hi) if ids[i] < E]
        if txt:
            out.append((base + min(t0, clip), base + min(t1, clip), txt[0], txt[-1] + 1))

    bounds = [i for i in range(1, n) if ts(i - 1) and ts(i)]
    if bounds:
        if n >= 2 and ts(n - 1) and not ts(n - 2):
            bounds.append(n)
        prev, prev_end = 0, 0.0
        for b in bounds:
            prev_end = time(b - 1)
            emit(prev, b, time(prev), prev_end)
            prev = b
        if prev < n:
            emit(prev, n, time(prev) if ts(prev) else prev_end, clip)
    else:
        last = [i for i in range(n) if ts(i)]
        emit(0, n, 0.0, time(last[-1]) if last and ids[last[-1]] != T else clip)
    return out


def cut_window(norm, seek, length):
    """[n_mels][3000] float32: rows [seek, seek + length) of a file's normalised rows, zero from frame `length` on and past the file."""
    n_frames, n_mels = norm.shape
    out = np.zeros((n_mels, 3000), dtype=np.float32)
    k = max(0, min(length, 3000, n_frames - seek))
    out[:, :k] = norm[seek:seek + k].T.astype(np.float32)
    return out


def crafted_levels():
    """name -> (s float32, W_min, W_max): the cases the host rule and the plan kernel are both checked on."""
    rng = np.random.default_rng(20261)
    cases = {}
    s = rng.uniform(1.0, 2.0, 700).astype(np.float32)
    s[260] = 0.25
    cases["one_clear_minimum"] = (s, 200, 300)
    s = np.full(900, 1.5, dtype=np.float32)
    s[[210, 250, 290]] = 0.5  # three equal minima in the first range: 290 wins; then everything ties: the latest frame
    cases["exact_ties"] = (s, 200, 300)
    s = rng.uniform(1.0, 2.0, 700).astype(np.float32)
    s[251] = -5.0  # the smallest level of all, on an odd frame
    s[240] = 0.75
    cases["odd_minimum_not_taken"] = (s, 200, 300)
    cases["signed_zero_tie"] = (np.where(np.arange(700) % 4 == 0, -0.0, 0.0).astype(np.float32), 200, 300)
    for name, n in (("one_window", 300), ("one_window_short", 7), ("content_wmax_plus_1", 301), ("content_wmax_plus_wmin", 500)):
        cases[name] = (rng.uniform(0.0, 1.0, n).astype(np.float32), 200, 300)
    cases["wmin_equals_wmax"] = (rng.uniform(0.0, 1.0, 1000).astype(np.float32), 300, 300)
    cases["smallest_windows"] = (rng.uniform(0.0, 1.0, 41).astype(np.float32), 2, 4)
    cases["full_size"] = (rng.uniform(0.0, 1.0, 9000).astype(np.float32), 2000, 3000)
    return cases


def random_levels(k):
    """Seeded random array k of 20 000 frames (W = 200 / 300); quantised so that exact ties occur."""
    rng = np.random.default_rng(1000 + k)
    return np.round(rng.uniform(0.0, 1.0, 20000) * 64).astype(np.float32) / np.float32(64)
