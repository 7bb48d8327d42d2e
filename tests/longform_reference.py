"""Python restatement of the long-form contract (DESIGN.md "Long-form"): the window rule, the seek loop, and a whole-file log-mel
in numpy float64 that is pinned against oracle.log_mel below frame 3000 (tests/test_longform_host.py) and trusted beyond it.

AX_WHISPER_SplitWindow, the whole-file front-end + window kernel and AX_WHISPER_RunPCMLongWindows are checked against these."""
import numpy as np

N_FFT, HOP, WINDOW = 400, 160, 3000
GAINS = [1.0, 0.7, 1.3, 0.5, 0.9]
LENGTHS = {1: 12 * 16000, 2: 480000, 3: 45 * 16000, 4: 75 * 16000, 5: 100 * 16000}  # file k -> samples


def split_window(ids, T, E, window_frames):
    """The window rule, literally -> ([(start, end, tok_begin, tok_end)] relative to the window, advance in frames, branch).
    branch: "none" (no cuts), "single_end" (cuts and the ids end in a single timestamp), "cuts" (cuts, not single_end)."""
    ids = list(ids)
    n = len(ids)
    ts = lambda i: ids[i] >= T
    pos = lambda i: ids[i] - T
    segs = []

    def emit(lo, hi, t0, t1):
        txt = [i for i in range(lo, hi) if ids[i] < E]
        if txt:
            segs.append((t0, t1, txt[0], txt[-1] + 1))

    cuts = [i for i in range(1, n) if ts(i - 1) and ts(i)]
    single_end = n >= 2 and ts(n - 1) and not ts(n - 2)
    if cuts:
        bounds = cuts + ([n] if single_end else [])
        lo = 0
        for hi in bounds:
            emit(lo, hi, pos(lo) * 0.02, pos(hi - 1) * 0.02)
            lo = hi
        advance = window_frames if single_end else 2 * pos(bounds[-1] - 1)
        branch = "single_end" if single_end else "cuts"
    else:
        last = [i for i in range(n) if ts(i)]
        end = pos(last[-1]) * 0.02 if last and ids[last[-1]] != T else window_frames * 0.01
        emit(0, n, 0.0, end)
        advance = window_frames
        branch = "none"
    if advance <= 0 or advance > window_frames:  # the progress guard, and the cap
        advance = window_frames
    return segs, advance, branch


def loop(n_samples, decode, T, E):
    """The seek loop of one file: decode(seek, window_frames) -> ids. Returns [(seek, window_frames, advance, ids)]."""
    content = n_samples // HOP
    seek, out = 0, []
    while seek < content:
        wf = min(WINDOW, content - seek)
        ids = list(decode(seek, wf))
        _, adv, _ = split_window(ids, T, E, wf)
        out.append((seek, wf, adv, ids))
        seek += adv
    return out


def file_log_mel(pcm, n_mels, basis=None):
    """Whole-file log-mel in float64 -> (normalised [n_frames][n_mels] float64, n_frames, maximum before the clamp):
    reflect pad 200 at the file's two ends, periodic Hann, rfft, |.|^2, the oracle's mel filterbank, log10(max(., 1e-10)),
    one maximum over all frames, max(., max - 8), (. + 4) / 4."""
    if basis is None:
        import oracle

        basis = oracle.mel_filterbank(n_mels)
    x = np.asarray(pcm, dtype=np.float64)
    n = len(x)
    n_frames = 1 + n // HOP
    xp = np.pad(x, N_FFT // 2, mode="reflect")
    win = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT))
    out = np.empty((n_frames, n_mels), dtype=np.float64)
    bt = np.asarray(basis, dtype=np.float64).T
    for f0 in range(0, n_frames, 4096):  # in blocks: a 100 s file is 10001 frames
        f1 = min(f0 + 4096, n_frames)
        idx = (np.arange(f0, f1) * HOP)[:, None] + np.arange(N_FFT)[None, :]
        spec = np.fft.rfft(xp[idx] * win, axis=1)
        power = spec.real ** 2 + spec.imag ** 2
        out[f0:f1] = np.log10(np.maximum(power @ bt, 1e-10))
    mmax = float(out.max())
    return (np.maximum(out, mmax - 8.0) + 4.0) / 4.0, n_frames, mmax


def window_of(norm, seek):
    """[n_mels][3000] float32 window at `seek` of file_log_mel's rows, zero past the file's last frame."""
    n_frames, n_mels = norm.shape
    out = np.zeros((n_mels, WINDOW), dtype=np.float32)
    k = max(0, min(WINDOW, n_frames - seek))
    out[:, :k] = norm[seek:seek + k].T.astype(np.float32)
    return out


def make_file(demo, k):
    """Input file k = 1..5 (12 s, exactly 30 s, 45 s, 75 s, 100 s) built from the 4.2 s demo clip so that no two files and no
    two 30 s stretches are alike: pieces j = 0, 1, ... of the demo rotated by (7919 k) mod n samples, truncated to
    n - ((3 j + k) mod 4) * (n // 9) samples, times gain GAINS[(j + k) mod 5]; concatenated and cut to length."""
    demo = np.asarray(demo, dtype=np.float32)
    n = len(demo)
    rot = np.roll(demo, -((7919 * k) % n))  # rotated left: sample i is demo[(i + r) mod n]
    pieces, total, j = [], 0, 0
    while total < LENGTHS[k]:
        p = rot[: n - ((3 * j + k) % 4) * (n // 9)] * np.float32(GAINS[(j + k) % 5])
        pieces.append(p)
        total += len(p)
        j += 1
    return np.ascontiguousarray(np.concatenate(pieces)[: LENGTHS[k]], dtype=np.float32)
