"""GPU: the two kernels of csrc/cross_kv_fp8.hip alone, through tests/cpp/cross_fp8_driver.cpp linked against the shipped objects, one
driver process per test, both dtype builds.

  cross_kv_quantize_kernel            codes and scales bit-equal to tests/cross_fp8_reference.quantize: no tolerance, no exemption
                                      (the power-of-two scale makes x * 2^-e exact; the code is one round-to-nearest-even)
  decode_cross_attention_fp8_kernel   the whole output pair against float64 (decode_kernel_reference.softmax_expect on the code
                                      values, chain length cross_fp8_reference.attn_chain) within the derived bound; what the launch
                                      does not write keeps its sentinel
"""
import os
import subprocess

import numpy as np
import pytest

import cross_fp8_reference as R
from decode_kernel_reference import (GUARD, SCORE_FAMILIES, SENT16, PairExpect, attn_qkv, check_pair, f32_slack, frag_index, ln_rows, pair_err,
                                     query_expect, realistic_stream, round16, sentinel, to_bits, typed, weights)
from kernel_driver import DTYPES, driver_exe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=DTYPES)
def driver(request):
    return request.param, driver_exe(request.param, "cross_fp8_driver.cpp", linked=("cross_kv_fp8",))


def run(driver, tmp_path, bufs, launches, timeout=120):
    """One driver process: bufs {name: array}, launches [(cmd, id, {key: value}, [buffers to dump])] -> per launch {name: bytes with guards}."""
    _, exe = driver
    lines = []
    for name, content in bufs.items():
        f = os.path.join(tmp_path, f"in.{name}.bin")
        np.ascontiguousarray(content).tofile(f)
        lines.append(f"alloc {name} {np.ascontiguousarray(content).nbytes} {f}")
    for li, (cmd, ident, p, outs) in enumerate(launches):
        lines.append(f"{cmd} {ident} " + " ".join(f"{k}={v}" for k, v in p.items()))
        lines += [f"dump {o} {os.path.join(tmp_path, f'l{li}.{o}')}" for o in outs]
    mf = os.path.join(tmp_path, "manifest.txt")
    with open(mf, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, mf], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), f"driver exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
    grids = {ln.split()[1]: tuple(int(v) for v in ln.split()[2:5]) for ln in r.stdout.splitlines() if ln.startswith("ran ")}
    got = []
    for li, (cmd, ident, p, outs) in enumerate(launches):
        got.append({o: np.fromfile(os.path.join(tmp_path, f"l{li}.{o}"), dtype=np.uint8) for o in outs})
    return grids, got


def inner(dump):
    """a dump without its guards, which must still hold the sentinel"""
    g = np.frombuffer(np.array([SENT16], dtype=np.uint16).tobytes() * (GUARD // 2), dtype=np.uint8)
    assert np.array_equal(dump[:GUARD], g) and np.array_equal(dump[-GUARD:], g), "store into a guard"
    return dump[GUARD:-GUARD]


# ------------------------------------------------------------------ quantise
def k16_index(key, dim):
    """the h16 blocked K [key / 64][dim / 8][key % 64][8] (decode_layout.hpp k_index)"""
    return (key >> 6) * 4096 + (dim >> 3) * 512 + (key & 63) * 8 + (dim & 7)


def quant_case(dt, seed, L, S, H, n_keys, keys_pad):
    """natural [L][S][H][keys_pad][64] K and V of the 16-bit type: the channel families of the CPU test dealt over the heads, rows
    beyond the keys large finite garbage (they must neither move a scale nor leave a non-zero code)."""
    rng = np.random.default_rng(seed)
    nat = []
    for _ in range(2):
        x = rng.uniform(-3e4, 3e4, (L, S, H, keys_pad, 64))
        for l in range(L):
            for s in range(S):
                for h in range(H):
                    x[l, s, h, :n_keys] = R.channel_families(rng, n_keys, lambda a: a) * 4.0 ** ((l + s + h) % 3 - 1) if n_keys >= 9 else rng.standard_normal((n_keys, 64))
        nat.append(round16(x, dt).astype(np.float64))
    return nat


def quant_images(nat, dt, keys_pad):
    key, dim = np.meshgrid(np.arange(keys_pad), np.arange(64), indexing="ij")
    k = np.zeros(nat[0].shape[:3] + (keys_pad * 64,), dtype=np.uint16)
    k[..., k16_index(key, dim).ravel()] = to_bits(nat[0], dt).reshape(nat[0].shape[:3] + (-1,))
    return k.ravel(), to_bits(nat[1], dt).ravel()


def quant_expect(nat, n_keys, keys_pad, slots, sent8):
    """(k8, v8, scales as uint8 bytes) with the slots in `slots` written and the others at the sentinel"""
    L, S, H = nat[0].shape[:3]
    key, dim = np.meshgrid(np.arange(keys_pad), np.arange(64), indexing="ij")
    k8 = np.tile(sent8, L * S * H * keys_pad * 64 // 2).reshape(L, S, H, keys_pad * 64).copy()
    v8 = k8.copy()
    sc = np.tile(sent8, L * S * H * 128 * 2).reshape(L, S, H, 2, 64 * 4).copy()
    for s in slots:
        ck, ek = R.quantize(nat[0][:, s], n_keys)
        cv, ev = R.quantize(nat[1][:, s], n_keys)
        k8[:, s][..., R.k8_index(key, dim).ravel()] = ck.reshape(L, H, -1)
        v8[:, s] = cv.reshape(L, H, -1)
        sc[:, s, :, 0] = R.scales_of(ek).view(np.uint8).reshape(L, H, 256)
        sc[:, s, :, 1] = R.scales_of(ev).view(np.uint8).reshape(L, H, 256)
    return k8.ravel(), v8.ravel(), sc.ravel()


@pytest.mark.parametrize("n_keys,keys_pad", [(1500, 1536), (100, 128)])
def test_quantise_kernel_bit_exact(driver, tmp_path, n_keys, keys_pad):
    dt, _ = driver
    L, S, H = 2, 3, 3
    nat = quant_case(dt, 7 + n_keys, L, S, H, n_keys, keys_pad)
    k, v = quant_images(nat, dt, keys_pad)
    n8 = L * S * H * keys_pad * 64
    bufs = dict(k=k, v=v, k8=sentinel(n8, 1), v8=sentinel(n8, 1), sc=sentinel(L * S * H * 128, 4), k8m=sentinel(n8, 1), v8m=sentinel(n8, 1),
                scm=sentinel(L * S * H * 128, 4), map=np.array([2, 0], dtype=np.int32))
    p = dict(n_layer=L, n_slots=S, n_head=H, n_keys=n_keys, keys_pad=keys_pad, k="k", v="v")
    launches = [("quant", "all", dict(p, clips=S, k8="k8", v8="v8", scales="sc"), ["k8", "v8", "sc"]),
                ("quant", "mapped", dict(p, clips=2, k8="k8m", v8="v8m", scales="scm", slot_map="map"), ["k8m", "v8m", "scm"])]
    grids, got = run(driver, str(tmp_path), bufs, launches)
    assert grids == {"all": (2 * H, S, L), "mapped": (2 * H, 2, L)}
    sent8 = np.array([SENT16], dtype=np.uint16).view(np.uint8)
    for (names, slots), g in zip(((("k8", "v8", "sc"), (0, 1, 2)), (("k8m", "v8m", "scm"), (2, 0))), got):  # slot 1 of the mapped run keeps the sentinel
        for name, want in zip(names, quant_expect(nat, n_keys, keys_pad, slots, sent8)):
            have = inner(g[name])
            assert np.array_equal(have, want), (dt, name, slots, int((have != want).sum()), int(np.nonzero(have != want)[0][0]))


# ------------------------------------------------------------------ attention
def attn_inputs(dt, seed, mode, B, H, cap, n_keys, nan_pad):
    """Buffers and keys of one launch's inputs, and per (clip, head) the codes and scales the reference attends over. Bytes beyond
    the keys: NaN codes, or the largest finite codes (K's with the signs that would win the softmax)."""
    rng = np.random.default_rng(seed)
    d = H * 64
    b, p = {}, dict(batch=B, n_head=H, d_model=d, n_keys=n_keys, cap_blocks=cap)
    q = np.zeros((B, d), np.float32)
    head_bytes = cap * 4096
    k8, v8 = np.zeros((B, H, head_bytes), np.uint8), np.zeros((B, H, head_bytes), np.uint8)
    sc = np.zeros((B, H, 2, 64), np.float32)
    codes = {}
    for c in range(B):
        for h in range(H):
            fam = SCORE_FAMILIES[(c * H + h + seed) % len(SCORE_FAMILIES)] if mode == "q" else "flat"
            qq, kn, vn = attn_qkv(rng, n_keys, dt, fam)
            q[c, h * 64:h * 64 + 64] = qq / np.float32(4.0 ** ((c + h) % 3))  # (the family's scores, whatever K's magnitude)
            kn = kn * 4.0 ** ((c + h) % 3)  # scales that differ between clips, heads and K / V
            vn = vn * 8.0 * 4.0 ** ((c + 2 * h) % 3)
            kc, ke = R.quantize(round16(kn, dt))
            vc, ve = R.quantize(round16(vn, dt))
            sc[c, h, 0], sc[c, h, 1] = R.scales_of(ke), R.scales_of(ve)
            codes[c, h] = (kc, vc)
            gk = 0x7F if nan_pad else np.where(qq > 0, 0x7E, 0xFE).astype(np.uint8)
            kimg = np.full((cap * 64, 64), 0, np.uint8)
            kimg[:] = gk
            kimg[:n_keys] = kc
            key, dim = np.meshgrid(np.arange(cap * 64), np.arange(64), indexing="ij")
            k8[c, h][R.k8_index(key, dim).ravel()] = kimg.ravel()
            vimg = np.full((cap * 64, 64), 0xFF if nan_pad else 0x7E, np.uint8)
            vimg[:n_keys] = vc
            v8[c, h] = vimg.ravel()
    b.update(k8=k8.ravel(), v8=v8.ravel(), sc=sc.ravel())
    p.update(k8="k8", v8="v8", scales="sc", kv_batch_bytes=H * head_bytes, scale_batch_stride=H * 128)
    if mode == "q":
        b["q"], p["q"] = f32_slack(q, d), "q"
    elif mode == "fused":
        x, g, be, _ = realistic_stream(rng, B, d) if seed % 2 else (ln_rows(rng, B, d), rng.uniform(0.5, 1.5, d).astype(np.float32), rng.uniform(-1, 1, d).astype(np.float32), ())
        b.update(x=f32_slack(x, d), ln_w=g, ln_b=be, wq=to_bits(weights(rng, d, d, dt, "realistic"), dt), bq=rng.uniform(-1, 1, d).astype(np.float32))
        p.update(x="x", ln_w="ln_w", ln_b="ln_b", wq="wq", bq="bq")
    else:  # folded: T rows, the block statistics of a residual row, two constant vectors — all taken as given
        xr = ln_rows(rng, B, d).astype(np.float64).reshape(B, d // 16, 16)
        s1 = xr.sum(2)
        q2 = ((xr - s1[..., None] / 16) ** 2).sum(2)
        b.update(tq=f32_slack(rng.standard_normal((B, d)).astype(np.float32), d), stat=np.stack([s1, q2], axis=2).astype(np.float32).ravel(),
                 fold_s=rng.standard_normal(d).astype(np.float32), fold_c=rng.standard_normal(d).astype(np.float32))
        p.update(tq="tq", stat_part="stat", fold_s="fold_s", fold_c="fold_c")
    return b, p, codes, sc


def attn_check(name, dt, b, p, codes, sc, got, done, init_hi, init_lo):
    B, H, d, cap, ns, nbs = p["batch"], p["n_head"], p["d_model"], p["cap_blocks"], p["n_split"], p["nbs"]
    q, dq = query_expect(p, typed(p, b), dt)
    pe = PairExpect(init_hi.size)
    for c in range(B):
        if done[c]:
            continue
        for h in range(H):
            o, e = R.attn_expect(q[c, h * 64:h * 64 + 64], dq[c, h * 64:h * 64 + 64], codes[c, h][0], codes[c, h][1], sc[c, h, 0], sc[c, h, 1], cap, ns)
            pe.put(frag_index(c, h * 64 + np.arange(64), nbs), o, e + pair_err(np.abs(o) + e, dt))
    return check_pair(name, got["out_hi"].view(np.uint16), got["out_lo"].view(np.uint16), init_hi, init_lo, pe, dt)


ATTN_CASES = [  # (mode, n_keys, cap_blocks, n_split, done, done_late, NaN codes beyond the keys, relaunch)
    *[(m, 1500, 24, s, None, 0, (s + i) % 2 == 0, s == 3) for i, m in enumerate(("q", "fused", "folded")) for s in (1, 2, 3, 4, 6)],
    *[("q", n, 24, 1, None, 0, n % 2 == 0, False) for n in (1, 63, 64, 65, 128)],
    *[("folded", n, 4, 2, None, 1, n % 2 == 1, True) for n in (1, 63, 64, 65, 128)],
    ("q", 1500, 24, 2, (0, 1, 0), 0, True, False), ("fused", 1500, 24, 2, (0, 1, 0), 1, False, False), ("folded", 100, 2, 1, (1, 0, 0), 1, True, False),
]


def test_attention_kernel_against_float64(driver, tmp_path):
    dt, _ = driver
    B, H = 3, 3
    d, nbs = H * 64, 2
    bufs, launches, checks = {}, [], []
    for ci, (mode, n_keys, cap, ns, done, late, nan_pad, again) in enumerate(ATTN_CASES):
        b, p, codes, sc = attn_inputs(dt, 100 + ci, mode, B, H, cap, n_keys, nan_pad)
        done = np.asarray(done if done is not None else (0, 0, 0), dtype=np.int32)
        b.update(done=done, out_hi=sentinel(d // 32 * nbs * 512, 2), out_lo=sentinel(d // 32 * nbs * 512, 2))
        p.update(n_split=ns, nbs=nbs, done_late=late, done="done", out_hi="out_hi", out_lo="out_lo")
        if ns > 1:
            b.update(mpart=sentinel(B * H * ns * 66, 4), mcnt=np.zeros(B * H + 2, np.int32))
            p.update(mpart="mpart", mcnt="mcnt")
        names = {k: f"c{ci}.{k}" for k in b}
        bufs.update({names[k]: v for k, v in b.items()})
        pp = {k: (names[v] if isinstance(v, str) and v in names else v) for k, v in p.items()}
        ident = f"{mode}.keys{n_keys}.cap{cap}.s{ns}.late{late}.{'nan' if nan_pad else 'big'}"
        for rep in range(2 if again else 1):  # again: a second launch on the tickets the first one left
            launches.append(("attn8", f"{ci}.{ident}.{rep}", pp, [names["out_hi"], names["out_lo"]] + ([names["mcnt"]] if ns > 1 else [])))
            checks.append((ident + (".again" if rep else ""), b, p, codes, sc, done, names))
    grids, got = run(driver, str(tmp_path), bufs, launches, timeout=300)
    worst = {}
    for (cmd, lid, pp, outs), (ident, b, p, codes, sc, done, names), g in zip(launches, checks, got):
        assert grids[lid] == (p["n_split"], H, B), (lid, grids[lid])
        res = {k: g[names[k]] for k in ("out_hi", "out_lo")}  # (check_pair looks at the guards itself)
        w = attn_check(ident, dt, b, p, codes, sc, res, done, b["out_hi"], b["out_lo"])
        if p["n_split"] > 1:
            assert not inner(g[names["mcnt"]]).any(), (ident, "the launch leaves its tickets at zero")
        form = ident.split(".")[0]
        worst[form] = max(worst.get(form, 0.0), w)
        assert w <= 1.0, (dt, ident, w)
    for form, w in sorted(worst.items()):
        print(f"{dt} fp8 cross-attention, query mode {form}: worst error / bound {w:.4f}")
