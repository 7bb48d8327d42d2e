"""CPU: the float64 reference of the FP8 cross K/V format (tests/cross_fp8_reference.py) against independent statements of the same
things — torch's float8_e4m3fn for the code table and the rounding, the header's own index functions and scale rule (printed by
tests/cpp/cross_fp8_layout_tables.cpp), the definition of the scale for the quantiser — and a proof that the attention comparison
the GPU tests make is sharp: every way of reading the format wrongly moves the float64 result by at least 8x the largest bound."""
import os
import subprocess

import numpy as np
import pytest
import torch

import cross_fp8_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bf16(x):
    return torch.tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


def torch_codes(y):
    return torch.tensor(np.asarray(y, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ------------------------------------------------------------------ codes
def test_code_table_against_torch():
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    nan = np.isnan(R.TABLE)
    assert np.nonzero(nan)[0].tolist() == [0x7F, 0xFF] and np.array_equal(nan, np.isnan(t))
    assert np.array_equal(R.TABLE[~nan], t[~nan]) and np.array_equal(np.signbit(R.TABLE), np.signbit(t))
    assert R.TABLE[0x7E] == 448.0 and R.TABLE[0x01] == 2.0 ** -9 and R.TABLE[0x08] == 2.0 ** -6


def test_encode_is_round_to_nearest_even_like_torch():
    rng = np.random.default_rng(1)
    vals = R.TABLE[:0x7F]
    mids = (vals[:-1] + vals[1:]) / 2  # every exact tie between neighbouring codes, subnormal ones included
    y = np.concatenate([vals, mids, np.nextafter(mids.astype(np.float32), np.float32(0)), np.nextafter(mids.astype(np.float32), np.float32(1e9)),
                        rng.uniform(0, 448, 4000), rng.uniform(0, 2.0 ** -5, 2000), [0.0, 448.0, 2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -10]])
    y = np.concatenate([y, -y]).astype(np.float32).astype(np.float64)
    got = R.encode(y)
    assert np.array_equal(got, torch_codes(y))
    assert np.array_equal(R.encode(mids) & 1, np.zeros(mids.size, dtype=np.uint8))  # a tie goes to the even code
    assert R.encode(np.array([-0.0]))[0] == 0x80 and R.encode(np.array([-(2.0 ** -11)]))[0] == 0x80 and R.encode(np.array([2.0 ** -10]))[0] == 0x00


# ------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("narrow", [bf16, f16], ids=["bf16", "fp16"])
def test_quantiser_definition(narrow):
    rng = np.random.default_rng(2)
    n, pad = 100, 128
    x = np.zeros((pad, 64))
    x[:n] = R.channel_families(rng, n, narrow)
    x[n:] = 1e4  # pad rows hold anything: they take no part in amax and come out as code 0
    codes, e = R.quantize(x, n_keys=n)
    amax = np.abs(x[:n]).max(0)
    assert e[1] == 0 and not codes[:, 1].any()
    nz = amax > 0
    assert (amax[nz] * np.exp2(-e[nz].astype(float)) <= 448).all() and (amax[nz] * np.exp2(-(e[nz] - 1.0)) > 448).all()  # the smallest such e
    assert e[7] == 0 and e[8] == 1 and e[5] == -1 and e[6] == 0 and e[3] > e[0] + 3 and e[4] < e[0] - 10
    assert not codes[n:].any()
    assert (codes[:n, 2] & 0x80).all()
    # exactness: x * 2^-e is representable in fp32, and the code is torch's rounding of it
    y = x[:n] * np.exp2(-e.astype(float))
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    assert np.array_equal(codes[:n], torch_codes(y))
    assert ((codes[:n, 6] & 0x7F) < 0x08).sum() > n // 2  # subnormal codes are exercised
    ay = np.abs(y[:, 5])  # integers: in [16, 32) the code spacing is 2, so the odd ones are exact ties
    assert ((ay >= 16) & (ay < 32) & (ay % 2 == 1)).sum() >= 2
    # the error of a stored value: half a code spacing, relative 2^-4 in the normal range
    d = R.dequantize(codes[:n], R.scales_of(e))
    normal = np.abs(y) >= 2.0 ** -6
    assert (np.abs(d - x[:n])[normal] <= np.abs(x[:n])[normal] * 2.0 ** -4).all()
    assert (np.abs(d - x[:n])[~normal] <= 2.0 ** -10 * np.exp2(e.astype(float))[None].repeat(n, 0)[~normal]).all()


def test_scale_exponent_limits():
    assert R.scale_exponent(0.0) == 0 and R.scale_exponent(1e-45) == R.E_MIN and R.scale_exponent(3.4e38) == R.E_MAX
    assert R.scale_exponent(448.0) == 0 and R.scale_exponent(np.nextafter(np.float32(448), np.float32(1e9))) == 1 and R.scale_exponent(224.0) == -1


# ------------------------------------------------------------------ the header's own functions
@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = tmp_path_factory.mktemp("layout8") / "cross_fp8_layout_tables"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "whisper.axera_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "cross_fp8_layout_tables.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in out.splitlines()}


def test_index_maps_against_the_header(tables):
    KEYS, L, SLOTS, H = 192, 2, 3, 3
    key, dim = np.meshgrid(np.arange(KEYS), np.arange(64), indexing="ij")
    assert np.array_equal(tables["k8"], R.k8_index(key, dim).ravel())
    assert np.array_equal(tables["v8"], R.v8_index(key, dim).ravel())
    assert sorted(tables["k8"].tolist()) == list(range(KEYS * 64))  # a bijection onto the image
    b, i, r = np.meshgrid(np.arange(KEYS // 64), np.arange(4), np.arange(64), indexing="ij")
    assert np.array_equal(tables["k8_chunk"], R.k8_index(b * 64 + r, i * 16).ravel())
    assert (tables["k8_chunk"] % 16 == 0).all()
    idx = np.meshgrid(np.arange(L), np.arange(SLOTS), np.arange(H), np.arange(2), np.arange(64), indexing="ij")
    assert np.array_equal(tables["scale"], R.scale_index(*idx, SLOTS, H).ravel())
    assert tables["sizes"].tolist() == [KEYS * 64, L * SLOTS * H * 128, 4096, 1024, 128, R.E_MIN, R.E_MAX]


def test_scale_rule_against_the_header(tables):
    pairs = tables["exponent"].reshape(-1, 2)
    for bits, e in pairs:
        amax = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
        assert R.scale_exponent(amax) == e, (amax, e)
    want = np.exp2(np.arange(R.E_MIN, 128, dtype=np.float64)).astype(np.float32).view(np.uint32)
    assert np.array_equal(tables["pow2"], want)


# ------------------------------------------------------------------ the attention comparison bites
def test_every_misreading_moves_the_result_by_8_bounds():
    """Three clips of 1500 keys in 24 blocks, V eight times K's magnitude, the clips' magnitudes a factor 4 apart, the bytes beyond the
    keys finite garbage: the float64 result of the correct reading against the result of each wrong one."""
    rng = np.random.default_rng(3)
    n, cap = 1500, 24
    clips = []
    for c in range(3):
        k = bf16(rng.standard_normal((n, 64)) * 4.0 ** c * (1 + rng.integers(0, 3, 64)))
        v = bf16(rng.standard_normal((n, 64)) * 8 * 4.0 ** c * (1 + rng.integers(0, 3, 64)))
        kc, ke = R.quantize(k)
        vc, ve = R.quantize(v)
        clips.append((kc, vc, R.scales_of(ke).astype(np.float64), R.scales_of(ve).astype(np.float64)))
    kc, vc, ks, vs = clips[1]
    q = rng.standard_normal(64) / 4.0
    o, e = R.attn_expect(q, np.zeros(64), kc, vc, ks, vs, cap, 1)
    bound = e.max()
    print(f"largest bound {bound:.3e}, |o| up to {np.abs(o).max():.3e}")

    def moved(kc2, vc2, ks2, vs2):
        o2, _ = R.attn_expect(q, np.zeros(64), kc2, vc2, ks2, vs2, cap, 1)
        return np.abs(o2 - o).max() / bound

    # what a pad row holds in the kernel tests (finite garbage): the largest codes, K's with the signs of the query
    garbage_k, garbage_v = np.where(q > 0, 0x7E, 0xFE).astype(np.uint8)[None], np.full((1, 64), 0x7E, dtype=np.uint8)
    swapped = kc.copy()
    swapped[:, 0:16], swapped[:, 16:32] = kc[:, 16:32], kc[:, 0:16]
    cases = {
        "K exponents off by one": moved(kc, vc, ks * 2, vs),
        "V exponents off by one": moved(kc, vc, ks, vs * 2),
        "one V exponent off by one": moved(kc, vc, ks, np.where(np.arange(64) == int(np.abs(o).argmax()), vs / 2, vs)),
        "a neighbouring clip's scales": moved(kc, vc, clips[2][2], clips[2][3]),
        "K scales used for V": moved(kc, vc, ks, ks),
        "two swapped 16-byte chunks": moved(swapped, vc, ks, vs),
        "one pad row taken as a key": moved(np.concatenate([kc, garbage_k]), np.concatenate([vc, garbage_v]), ks, vs),
    }
    for what, w in cases.items():
        print(f"{what}: {w:.1f} bounds")
    assert min(cases.values()) >= 8, cases
    # and the chain length is the kernel's: two blocks per iteration
    assert R.attn_chain(24, 1) == 6 and R.attn_chain(24, 6) == 11 and R.attn_chain(2, 1) == 4
