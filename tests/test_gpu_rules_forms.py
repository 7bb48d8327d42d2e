"""GPU: the four forms of the timestamp rules agree (whisper.axera_amd/csrc/decode_rules.hpp) — one table of rows and histories through
apply_timestamp_rules, score_timestamp_rules, sample_timestamp_rules and beam_candidates on the micro model.

The unscored, scored and sampled-at-temperature-0 decisions are equal, the first beam candidate is that decision, the scored and
sampled-at-0 log-probabilities are bit-equal, and the first candidate's log-probability is within test_gpu_beam.py's bar of the
scored one (the beam kernel adds the timestamps in chunks of four, the rules kernels one by one: other rounding, not other rules).
The table sits where a shared chunk loop can go wrong; what a row claims about itself is checked against tests/ts_reference.py."""
import math

import numpy as np
import pytest

import ts_reference as tsr

pytestmark = pytest.mark.gpu

SEED = 1234


def _bar(xc, lse):  # test_gpu_beam.py's bar for a candidate's log-probability
    m = max(abs(xc) if math.isfinite(xc) else 0.0, abs(lse) if math.isfinite(lse) else 0.0)
    return 1e-4 + 1e-6 * m


def _table(nv, T, E):
    """(name, row, history). Built once, never changed."""
    assert T % 4 == 0 and E % 4 == 1 and nv - 1 == T + 1500  # what the names below say about chunks of four ids
    rng = np.random.default_rng(7)
    rand = lambda std=3.0: (rng.standard_normal(nv) * std).astype(np.float32)
    flat = lambda v=-10.0: np.full(nv, v, dtype=np.float32)
    out = [(name, x, seq) for name, x, seq, _ in tsr.crafted_cases(nv)]
    # histories of length 0 (timestamps [T, T + 51) alone) and 1
    x = rand(); x[T + 51] = 60.0; x[T + 50] = 20.0; x[11] = 70.0
    out.append(("empty_history", x, []))
    out.append(("one_text_id", rand(), [5]))
    out.append(("one_timestamp", rand(), [T + 2]))
    # an open pair and a pair just closed; text off with only eot on: the text loop starts at E, in the chunk of E - 1
    x = rand(); x[E - 1] = 80.0
    out.append(("open_pair_text_off_loud_neighbour_of_eot", x, [T, 5, T + 10]))
    x = rand(); x[E - 1] = 80.0; x[E] = 40.0
    out.append(("open_pair_eot_wins", x, [T, 5, T + 10]))
    out.append(("closed_pair", rand(), [T, 5, T + 30, T + 30]))
    # the first allowed timestamp at every residue mod 4
    for k in range(4):
        x = rand(); x[T + k] = 50.0 - k
        out.append(("ts_lo_residue_%d" % ((k + 1) % 4), x, [T + k, 5]))
    # no timestamp left (ts_lo == ts_hi), and the vocabulary's last id as the only one, with text and without
    x = rand(); x[nv - 1] = 90.0
    out.append(("ts_range_empty_after_30s", x, [T + 1500, 5]))
    x = rand(); x[nv - 1] = 90.0; x[nv - 2] = 95.0
    out.append(("only_last_id_with_text", x, [T + 1499, 5]))
    out.append(("only_last_id_open_pair", x.copy(), [T, 5, T + 1500]))
    # rule 5 and a near miss: a hundred timestamps at 0 (logsumexp 4.6058 with the floor's share) against one text id
    for name, v in (("rule5_fires", 4.60), ("rule5_near_miss", 4.61)):
        x = flat(); x[T + 1:T + 101] = 0.0; x[7] = v
        out.append((name, x, [T, 5]))
    # NaN where the maximum would be, in both ranges
    x = rand(); x[int(np.argmax(x[:E]))] = np.nan; x[T + int(np.argmax(x[T:]))] = np.nan; x[E] = np.nan
    out.append(("nan_at_the_maxima", x, [T, 5, 9]))
    # nothing finite
    out.append(("all_nan_after_text", flat(np.nan), [T, 5]))
    out.append(("all_minus_inf_empty_history", flat(-np.inf), []))
    return out


@pytest.fixture(scope="module")
def forms(built_lib, micro_case):
    e = built_lib.Whisper("micro", micro_case.root, "zh", device=0, max_batch=48)
    T, E, nv = e.timestamp_begin, e.eot, e.n_vocab
    rows = _table(nv, T, E)
    logits = np.stack([r[1] for r in rows])
    hists = [r[2] for r in rows]
    B = len(rows)
    out = dict(T=T, E=E, nv=nv, rows=rows, logits=logits, hists=hists)
    out["plain"] = e.apply_timestamp_rules(logits, hists)
    out["scored"], out["scored_lp"] = e.score_timestamp_rules(logits, hists)
    out["sampled0"], out["sampled0_lp"] = e.sample_timestamp_rules(logits, hists, 0.0, list(range(B)), SEED)
    out["temps"] = [(0.0, 0.7, 1.0)[b % 3] for b in range(B)]  # a clip at 0 beside clips above 0 in one launch
    out["mixed"], out["mixed_lp"] = e.sample_timestamp_rules(logits, hists, out["temps"], list(range(B)), SEED)
    out["cand"] = {M: e.beam_candidates(logits, hists, M) for M in (1, 6)}
    e.close()
    return out


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def test_the_table_is_what_its_names_say(forms):
    T, E, nv = forms["T"], forms["E"], forms["nv"]
    by_name = {r[0]: r for r in forms["rows"]}
    first_ts = lambda name: int(np.flatnonzero(tsr.allowed(by_name[name][2], T, E, nv)[T:])[0])
    assert [first_ts("ts_lo_residue_%d" % r) % 4 for r in (1, 2, 3, 0)] == [1, 2, 3, 0]
    ok = tsr.allowed(by_name["empty_history"][2], T, E, nv)
    assert not ok[:T].any() and ok[T:T + 51].all() and not ok[T + 51:].any()
    assert not tsr.allowed(by_name["ts_range_empty_after_30s"][2], T, E, nv)[T:].any()
    for name, text in (("only_last_id_with_text", True), ("only_last_id_open_pair", False)):
        ok = tsr.allowed(by_name[name][2], T, E, nv)
        assert np.flatnonzero(ok[T:]).tolist() == [1500] and ok[:E].all() == text and ok[:E].any() == text and ok[E]
    ok = tsr.allowed(by_name["open_pair_eot_wins"][2], T, E, nv)
    assert not ok[:E].any() and ok[E]
    fires = {name: tsr.decide(by_name[name][1], by_name[name][2], T, E)[1] for name in ("rule5_fires", "rule5_near_miss")}
    assert fires["rule5_fires"]["rule5"] and not fires["rule5_near_miss"]["rule5"]
    assert all(abs(i["lse"] - i["max_text"]) < 0.01 for i in fires.values())


def test_decisions_are_equal_in_every_form(forms):
    T, E = forms["T"], forms["E"]
    names = [r[0] for r in forms["rows"]]
    want = [tsr.decide(x, seq, T, E)[0] for _, x, seq in forms["rows"]]
    assert forms["plain"] == want, [(n, g, w) for n, g, w in zip(names, forms["plain"], want) if g != w]  # (no near tie in this table)
    assert forms["scored"] == forms["plain"]
    assert forms["sampled0"] == forms["plain"]
    for M, (cid, clp, nc) in forms["cand"].items():
        assert cid[:, 0].tolist() == forms["plain"], (M, [(n, int(g), w) for n, g, w in zip(names, cid[:, 0], want) if g != w])
    # nothing finite: eot, with -inf, and no candidate
    for name in ("all_nan_after_text", "all_minus_inf_empty_history"):
        b = names.index(name)
        assert forms["plain"][b] == E and forms["scored_lp"][b] == -np.inf and forms["cand"][6][2][b] == 0


def test_log_probabilities_agree(forms):
    assert _bits(forms["sampled0_lp"]) == _bits(forms["scored_lp"])
    for M, (cid, clp, nc) in forms["cand"].items():
        for b, (name, x, seq) in enumerate(forms["rows"]):
            want, got = float(forms["scored_lp"][b]), float(clp[b, 0])
            if not math.isfinite(want) or not math.isfinite(got):
                assert got == want, (M, name, got, want)
                continue
            xc = float(x[forms["scored"][b]])
            assert abs(got - want) <= _bar(xc, xc - want), (M, name, got, want)


def test_a_clip_at_zero_beside_clips_that_draw(forms):
    T, E, nv = forms["T"], forms["E"], forms["nv"]
    drew_another = 0
    for b, (name, x, seq) in enumerate(forms["rows"]):
        g, lp = forms["mixed"][b], forms["mixed_lp"][b]
        if forms["temps"][b] == 0.0:
            assert g == forms["scored"][b] and _bits([lp]) == _bits([forms["scored_lp"][b]]), (name, g, float(lp))
            continue
        # a draw: an id of the final allowed set (or eot where that is empty), scored under the untempered set
        _, info = tsr.decide(x, seq, T, E)
        ok = tsr.allowed(seq, T, E, nv) & ~np.isnan(x) & (x > -np.inf)
        if info["rule5"]:
            ok[:T] = False
        assert ok[g] if ok.any() else g == E, (name, g)
        drew_another += g != forms["scored"][b]
        if ok.any() and math.isfinite(float(forms["scored_lp"][b])):
            want = float(forms["scored_lp"][b]) + float(x[g]) - float(x[forms["scored"][b]])  # the same logsumexp under another id
            assert abs(float(lp) - want) <= _bar(float(x[g]), float(x[g]) - want), (name, g, float(lp), want)
    assert drew_another > 0
