"""Python statement of "Language and task per clip" (DESIGN.md): the language set, the detection rule, the per-clip context, and
LangCase — a test model whose detected language depends on the audio.

The engine (whisper.axera_amd/csrc/decode_language.hip, engine_prefill.cpp) is checked against this file.

Language set: the config's all_language_tokens / all_language_codes in file order; index j means lang_tokens[j].
Detection (openai-whisper's detect_language): context [sot] alone at position 0, the clip's own cross K/V, x the logits row of that
position. lang_logit[j] = x[lang_tokens[j]]; lang_logprob[j] = lang_logit[j] - logsumexp_j(lang_logit), natural log, float32 out, NaN
entries left out of the sum and given -inf; the detected index is the first maximum in file order, NaN never wins; nothing finite:
the handle's language, every lang_logprob -inf.
Request: lang[b] >= 0 an index, -1 the handle's language, -2 detect; task[b] 0 transcribe, 1 translate.
Context: a clip needs one if it has a prompt, or its language resolves to another than the handle's, or its task is not transcribe,
or it detects: ([sot_prev, the last 223 prompt ids] if prompted) + [sot, language], handed over at offset L (2, or P + 3) with the
task id as the token about to be fed."""
import numpy as np

import modelgen
import oracle
from eot_case import _round16, eot_clips

KEEP = 223
MARGIN = 0.5  # the decision margin (best language logit minus the second best) a LangCase clip must have to be kept
N_CLIPS = 16
MODELS = (("micro", 11, "BF16"), ("miniturbo", 21, "F16"))
K = 8  # residual coordinates set aside for the language signal


def lang_tokens(cfg):
    return [int(t) for t in cfg["all_language_tokens"].split(",")]


def lang_codes(cfg):
    return cfg["all_language_codes"].split(",")


def pick(lang_logit, handle_index):
    """(index, lang_logprob float32 [n_lang]) of one row of language logits."""
    x = np.asarray(lang_logit, dtype=np.float32)
    ok = ~np.isnan(x)
    if not np.isfinite(x).any():
        return int(handle_index), np.full(x.shape, -np.inf, dtype=np.float32)
    x64 = x.astype(np.float64)
    m = x64[ok].max()
    index = int(np.nonzero(ok & (x64 == m))[0][0])
    if m == np.inf:
        lp = np.where(ok & (x64 == np.inf), 0.0, -np.inf)
    else:
        lse = m + np.log(np.exp(x64[ok] - m).sum())
        lp = np.where(ok, x64 - lse, -np.inf)
    return index, lp.astype(np.float32)


def detect(orc, ck, cv, handle_index=None):
    """(index, lang_logprob, lang_logit) of the oracle on one clip's cross K/V."""
    cfg = orc.cfg
    sk, sv = orc.new_self_cache()
    x = orc.decoder_step(int(cfg["sot"]), 0, ck, cv, sk, sv, want_logits=True)
    lg = x[lang_tokens(cfg)].astype(np.float32)
    if handle_index is None:
        handle_index = lang_codes(cfg).index("zh")
    index, lp = pick(lg, handle_index)
    return index, lp, lg


def needs_context(n_prompt, lang, task, handle_index):
    return n_prompt > 0 or lang == -2 or (handle_index if lang == -1 else lang) != handle_index or task != 0


def context(cfg, prompt, lang_index, task):
    """The ids of a clip that needs a context, the task id last: ([sot_prev, the last KEEP prompt ids]) + [sot, language, task]. The
    engine caches all but the last and hands the clip over at offset L = len - 1 with the last one about to be fed."""
    prompt = [int(t) for t in prompt][-KEEP:]
    head = [int(cfg["sot_prev"])] + prompt if prompt else []
    return head + [int(cfg["sot"]), lang_tokens(cfg)[lang_index], int(cfg["translate"] if task else cfg["transcribe"])]


class LangCase:
    """modelgen.synth_weights shaped so that the language logits depend on the audio: K residual coordinates reach no logit but the
    languages' (their embedding columns are zero for every id, every language row is zero outside them), the cross-attention output
    projections feed those coordinates 64 times harder, the final LayerNorm's bias centres them over the probe clips, and language
    row j holds 16 N(0, 1) on them."""

    def __init__(self, model_type, seed, dtype):
        self.model_type, self.seed, self.dtype = model_type, seed, dtype
        self.dims = modelgen.DIMS[model_type]
        self.cfg = modelgen.make_config(model_type, self.dims)
        self.policy = 2 if dtype == "F16" else True
        self.tokens = lang_tokens(self.cfg)
        self.codes = lang_codes(self.cfg)
        self.n_lang = len(self.tokens)
        self.handle_index = self.codes.index("zh")
        w = dict(modelgen.synth_weights(self.dims, seed, bf16=(dtype != "F16")))
        if dtype == "F16":
            w = {k: v.astype(np.float16).astype(np.float32) for k, v in w.items()}
        for l in range(self.dims["dec_layers"]):
            o = w[f"decoder.blocks.{l}.cross_attn.out.weight"].copy()
            o[:K] *= np.float32(64.0)
            w[f"decoder.blocks.{l}.cross_attn.out.weight"] = o
        emb = w["decoder.token_embedding.weight"].copy()
        emb[:, :K] = 0.0
        lb = w["decoder.ln.bias"].copy()
        lb[:K] = 0.0
        # probe: language j < K reads coordinate j alone through a 2^-6 entry
        pemb = emb.copy()
        for j in range(K):
            pemb[self.tokens[j]] = 0.0
            pemb[self.tokens[j], j] = 2.0 ** -6
        probe = dict(w)
        probe["decoder.token_embedding.weight"] = pemb
        probe["decoder.ln.bias"] = lb
        orc = oracle.Oracle(self.cfg, probe, bf16_policy=self.policy)
        vals = []
        for c in eot_clips(K):
            mel, _, _ = oracle.log_mel(c, self.dims["n_mels"])
            ck, cv = orc.encoder(mel)
            vals.append(detect(orc, ck, cv, self.handle_index)[2][:K].astype(np.float64) * 64.0)
        del orc
        lb[:K] = _round16(-np.mean(vals, axis=0), dtype)
        rows = _round16(16.0 * np.random.default_rng(seed).standard_normal((self.n_lang, K)), dtype)
        for j in range(self.n_lang):
            emb[self.tokens[j]] = 0.0
            emb[self.tokens[j], :K] = rows[j]
        w["decoder.token_embedding.weight"] = emb
        w["decoder.ln.bias"] = lb
        self.weights = w
        self.oracle = oracle.Oracle(self.cfg, w, bf16_policy=self.policy)
        self._clips = None
        self._expect = {}

    def clips(self):
        if self._clips is None:
            self._clips = eot_clips(N_CLIPS)
        return self._clips

    def encode(self, i):
        mel, _, _ = oracle.log_mel(self.clips()[i], self.dims["n_mels"])
        return mel, self.oracle.encoder(mel)

    def expect(self, i):
        """dict(index, lang_logprob, lang_logit, margin, mel, ck, cv) of the oracle on clip i, computed once."""
        if i not in self._expect:
            mel, (ck, cv) = self.encode(i)
            index, lp, lg = detect(self.oracle, ck, cv, self.handle_index)
            top = np.sort(lg)
            self._expect[i] = dict(index=index, lang_logprob=lp, lang_logit=lg, margin=float(top[-1] - top[-2]), mel=mel, ck=ck, cv=cv)
        return self._expect[i]

    def kept(self):
        """The clips whose oracle decision keeps MARGIN."""
        return [i for i in range(N_CLIPS) if self.expect(i)["margin"] >= MARGIN]

    def write(self, root):
        import os

        modelgen.write_model_dir(str(root), self.model_type, self.dims, weights=self.weights, dtype=self.dtype,
                                 tiktoken_path=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multilingual.tiktoken"))
        return str(root)
