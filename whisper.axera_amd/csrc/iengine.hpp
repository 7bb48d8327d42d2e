// iengine.hpp — the dtype-independent face of the engine, as the C ABI (api.cpp) sees it.
//
// engine.{hpp,cpp} and every kernel file are compiled twice (bfloat16 and IEEE-half storage, see common.hpp); each
// build defines axw::<ns>::Engine : IEngine and one factory below. api.cpp picks the factory from the dtype of the
// model's weights file, so one libax_whisper.so serves "Whisper-small bf16" and "Whisper-turbo fp16" alike.
#pragma once

#include <cstdint>
#include <map>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "beam.hpp"
#include "longform.hpp"

namespace axw {

struct ModelConfig {
  int n_mels = 0, n_audio_ctx = 1500, n_audio_state = 0, n_audio_head = 0, n_audio_layer = 0;
  int n_vocab = 0, n_text_ctx = 448, n_text_state = 0, n_text_head = 0, n_text_layer = 0;
  int sot = 0, eot = 0, transcribe = 0, translate = 0, no_timestamps = 0;
  std::vector<int> lang_tokens;
  std::vector<std::string> lang_codes;
  std::map<std::string, long> ints;  // every integer-valued key of the config file
};

class IEngine {
 public:
  virtual ~IEngine() {}
  // decode modes: kDecodePlain = prefix [sot, lang, transcribe, notimestamps];
  // kDecodeTimestamps = prefix [sot, lang, transcribe] and Whisper's timestamp rules at every sampled step (DESIGN.md
  // "Segment timestamps"); ids then include timestamp tokens
  // kDecodeScored = kDecodeTimestamps that also keeps, per clip, the log-probability of every decision and log p(<|nospeech|>) at
  // the step that fed sot (DESIGN.md "Confidence"); the ids are those of kDecodeTimestamps
  // kDecodeSampled = kDecodeScored whose decisions are drawn at a per-clip temperature from a per-clip random stream (DESIGN.md
  // "Temperature fallback"); a clip at temperature 0 decides as kDecodeScored does. Needs a SampleSpec.
  enum DecodeMode : int { kDecodePlain = 0, kDecodeTimestamps = 1, kDecodeScored = 2, kDecodeSampled = 3 };
  // what kDecodeSampled draws with: host temperature [batch] (>= 0, not NaN), stream [batch] (the clip's random stream: equal
  // (seed, stream, history length) give equal noise wherever the clip sits), one seed per call
  struct SampleSpec { const float* temperature; const uint64_t* stream; uint64_t seed; };
  // what kDecodeScored keeps (DESIGN.md "Confidence"); every array may be null.
  // greedy: token_logprob [batch][n_text_ctx]: entries 0 .. n_ids[b] (one per kept id + the decision that ended the clip), the
  // rest 0; avg_logprob, no_speech_logprob, ended_eot [batch]
  struct ClipScores { float *token_logprob, *avg_logprob, *no_speech_logprob; int* ended_eot; };
  // forced: logprob [batch][n_forced+1] of each step's chosen id, no_speech_logprob [batch], logits0 [batch][n_vocab]: the raw row
  // of decode offset 0
  struct ForcedScores { float *logprob, *no_speech_logprob, *logits0; };
  // prompt conditioning (DESIGN.md "Prompt conditioning"): n_prompt[b] ids of clip b at ids + b * stride (text ids below eot and
  // timestamp ids; the last n_text_ctx / 2 - 1 are used), n_prompt[b] == 0: no prompt, the clip decodes as it does without this
  struct PromptSpec { const int32_t* ids; int stride; const int* n_prompt; };
  // language and task per clip (DESIGN.md "Language and task per clip"): lang[b] >= 0 an index into the config's language list,
  // -1 the handle's language, -2 detect it from the clip; task[b] 0 transcribe, 1 translate. A null array: all -1 / all 0.
  struct LangSpec { const int* lang; const int* task; };
  // what comes back per clip; every array may be null. detected [batch]: the language index the clip was decoded under (for explicit
  // and default clips the index they were given); lang_logprob, lang_logit [batch][n_lang]: detecting clips only, the others' rows are 0
  struct LangResult { int* detected; float* lang_logprob; float* lang_logit; };
  // What stands in front of `transcribe` for the clips of one call (engine_prefill.cpp): their prompts and their language and task. Both
  // exist in the timestamp modes only; a language spec also refuses an open Stream*. lang_out is written when `lang` is present
  // (detected[b] for every clip), and only then.
  struct ClipContexts {
    std::optional<PromptSpec> prompts;
    std::optional<LangSpec> lang;
    LangResult lang_out{};
    bool any() const { return prompts || lang; }
    ClipContexts block(int lo, int n_lang) const;
  };
  // The optional parts of one decode over a batch of clips. max_new_clip: host [batch] per-clip id budgets (<= 0: none), each capped by
  // max_new; sample: kDecodeSampled, and it alone (required there); scores: kDecodeScored and kDecodeSampled only.
  struct DecodeRequest {
    DecodeMode mode = kDecodePlain;
    int max_new = 0;
    const int* max_new_clip = nullptr;
    // host [batch] sample rates of the clips in Hz (DESIGN.md "Sample rates"), null: every clip is 16000 Hz. A clip at another rate is
    // resampled on the GPU between its upload and the front-end; a rate resample.hpp refuses fails the call before any GPU work
    const int* sample_rate = nullptr;
    std::optional<SampleSpec> sample;
    ClipContexts ctx;
    std::optional<ClipScores> scores;
    // THE block rule of a batch split over devices (multi_device.hpp): the same request for the clips from `lo` on. Every per-clip
    // array that is not null (the sample rates among them) moves to its entry of clip lo: token_logprob by rows of n_ctx, the prompt ids by rows of their stride,
    // lang_logprob and lang_logit by rows of n_lang, every other array by one entry per clip.
    DecodeRequest block(int lo, int n_ctx, int n_lang) const;
  };
  // full path, host PCM or device PCM; ids [batch][n_text_ctx], n_ids [batch]. A request with contexts fails on a bad prompt, language
  // or task before any GPU work; a language spec is not taken in kDecodeSampled.
  virtual void run_tokens(const DecodeRequest& rq, const float* const* pcm, const float* d_pcm, int d_stride, const int* n_samples, int batch,
                          int32_t* ids, int* n_ids) = 0;
  virtual std::string detokenize(const int32_t* ids, int n) const = 0;
  virtual const std::vector<std::string>& token_table() const = 0;  // the bytes of every id of the tokens file
  // detokenize + the reference's zh post-pass (Traditional -> Simplified, Whisper.cpp:231-236) when its OpenCC data files were found
  virtual std::string transcript(const int32_t* ids, int n) const = 0;
  // the text of ids decoded under language `lang` (an index of the config's list): the zh pass follows that language, not the handle's
  virtual std::string transcript_lang(const int32_t* ids, int n, int lang) const = 0;
  // stage-level
  // rate: the clip's sample rate; other than 16000 Hz the clip is resampled on the GPU first (the fused upload path)
  virtual void compute_mel(const float* pcm, int n_samples, float* mel_out, int rate = 16000) = 0;
  // the resample kernel alone on host clips (DESIGN.md "Sample rates"): out[b] (capacity out_cap[b] samples) receives the n_out[b]
  // samples of clip b at 16000 Hz; a clip at 16000 Hz is copied bit for bit. Device buffers are sized by the call.
  virtual void resample(const float* const* pcm, const int* n_samples, const int* rates, int batch, float* const* out, const int* out_cap,
                        int* n_out) = 0;
  virtual void encode_mel(const float* mel, int batch) = 0;
  virtual void get_cross_kv(int slot, float* k_out, float* v_out) = 0;
  // FP8 cross K/V (a handle made under AX_WHISPER_CROSS_KV=fp8; throws on another): the slot's codes de-blocked to [L][n_audio_ctx][d]
  // bytes and its scales [L][H][2][64]; the quantise kernel alone on every slot of the handle
  virtual void get_cross_kv_fp8(int slot, unsigned char* k_codes, unsigned char* v_codes, float* scales) = 0;
  virtual void cross_kv_quantize() = 0;
  // the slot's self-attention cache rows [0, n_rows), de-blocked: k_out, v_out fp32 [n_text_layer][n_rows][d]
  virtual void get_self_kv(int slot, int n_rows, float* k_out, float* v_out) = 0;
  // the self-attention cache of clip `clip` (1 or 2: its position in the last multi-clip persistent launch), all 8 blocks x 64 keys
  // of every (layer, head), de-blocked: k_out, v_out fp32 [n_text_layer][512][d]. Throws where the handle holds no such cache.
  virtual void get_persistent_self_kv(int clip, float* k_out, float* v_out) = 0;
  // after encode_mel: the decode state of slots [0, batch) as a greedy loop under `ctx` finds it before its first step (reset, then the
  // clips' contexts cached and their task id about to be fed); no_speech_logprob (or null): [batch], 0 for slots without a context
  // sot_logits (or null): [batch][n_vocab], the raw row the no-speech value of a slot behind a context was taken from
  virtual void prefill_stage(int batch, const ClipContexts& ctx, float* no_speech_logprob, float* sot_logits) = 0;
  // ---- language detection (engine_prefill.cpp); refuses an open Stream*
  // front-end, encoder and detection only: out.detected [batch] (required), out.lang_logprob optional
  virtual void detect_language(const float* const* pcm, const int* n_samples, int batch, const LangResult& out) = 0;
  // after encode_mel: detection of slots [0, batch) (the decode state is reset and left reset)
  virtual void detect_language_stage(int batch, const LangResult& out) = 0;
  // the detection kernel alone on host residual rows [n][d]: lang_logprob [n][n_lang], lang_index [n], lang_logit [n][n_lang] or null
  virtual void language_logprob_rows(const float* rows, int n, float* lang_logprob, int* lang_index, float* lang_logit) = 0;
  // timestamp, scored and sampled mode: logits are the raw logits (before the rules), chosen the ids the rules choose; scores:
  // kDecodeScored and kDecodeSampled only; sample (or null): kDecodeSampled only (and required there)
  // ctx (timestamp modes): the forced ids follow each clip's own context. Under prompts alone every clip needs one; under a language
  // spec (not in kDecodeSampled) EVERY clip is handed over behind its context [.., sot, language] with its task id. Behind a context
  // no step visits decode offset 0: scores->logits0 is refused and the no-speech value is the hand-over's.
  virtual void decode_forced(DecodeMode mode, const ClipContexts& ctx, int batch, const int32_t* forced, int n_forced, float* logits,
                             int32_t* chosen, const ForcedScores* scores, const SampleSpec* sample) = 0;
  // plain or timestamp mode; max_new_clip: optional host [batch] per-clip id budgets (<= 0: none), each capped by max_new
  virtual void decode_greedy(DecodeMode mode, int batch, int max_new, const int* max_new_clip, int32_t* ids, int* n_ids) = 0;
  // the rules kernel alone on host data: logits [batch][n_vocab], hist [batch][n_text_ctx] (n_hist[b] ids each) -> chosen [batch];
  // logprob [batch] (null: the unscored kernel): the scored kernel, + the log-probability of every chosen id
  // sample != nullptr (logprob required): the sampled kernel. The sample arrays are per-slot buffers: unlike the other two forms, a
  // call with batch above the engine's current capacity grows it, which re-makes the slot buffers (the cross K/V of earlier calls is lost)
  virtual void timestamp_rules(const float* logits, const int32_t* hist, const int* n_hist, int batch, int32_t* chosen, float* logprob,
                               const SampleSpec* sample = nullptr) = 0;
  // the no-speech kernel alone: logits [batch][n_vocab] -> out [batch] = log p(<|nospeech|>) over the whole row
  virtual void no_speech_logprob(const float* logits, int batch, float* out) = 0;
  // beam search (DESIGN.md "Beam search"; beam.hpp): K = beam_size hypotheses per clip, each in a slot of its own, so clips * K
  // slots must fit the engine's capacity. out: the winner and every record of every clip (BeamResult's arrays, stride n_text_ctx).
  // trace (decode_beam only; null: none): per sampled step n < cap, over S = clips * K slots: the dumped rows [cap][S][n_vocab], the
  // candidates [cap][S][K + 1] and their counts [cap][S], and after the selection sum_logprob by rank [cap][S], rank -> slot
  // [cap][S], the reorder's source by slot [cap][S], the id written at the history's index n by slot [cap][S], pool sizes [cap][clips].
  // Every array may be null. n_steps: sampled steps the loop ran.
  // decode_beam with beam_size > 1 spreads clip c's cross K/V over slots [c K, c K + K): the encoded slots are overwritten, and a
  // further stage-level decode needs a new encode_mel.
  struct BeamTrace {
    int cap; float* rows; int32_t* cand_id; float* cand_logprob; int* n_cand; float* S; int* slot; int* src; int32_t* tok; int* pool_n;
    int n_steps;
  };
  virtual void run_beam(const float* const* pcm, const int* n_samples, int clips, int beam_size, int max_new, const BeamResult& out,
                        float* no_speech_logprob) = 0;
  virtual void decode_beam(int clips, int beam_size, int max_new, const BeamResult& out, float* no_speech_logprob, BeamTrace* trace) = 0;
  // the candidates kernel alone on host data: logits [rows][n_vocab], hist [rows][n_text_ctx] (n_hist[b] ids each) ->
  // cand_id, cand_logprob [rows][n_cand_max], n_cand [rows]
  virtual void beam_candidates(const float* logits, const int32_t* hist, const int* n_hist, int rows, int n_cand_max, int32_t* cand_id,
                               float* cand_logprob, int* n_cand) = 0;
  // the selection kernel alone on host data (common.hpp: BeamSelectParams; every pointer is host memory here, M = beam + 1):
  // S, slot, pool_*, complete are updated in place; tok, src by slot and slot_score are written; returns the clips that completed
  struct BeamSelectIO {
    int clips, beam, eot, n, stride;
    const int32_t* cand_id; const float* cand_logprob; const int* n_cand;
    const int32_t* hist;
    float* S; int* slot; int* pool_n; int32_t* pool_ids; int* pool_len; float* pool_score; int* complete;
    int32_t* tok; int* src; float* slot_score;
  };
  virtual int beam_select(const BeamSelectIO& io) = 0;
  // ---- word-level timestamps (engine_align.cpp; DESIGN.md "Word-level timestamps"); refuses an open Stream*
  // After encode_mel: the alignment of slots [0, batch). Clip b: n_ids[b] text ids (< eot) at ids + b * stride, num_frames[b] mel
  // frames of its own (it aligns against num_frames[b] / 2 encoder frames), language index lang[b] (-1 or a null array: the handle's),
  // task[b] (0 transcribe, 1 translate; null: 0). Out: jump [batch][stride + 1] (n_ids[b] + 1 entries: the frame at which each text
  // token and the closing eot begin), token_logprob [batch][stride] (over the ids below eot), and optionally matrix
  // [batch][m_rows][m_ld]: rows [0, n_ids[b] + 5) x frames [0, num_frames[b] / 2) of the head-averaged matrix, the rest untouched.
  // A clip without ids gets nothing. The slots' self-attention caches and nothing else of the decode state are overwritten.
  struct AlignRequest {
    int batch; const int32_t* ids; int stride; const int* n_ids; const int* num_frames; const int* lang; const int* task;
    int* jump; float* token_logprob; float* matrix; int m_rows, m_ld;
    // how token_logprob is computed: kAlignLogProbRows, the logits launch four rows at a time and one value read out of every row,
    // or kAlignLogProbFused, vocab_logprob.hip (the LayerNorm'ed row is narrowed to the 16-bit type; no logits row is written).
    // AX_WHISPER_WORD_LOGPROB=rows|fused overrides it.
    int logprob_route = 0;
  };
  enum : int { kAlignLogProbRows = 0, kAlignLogProbFused = 1 };
  virtual void align_tokens(const AlignRequest& rq) = 0;
  // the token probabilities alone on host data (tests, A/B): x fp32 [n_rows][n_text_state] final residual rows, one id in [0, eot)
  // per row -> out [n_rows] = log p(id) over the ids below eot, by `route` itself (the environment does not override it here)
  virtual void vocab_logprob_rows(const float* x, int n_rows, const int32_t* ids, float* out, int route) = 0;
  // the list of (layer, head) pairs the alignment averages over; n == 0: the default, every head of the upper half of the layers
  virtual void set_alignment_heads(const int* pairs, int n) = 0;
  // token suppression (DESIGN.md "Token suppression"): the handle's suppress set, which every timestamp-mode decode and rules entry
  // point applies; n == 0: what the config file gave. Refuses an open Stream*.
  virtual void set_suppress_tokens(const int* ids, int n) = 0;
  virtual const std::vector<int>& suppress_tokens() const = 0;  // sorted
  // One kernel of decode_align.hip alone on host data (tests). Clip c has len[c] rows and n_keys[c] frames.
  // qk_softmax: q fp32 [rows][64 n_head] (clip c at row0[c]), k fp32 [n_slots][n_head][keys_pad][64] (clip c reads slot[c]), both
  // narrowed to the 16-bit type; P [n_clips][n_align][rows_pad][f_pad] is updated in place (the kernel writes what it writes).
  // normalize: P as above, matrix [n_clips][m_rows][m_ld] updated in place. dtw: matrix -> jump [n_clips][jump_ld].
  struct AlignKernelIO {
    int n_clips; const int* len; const int* n_keys;
    const float* q; int rows, n_head; const int* row0;
    const float* k; int n_slots, keys_pad; const int* slot;
    const int* heads; int n_align;
    float* P; int rows_pad, f_pad;
    float* matrix; int m_rows, m_ld; float inv_heads;
    int* jump; int jump_ld;
  };
  virtual void align_kernel(int which, const AlignKernelIO& io) = 0;  // 0 qk_softmax, 1 normalize, 2 dtw
  // utterance slots refilled while the others decode (include/ax_whisper_api.h: AX_WHISPER_Stream*)
  // mode 0: the plain greedy decode in the handle's language; mode 1: the scored timestamp mode (DESIGN.md "Slot stream in timestamp
  // mode"): prefix [sot, language, task] per slot, ids with their timestamp tokens, scores and a language per slot. One mode per stream.
  virtual void stream_open(int n_slots, int mode = 0) = 0;
  // rates (or null: 16000 Hz): host [count], as DecodeRequest::sample_rate
  // lang, task (mode 1 only; either may be null: all -1 / all 0): host [count], as LangSpec
  virtual void stream_admit(const int* slots, const float* const* pcm, const int* n_samples, const int* max_new, int count,
                            const int* rates = nullptr, const int* lang = nullptr, const int* task = nullptr) = 0;
  virtual int stream_step(int n_steps, int* finished_slots) = 0;  // returns the number of finished slots written
  virtual void stream_collect(int slot, int32_t* ids, int* n_ids) = 0;
  // mode 1: stream_collect plus the slot's scores (token_logprob [n_text_ctx]: entries 0 .. n_ids, the rest 0; the others one value)
  // and its language (lang_logprob [n_lang]: a detecting clip's, else zeros). Every array but ids and n_ids may be null.
  struct SlotScores { float *token_logprob, *avg_logprob, *no_speech_logprob; int* ended_eot; int* lang; float* lang_logprob; };
  virtual void stream_collect_scored(int slot, int32_t* ids, int* n_ids, const SlotScores& out) = 0;
  // the stream's rules kernel alone on host data (tests): rows [n][n_vocab], off / done / detect [n], hist [n][n_text_ctx] with
  // n_hist [n], slot_ctx [n][4] (in/out), and sentinel-filled outputs that are written only where the kernel writes: chosen, logprob
  // [n] (the decision and its log-probability of a slot that samples), no_speech [n], lang_out [n], lang_logprob [n][n_lang] (all in/out)
  struct StreamRulesIO {
    int n; const float* rows; const int* off; const int* done; const int* detect; const int32_t* hist; const int* n_hist;
    int* slot_ctx; int32_t* chosen; float* logprob; float* no_speech; int* lang_out; float* lang_logprob;
  };
  virtual void stream_rules_stage(const StreamRulesIO& io) = 0;
  virtual void stream_close() = 0;
  // every 16-bit tensor the engine STORES between kernels (encoder activations of `batch` clips, cross / self K/V caches, the
  // decoder's activation pairs): non-finite count and max |x| per buffer; returns the number of buffers reported (<= n_max)
  virtual int scan_stored16(int batch, int n_max, char (*names)[32], long long* nonfinite, float* maxabs) = 0;
  // long-form (DESIGN.md "Long-form"): the whole-file front-end + the window kernel for one file -> the window at `seek`
  // (frames) in the reference layout, host [n_mels * 3000]
  virtual void compute_mel_window(const float* pcm, int n_samples, int seek, float* mel_out) = 0;
  // the seek loop over n_files files, one window of every unfinished file per pass; log: every decoded window in execution
  // order (file counts from 0 within this call). max_new: per-window id budget (<= 0: none), max_passes <= 0: until every file ends
  // opts (null: the unscored loop): the scores of every window in the log; the silent-window rule under opts' thresholds
  virtual void run_long_windows(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes,
                                const LongScoreOptions* opts, std::vector<LongWindow>& log) = 0;
  // chunked long-form (DESIGN.md "Chunked long-form"; long_cuts.hpp): the cut points are chosen before decoding (levels kernel + plan
  // kernel on the files' log-mel store), then the windows are decoded min(slots, remaining) at a time in the flat order
  // file-then-seek. One log entry per window: window_frames = advance = the window's length.
  virtual void run_long_chunked(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes, const ChunkedOptions& opts,
                                std::vector<LongWindow>& log) = 0;
  // stage level: e and s of every file, host [n_files][1 + n_samples / 160] (either may be null)
  virtual void long_frame_levels(const float* const* pcm, const int* n_samples, int n_files, int smooth, float* const* e, float* const* s) = 0;
  // stage level: front-end + levels + plan; the flat lists and, when s_out is not null, the levels the plan was made from
  virtual void long_cut_plan(const float* const* pcm, const int* n_samples, int n_files, const CutParams& cut, std::vector<int>& n_windows,
                             std::vector<int>& win_file, std::vector<int>& win_seek, std::vector<int>& win_len, float* const* s_out) = 0;
  // stage level: the plan kernel alone on a caller's levels s [content]
  virtual void long_cut_plan_from_levels(const float* s, int content, int w_min, int w_max, std::vector<CutWindow>& plan) = 0;
  // stage level: compute_mel_window for a window of `len` frames
  virtual void compute_mel_window_cut(const float* pcm, int n_samples, int seek, int len, float* mel_out) = 0;
  virtual float bench(const std::string& what, int batch, int arg, int iters) = 0;
  virtual void set_stream(void* hip_stream) = 0;
  virtual const ModelConfig& config() const = 0;
  virtual const char* dtype_name() const = 0;  // "bf16" | "fp16"

  std::mutex& mutex() { return mu_; }
  float timings[5] = {0, 0, 0, 0, 0};

 protected:
  std::mutex mu_;
};

inline IEngine::ClipContexts IEngine::ClipContexts::block(int lo, int n_lang) const {
  auto from = [](auto* p, size_t k) { return p ? p + k : p; };
  ClipContexts c = *this;
  if (c.prompts) *c.prompts = {from(prompts->ids, (size_t)lo * prompts->stride), prompts->stride, from(prompts->n_prompt, lo)};
  if (c.lang) *c.lang = {from(lang->lang, lo), from(lang->task, lo)};
  c.lang_out = {from(lang_out.detected, lo), from(lang_out.lang_logprob, (size_t)lo * n_lang), from(lang_out.lang_logit, (size_t)lo * n_lang)};
  return c;
}

inline IEngine::DecodeRequest IEngine::DecodeRequest::block(int lo, int n_ctx, int n_lang) const {
  auto from = [](auto* p, size_t k) { return p ? p + k : p; };
  DecodeRequest r = *this;
  r.max_new_clip = from(max_new_clip, lo);
  r.sample_rate = from(sample_rate, lo);
  if (r.sample) *r.sample = {from(sample->temperature, lo), from(sample->stream, lo), sample->seed};
  r.ctx = ctx.block(lo, n_lang);
  if (r.scores)
    *r.scores = {from(scores->token_logprob, (size_t)lo * n_ctx), from(scores->avg_logprob, lo), from(scores->no_speech_logprob, lo),
                 from(scores->ended_eot, lo)};
  return r;
}

// One persistent decode launch at a time per GPU, whichever build (bfloat16 / half) the launching handle belongs to:
// the launch needs every CU, and two of them co-resident would each hold part of the chip until both give up. Defined
// once in api.cpp (the engine's translation units are compiled twice).
std::mutex& persistent_launch_mutex(int device);

// Stream capture of a decoder step (hipStreamBeginCapture ... EndCapture) and the calls that may invalidate SOMEBODY ELSE's
// capture on the same device (allocation, synchronous copies, device-wide synchronisation: engine construction, capacity
// growth, StreamOpen, the stage-level entry points) take this mutex — ONE for the whole process (round 4; it was one per
// device), whichever handle, device or build they belong to: two handles on one GPU — whisper_srv --devices 0,0, or a bf16
// and an fp16 model side by side — would otherwise break each other's capture ("operation failed due to a previous error
// during capture"), and whether handles on DIFFERENT GPUs can was never observable on a one-GPU box. Held for
// milliseconds, a few times per handle lifetime (engine construction: for its whole duration). Defined once in api.cpp.
std::recursive_mutex& device_capture_mutex(int device);

IEngine* make_engine_bf16(const std::string& model_type, const std::string& model_path, const std::string& language, int device, int max_batch);
IEngine* make_engine_f16(const std::string& model_type, const std::string& model_path, const std::string& language, int device, int max_batch);
// Host only: which persistent launch a decoder shape gets on n_cu compute units and its cross-attention role assignment
// (decode_persistent.hip: decode_persistent_plan; include/ax_whisper_api.h: AX_WHISPER_PersistentDecodePlan).
int persistent_decode_plan(int d_model, int n_head, int n_layer, int n_cu, int n_clips, int t0, int n_slots, int* plan4, int* units);

}  // namespace axw
