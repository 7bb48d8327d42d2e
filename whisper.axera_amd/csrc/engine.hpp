// engine.hpp — the MI355X Whisper engine behind the AX_WHISPER_* C ABI.
//
// Replaces class Whisper (cpp/src/Whisper.hpp:28-59, cpp/src/Whisper.cpp) together with the two
// AxModelRunner NPU executors it owns (cpp/src/ax_model_runner/ax_model_runner.hpp:23-80): model
// directory loading (Whisper.cpp:86-149), preprocess (:151-184), encoder call (:190-195),
// cross-KV hand-off (:260-288, here: none — the encoder writes the decoder's layouts in place),
// the greedy loop (:207-222) and detokenisation (:224-229). The reference handles one utterance at
// a time; this engine runs B utterance slots through every stage as one batch.
#pragma once

#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "iengine.hpp"
#include "suppress.hpp"
#include "t2s.hpp"

namespace axw {
class SafeTensors;  // host_io.hpp
inline namespace AXW_NS {

// Every HIP object of an engine has exactly one owner (engine_impl.hpp, through which this header is included), in one of the
// four groups below. Engine::destroy() empties them under device_capture_mutex in the order graph execs, memory, events,
// streams (Engine's base order is the reverse, so its destructor alone would keep that order): a member added to a group is
// released with it, nothing is listed a second time.
struct EngineStreams {
  Stream own_stream_;
  std::vector<Stream> pad_streams_;  // align_graph_queue() (engine_stream.cpp); AX_WHISPER_PAD_STREAMS (diagnostic)
  static constexpr int kMaxBranches = 4;   // parallel branches of the batched step graph
  Stream branch_stream_[kMaxBranches - 1];
  Stream admit_stream_, copy_stream_;  // (copies: stream_collect's D2H, never behind the queued decoder steps)
};

struct EngineEvents {
  Event ev_fork_, ev_join_[EngineStreams::kMaxBranches - 1];
  std::vector<Event> ev_admit_;     // one per slot: its encoder has finished
  Event ev_step_[3];  // the host stays two steps ahead of the device (stream_step)
  // admission passes do not wait for one another's encoder: clip lengths and slot maps go through a pinned ring of
  // kAdmitRing entries (an entry is reused once the pass that filled it has finished), the PCM staging rows are reused once
  // the previous pass's uploads have landed
  static constexpr int kAdmitRing = 4;
  Event ev_ring_[kAdmitRing], ev_upload_, ev_[5];
};

// long-form (engine_long.cpp): the PCM and the log-mel rows of every file of one call in one arena, kept for the next call
// when small (allocated and freed under device_capture_mutex)
struct LongArena {
  DeviceArray<char> base; size_t bytes = 0;
  float *pcm = nullptr, *store = nullptr;
  long long *pcm_off = nullptr, *frame_off = nullptr;
  int *n_samples = nullptr, *n_frames = nullptr, *win_file = nullptr, *win_seek = nullptr;
  unsigned* gmax = nullptr;
  int n_files = 0, n_windows = 0;
  // chunked calls only (long_prepare with cut parameters; else null): the smoothed and the frame levels [frames of all files], every
  // file's room in the per-file window lists, those lists, and the plan block the host fetches in one copy:
  // [n_windows per file | win_file | win_seek | win_len], the last three [plan_cap] in the flat order file-then-seek
  float *levels = nullptr, *levels_e = nullptr;
  int *seg_off = nullptr, *seg_seek = nullptr, *seg_len = nullptr, *plan = nullptr;
  int plan_cap = 0, max_frames = 0;
  int* plan_n() const { return plan; }
  int* plan_file() const { return plan + n_files; }
  int* plan_seek() const { return plan + n_files + plan_cap; }
  int* plan_len() const { return plan + n_files + 2 * (size_t)plan_cap; }
};

struct EngineMemory {
  std::vector<DeviceMem> slot_allocs_;  // capacity-dependent buffers
  std::vector<DeviceMem> allocs_;       // weights + constants (freed at destruction)
  DeviceMem load_stage_;  // staging buffer of load_weights
  PinnedArray<float> h_pcm_;
  // clips longer than a staging row (60 s): their tails, packed, so that the clamp floor comes from ALL frames of the
  // input however long it is (Whisper.cpp:158-172); grown on demand, empty for ordinary requests
  DeviceArray<float> d_over_; size_t over_cap_ = 0;
  // sample rates (DESIGN.md "Sample rates"): the filter tables of every rate the handle has met, packed in one arena (built on
  // first use under device_capture_mutex, kept for the handle's life), and the raw staging of clips that are not at 16 kHz: their
  // samples as uploaded (pinned host + device, grown on demand under the mutex, kept) and the launch's clip descriptors
  DeviceArray<float> d_rs_tables_; size_t rs_tables_cap_ = 0, rs_tables_used_ = 0;
  DeviceArray<float> d_raw_; PinnedArray<float> h_raw_; size_t raw_cap_ = 0;
  DeviceArray<ResampleClip> d_rs_clips_; PinnedArray<ResampleClip> h_rs_clips_; int rs_clips_cap_ = 0;
  LongArena long_;
  PinnedArray<int> h_long_win_; int h_long_win_cap_ = 0;  // pinned [2][windows per pass]: file and seek of every slot
  PinnedArray<int> h_poll_;
  PinnedArray<int> h_done_live_; int* d_done_live_ = nullptr;  // host-mapped [cap] (and its device alias): advance_kernel raises a clip's
                                                               // flag the moment it finishes; the host reads it without any wait
  PinnedArray<int> h_admit_ring_;          // pinned [kAdmitRing][2][cap]
  DeviceArray<unsigned long long> d_stamp_;  // bench "attn_stamp"
  // prompt prefill (engine_prefill.cpp): the pass's rows (residual stream fp32, activations h16, per-row tables) and per-clip
  // arrays (gathered sot rows, no-speech values, tables), grown on first use under device_capture_mutex
  struct PrefillScratch {
    DeviceArray<float> x, xg, nsp, sot_logits;  // sot_logits [clips][ts_stride_]: the rows the no-speech values were taken from
    DeviceArray<h16> ln, qkv, att, hid;
    DeviceArray<int> row_tab, clip_tab;
    int rows_cap = 0, clips_cap = 0;
    // language and task per clip: the detecting slots and the context entries to patch [2][clips], the clips' task ids, and the detection kernel's
    // language id list [n_lang] and outputs (index [clips], logprob and logit [clips][n_lang])
    DeviceArray<int> det_tab, task_tok, lang_tok, lang_idx;
    DeviceArray<float> lang_lp, lang_logit;
  } prefill_;
};

struct EngineGraphs {
  // key: Engine::graph_key; with every captured step, the fp8 cross-attention launches one replay of it runs
  struct StepGraph { GraphExec exec; int fp8_launches = 0; };
  struct StepGraphRef { hipGraphExec_t exec; int fp8_launches; operator hipGraphExec_t() const { return exec; } };  // what step_graph() hands out
  std::map<long, StepGraph> graphs_;
};

// Typed pointers into slot_allocs_ (they own nothing): Engine::free_slot_buffers() resets all of them with the pool.
struct SlotViews {
  float* d_ts_logits_ = nullptr;  // [cap][ts_stride_], allocated on first use under device_capture_mutex
  // scored mode (DESIGN.md "Confidence"): per-clip log-probability and id of every decision [cap][n_text_ctx], log p(<|nospeech|>)
  // [cap]; allocated like d_ts_logits_. own_scores_: these arrays as the scored rules kernel takes them (decode_forced hands it
  // its own [batch][n_forced + 1] buffers instead)
  float* d_tok_lp_ = nullptr; int* d_dec_id_ = nullptr; float* d_nospeech_ = nullptr;
  TsScoreParams own_scores_{};
  // sampled mode (DESIGN.md "Temperature fallback"): per-clip temperature and random stream [cap], the call's seed [1]; allocated
  // with the score arrays. own_sample_: these arrays as the sampled rules kernel takes them
  float* d_temp_ = nullptr; unsigned long long *d_rng_stream_ = nullptr, *d_rng_seed_ = nullptr;
  TsSampleParams own_sample_{};
  float *d_a0_ = nullptr, *d_statp_ = nullptr;  // [B][d] A0 -> T; [B][d/16][2] block statistics of the residual rows
  float* d_pcm_ = nullptr; long long* d_over_off_ = nullptr;
  int* d_nsamp_ = nullptr; unsigned* d_gmax_ = nullptr; float* d_logmel_ = nullptr; float* d_mel_ref_ = nullptr;
  h16 *d_mel_tm_ = nullptr, *d_h1_ = nullptr, *d_ln_ = nullptr, *d_q_ = nullptr, *d_k_ = nullptr, *d_vt_ = nullptr,
       *d_attn_ = nullptr, *d_ffn_ = nullptr;
  float *d_x_ = nullptr, *d_enc_part_ = nullptr;
  h16 *d_cross_k_ = nullptr, *d_cross_v_ = nullptr, *d_self_k_ = nullptr, *d_self_v_ = nullptr;
  // FP8 cross K/V (AX_WHISPER_CROSS_KV=fp8; decode_layout.hpp "FP8 cross K/V"): the code images [L][cap][H] and their scales, beside
  // the h16 images; null on a default handle
  unsigned char *d_cross_k8_ = nullptr, *d_cross_v8_ = nullptr;
  float* d_cross_scales_ = nullptr;
  float *d_xdec_ = nullptr, *d_qdec_ = nullptr, *d_hid_ = nullptr, *d_part_self_ = nullptr, *d_part_cross_ = nullptr;
  h16 *d_act_[2] = {nullptr, nullptr}, *d_att_[2] = {nullptr, nullptr}, *d_hidp_[2] = {nullptr, nullptr};
  float* d_part_ = nullptr; float* d_amax_val_ = nullptr; int* d_amax_idx_ = nullptr;
  float* d_attn_mpart_ = nullptr;     // batched cross-attention in splits: partials and tickets (DecAttnParams::mpart / mcnt)
  unsigned* d_attn_mcnt_ = nullptr;
  int *d_tok_ = nullptr, *d_done_ = nullptr, *d_done_none_ = nullptr, *d_nout_ = nullptr, *d_out_ids_ = nullptr, *d_max_new_clip_ = nullptr;
  int* d_off_ = nullptr;   // per-slot offsets (common.hpp: DecState)
  int* d_slot_map_ = nullptr;            // [cap]: clip index of an admission pass -> slot
  // slot stream in timestamp mode (DESIGN.md "Slot stream in timestamp mode"): every slot's prefix [cap][4] = [sot, language id, task
  // id, unused], detect flag and language index [cap], lang_logprob [cap][n_lang]; allocated like d_ts_logits_
  int *d_slot_ctx_ = nullptr, *d_slot_detect_ = nullptr, *d_slot_lang_ = nullptr;
  float* d_slot_lang_lp_ = nullptr;
  // beam search (engine_beam.cpp; common.hpp: BeamCandParams / BeamSelectParams): per-slot and per-clip state [cap], histories and
  // pool ids [cap][n_text_ctx], candidates [cap][kBeamMaxCand]; allocated on first use under device_capture_mutex
  struct BeamViews {
    int *hist = nullptr, *cand_id = nullptr, *n_cand = nullptr, *slot = nullptr, *src = nullptr, *pool_n = nullptr, *pool_ids = nullptr,
        *pool_len = nullptr, *complete = nullptr, *n_complete = nullptr;
    float *cand_lp = nullptr, *S = nullptr, *slot_score = nullptr, *pool_score = nullptr;
  } beam_;
  DecState* d_state_ = nullptr;
};

class Engine final : public IEngine, private EngineStreams, private EngineEvents, private EngineMemory, private EngineGraphs, private SlotViews {
 public:
  Engine(const std::string& model_type, const std::string& model_path, const std::string& language, int device, int max_batch);
  ~Engine() override;
  Engine(const Engine&) = delete;

  void run_tokens(const DecodeRequest& rq, const float* const* pcm, const float* d_pcm, int d_stride, const int* n_samples, int batch, int32_t* ids,
                  int* n_ids) override;
  std::string detokenize(const int32_t* ids, int n) const override;
  const std::vector<std::string>& token_table() const override { return tokens_; }
  std::string transcript(const int32_t* ids, int n) const override;
  std::string transcript_lang(const int32_t* ids, int n, int lang) const override;
  bool has_t2s() const { return (bool)t2s_; }
  void compute_mel(const float* pcm, int n_samples, float* mel_out, int rate = 16000) override;
  void resample(const float* const* pcm, const int* n_samples, const int* rates, int batch, float* const* out, const int* out_cap,
                int* n_out) override;
  void encode_mel(const float* mel, int batch) override;
  void get_cross_kv(int slot, float* k_out, float* v_out) override;
  void get_cross_kv_fp8(int slot, unsigned char* k_codes, unsigned char* v_codes, float* scales) override;
  void cross_kv_quantize() override;
  void decode_forced(DecodeMode mode, const ClipContexts& ctx, int batch, const int32_t* forced, int n_forced, float* logits, int32_t* chosen,
                     const ForcedScores* scores, const SampleSpec* sample) override;
  void get_self_kv(int slot, int n_rows, float* k_out, float* v_out) override;
  void get_persistent_self_kv(int clip, float* k_out, float* v_out) override;
  void prefill_stage(int batch, const ClipContexts& ctx, float* no_speech_logprob, float* sot_logits) override;
  void detect_language(const float* const* pcm, const int* n_samples, int batch, const LangResult& out) override;
  void detect_language_stage(int batch, const LangResult& out) override;
  void language_logprob_rows(const float* rows, int n, float* lang_logprob, int* lang_index, float* lang_logit) override;
  void decode_greedy(DecodeMode mode, int batch, int max_new, const int* max_new_clip, int32_t* ids, int* n_ids) override;
  void timestamp_rules(const float* logits, const int32_t* hist, const int* n_hist, int batch, int32_t* chosen, float* logprob,
                       const SampleSpec* sample = nullptr) override;
  void no_speech_logprob(const float* logits, int batch, float* out) override;
  void run_beam(const float* const* pcm, const int* n_samples, int clips, int beam_size, int max_new, const BeamResult& out,
                float* no_speech_logprob) override;
  void decode_beam(int clips, int beam_size, int max_new, const BeamResult& out, float* no_speech_logprob, BeamTrace* trace) override;
  void beam_candidates(const float* logits, const int32_t* hist, const int* n_hist, int rows, int n_cand_max, int32_t* cand_id,
                       float* cand_logprob, int* n_cand) override;
  int beam_select(const BeamSelectIO& io) override;
  void align_tokens(const AlignRequest& rq) override;
  void set_alignment_heads(const int* pairs, int n) override;
  void set_suppress_tokens(const int* ids, int n) override;
  const std::vector<int>& suppress_tokens() const override { return suppress_ids_; }
  void align_kernel(int which, const AlignKernelIO& io) override;
  void vocab_logprob_rows(const float* x, int n_rows, const int32_t* ids, float* out, int route) override;
  void stream_open(int n_slots, int mode = 0) override;
  void stream_admit(const int* slots, const float* const* pcm, const int* n_samples, const int* max_new, int count,
                    const int* rates = nullptr, const int* lang = nullptr, const int* task = nullptr) override;
  int stream_step(int n_steps, int* finished_slots) override;
  void stream_collect(int slot, int32_t* ids, int* n_ids) override;
  void stream_collect_scored(int slot, int32_t* ids, int* n_ids, const SlotScores& out) override;
  void stream_rules_stage(const StreamRulesIO& io) override;
  void stream_close() override;
  void compute_mel_window(const float* pcm, int n_samples, int seek, float* mel_out) override;
  void run_long_windows(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes,
                        const LongScoreOptions* opts, std::vector<LongWindow>& log) override;
  void run_long_chunked(const float* const* pcm, const int* n_samples, int n_files, int max_new, int max_passes, const ChunkedOptions& opts,
                        std::vector<LongWindow>& log) override;
  void long_frame_levels(const float* const* pcm, const int* n_samples, int n_files, int smooth, float* const* e, float* const* s) override;
  void long_cut_plan(const float* const* pcm, const int* n_samples, int n_files, const CutParams& cut, std::vector<int>& n_windows,
                     std::vector<int>& win_file, std::vector<int>& win_seek, std::vector<int>& win_len, float* const* s_out) override;
  void long_cut_plan_from_levels(const float* s, int content, int w_min, int w_max, std::vector<CutWindow>& plan) override;
  void compute_mel_window_cut(const float* pcm, int n_samples, int seek, int len, float* mel_out) override;
  int scan_stored16(int batch, int n_max, char (*names)[32], long long* nonfinite, float* maxabs) override;
  float bench(const std::string& what, int batch, int arg, int iters) override;
  void set_stream(void* s) override { user_stream_ = static_cast<hipStream_t>(s); }
  const ModelConfig& config() const override { return cfg_; }
  const char* dtype_name() const override { return kDtypeName; }
  const int* sot_seq() const { return sot_seq_; }

 private:
  struct EncLayer {
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    h16 *w_qkv, *w_o, *w_fc1, *w_fc2;
    float *b_qkv, *b_o, *b_fc1, *b_fc2;
  };

  void construct(const std::string& model_type, const std::string& model_path, const std::string& language, int device, int max_batch);
  void destroy();  // idempotent: the destructor's work, also run when the constructor throws
  hipStream_t stream() const { return user_stream_ ? user_stream_ : own_stream_.get(); }
  // a new buffer of `pool` (allocs_ / slot_allocs_), which owns it
  template <class T> T* pooled(std::vector<DeviceMem>& pool, size_t n, bool zero = false) {
    return static_cast<T*>(pool.emplace_back(device_alloc(n * sizeof(T), zero)).get());
  }
  void load_config(const std::string& dir, const std::string& type, const std::string& language);
  void load_weights(const SafeTensors& st);
  void load_t2s(const std::string& model_path);
  std::unique_ptr<T2SConverter> find_t2s() const;  // the converter of the first t2s.json found, or null
  void ensure_capacity(int batch);
  void free_slot_buffers();
  // rates (or null: every clip at 16000 Hz): a clip at another rate goes to the raw staging and the resample kernel writes its
  // staging row (and overflow tail); n_16k (required with rates): the clips' lengths at 16 kHz, which run_frontend then takes
  void upload_pcm(const float* const* pcm, const int* n_samples, int batch, const int* rates = nullptr, int* n_16k = nullptr);
  // sample rates (engine.cpp): a rate's filter and where its table sits in d_rs_tables_ (built and uploaded on first use)
  struct RateTable { int L, M, K; long long tab_off; };
  std::map<int, RateTable> rate_tables_;
  const RateTable& rate_table(int rate);
  void ensure_resample_staging(size_t raw_samples, int clips);  // d_raw_ / h_raw_, d_rs_clips_ / h_rs_clips_
  float bench_resample(int batch, int rate, int iters);
  // pinned_ns: optional pinned host [batch] the clip lengths are staged through (then nothing here waits for the stream)
  void run_frontend(const float* d_pcm, int stride, const int* n_samples, int batch, bool want_ref_layout, bool staged = false,
                    int* pinned_ns = nullptr);
  void run_encoder(int batch, const int* d_slot_map = nullptr);  // cross K/V of clip b goes to slot d_slot_map[b] (device), else b
  void reset_decode_state(int batch, const int* max_new_clip = nullptr);
  // What one decoder step is built as: every step sequence, the graph it is captured into and the key that graph is cached
  // under are made from ONE of these, handed down as an argument.
  struct StepSpec {
    DecodeMode mode = kDecodePlain;
    // launches of the step (all: 15): 1 GEMV/GEMM launches, 2 attention launches, 4 advance, 8 act_prep, 16 attention launches stamp
    // themselves (bench only)
    int mask = 15;
    TsScoreParams score_out{};  // kDecodeScored, kDecodeSampled: where the scored / sampled rules kernel writes
    TsSampleParams sample{};    // kDecodeSampled: what the sampled rules kernel draws with (the engine's own arrays)
    // step-fed prompt route (engine_prefill.cpp; never captured): advance feeds forced[0 ..] from position 0 (a one-id prefix) and
    // the logits launch is skipped (1) or dumps every row into d_ts_logits_ (2)
    int feed = 0;
    const int* base = nullptr;  // teacher-forced prompted decode: device [batch], the clips' L - 2 (AdvanceParams::base)
    // slot stream in timestamp mode (engine_stream.cpp; kDecodeScored only): the rules launch is stream_rules_kernel and the advance
    // launch feeds every slot its own prefix from d_slot_ctx_
    bool slots = false;
    // the cross-attention launches of a step of more than gemv_max_ clips read the FP8 code images (cross_kv_fp8.hip); set from the
    // handle's mode by step_spec(), left clear by beam search (its spread kernel copies only the h16 images) and by the detection
    // and step-fed context steps of engine_prefill.cpp
    bool cross_fp8 = false;
  };
  StepSpec step_spec(DecodeMode mode = kDecodePlain, int mask = 15) const { StepSpec sp{mode, mask}; sp.cross_fp8 = cross_fp8_; return sp; }
  // logits rows of one step that leave it: plain mode, the caller's; timestamp and scored mode, every row, into d_ts_logits_ for
  // the rules kernel; first_step: the first decode step whose row is computed
  struct LogitsDump { float* rows; long stride; int first_step; };
  LogitsDump logits_dump(const StepSpec& spec, float* d_logits, long logits_stride) const;
  void enqueue_decode_step(const StepSpec& spec, int batch, int max_new, const int* d_forced, int n_forced, float* d_logits,
                           long logits_stride, int* d_argmax);
  void enqueue_decode_step_batched(const StepSpec& spec, int batch, int max_new, const int* d_forced, int n_forced, float* d_logits,
                                   long logits_stride, int* d_argmax);
  // what both end in: the rules kernel (timestamp and scored mode) and advance_kernel; n_part: argmax partials of the logits launch
  void enqueue_step_tail(const StepSpec& spec, int batch, int max_new, const int* d_forced, int n_forced, int* d_argmax, int n_part,
                         hipStream_t s);
  void enqueue_layers_cblock(const StepSpec& spec, int b0, int nb, hipStream_t s, bool forced, bool one_branch);
  // what every attention launch of a step has in common, for clips [b0, b0 + nb): n_keys < 0 self-attention, else cross-attention
  DecAttnParams attn_params(const float* q, const h16* k, const h16* v, long stride, int n_keys, int cap_blocks, int b0, int nb, bool forced) const;
  int decode_branches(int batch) const;
  void ensure_branch_streams(int batch);
  // the captured step of spec.mode / spec.mask; a scored graph writes the engine's own score arrays (spec.score_out is not read)
  StepGraphRef step_graph(StepSpec spec, int batch, int max_new);
  void drop_step_graph(const StepSpec& spec, int batch, int max_new) { graphs_.erase(graph_key(spec, batch, max_new)); }
  // (two bits for the mode: plain, timestamp, scored and sampled steps are four different graphs; one for the slot stream's scored
  // step; one for "a suppress set is installed" where the graph holds a rules launch, which has the mask's pointer by value)
  long graph_key(const StepSpec& spec, int batch, int max_new) const {
    const bool suppress = spec.mode != kDecodePlain && (spec.mask & 4) && suppress_mask();
    return ((((long)batch * 1024 + max_new) * 32 + spec.mask) << 5) | (spec.cross_fp8 ? 16 : 0) | (suppress ? 8 : 0) | (spec.slots ? 4 : 0) | spec.mode;
  }
  void require_timestamp_vocab() const;
  // token suppression (DESIGN.md "Token suppression"; suppress.hpp): the handle's set as a sorted id list, what the config file
  // gave (what n == 0 restores), and its mask on the device: allocated on first use under device_capture_mutex, at one address
  // for the life of the handle, rewritten on the engine's stream
  std::vector<int> suppress_ids_, config_suppress_;
  unsigned* d_suppress_ = nullptr;  // (in allocs_)
  const unsigned* suppress_mask() const { return suppress_ids_.empty() ? nullptr : d_suppress_; }  // what the parameter structs get
  void install_suppress(const std::vector<int>& ids);
  void ensure_ts_logits();  // d_ts_logits_ (SlotViews)
  void enqueue_timestamp_rules(const StepSpec& spec, int batch, const int* d_forced, int n_forced, hipStream_t s);
  long ts_stride_ = 0;
  void require_scored_vocab() const;  // require_timestamp_vocab + a usable no_speech id
  // What the kernels-alone entry points hand their kernel: host rows [rows][n_vocab] on the device at a stride of whole 16-byte
  // chunks, with their histories [rows][n_text_ctx] and lengths (hist == nullptr: the rows alone), copied on the stream.
  // Throws "<what>: n_hist out of range" before it allocates or copies anything.
  struct StagedRows { DeviceArray<float> logits; DeviceArray<int> hist, n_hist; long stride = 0; };
  StagedRows stage_rows(const char* what, const float* logits, const int32_t* hist, const int* n_hist, int rows, hipStream_t s);
  void ensure_ts_scores();
  // checks a SampleSpec of `batch` clips and puts it into the engine's own arrays (on the stream, before the steps that read them)
  void upload_sample(const SampleSpec& sample, int batch);
  // scores of the last scored greedy loop over `batch` slots (n_ids: what fetch_ids returned)
  void fetch_scores(int batch, const int* n_ids, float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot);
  // one clip of it: lp / dec [n_text_ctx] as the scored rules kernel left them -> token_logprob [n_text_ctx], avg_logprob, ended_eot
  void clip_score_summary(const float* lp, const int* dec, int n_ids, float* token_logprob, float* avg_logprob, int* ended_eot) const;
  void recover_streams();
  // long-form (engine_long.cpp)
  // upload + whole-file front-end; cut (chunked calls): also room for the levels (want_e: both of them) and the cut plan
  void long_prepare(const float* const* pcm, const int* n_samples, int n_files, int n_windows, const CutParams* cut = nullptr, bool want_e = false);
  void long_plan(const CutParams& cut);  // levels kernel + plan kernels over the prepared files
  // the plan block in one copy -> windows per file and the flat lists; returns the number of windows
  int long_fetch_plan(std::vector<int>& n_windows, std::vector<int>& win_file, std::vector<int>& win_seek, std::vector<int>& win_len);
  void long_cut_windows_to_slots(int first, int count, bool want_ref_layout);  // windows [first, first + count) of the plan -> slots 0 ..
  void long_windows_to_slots(const int* files, const int* seeks, int count, bool want_ref_layout);
  void long_release();
  // ctx: what the clips decode behind (prefill_prompts after reset_decode_state); an empty one: nothing in front of the start sequence
  int greedy_loop(const StepSpec& spec, int batch, int max_new, const int* max_new_clip, const ClipContexts& ctx);
  // prompt conditioning and a language and task per clip (engine_prefill.cpp; DESIGN.md "Prompt conditioning", "Language and task per
  // clip"). A call's contexts travel as an argument from its entry point to prefill_prompts, which plans them and brings every clip
  // that gets one to "context cached, task id about to be fed". force_context: every clip gets a context (decode_forced under a
  // language spec).
  // no_speech_out / sot_logits_out (stage level; host [batch] / [batch][n_vocab], or null): the no-speech value of the slots behind a
  // context and the raw logits row it was taken from; entries of the other slots are 0
  void prefill_prompts(int batch, const ClipContexts& ctx, bool force_context, bool want_no_speech, float* no_speech_out = nullptr,
                       float* sot_logits_out = nullptr);
  // after_cq (null for every caller but the alignment): called for layer l once its cross-attention queries stand in prefill_.qkv
  // (h16 [rows][d], behind the w_cq GEMM), before anything overwrites them
  using LayerHook = std::function<void(int layer)>;
  void prefill_pass(int rows, int n_clips, int max_len, bool want_no_speech, const LayerHook* after_cq = nullptr);
  // word-level timestamps (engine_align.cpp; DESIGN.md "Word-level timestamps")
  std::vector<std::pair<int, int>> align_heads_;  // (layer, head), sorted; empty: the default list
  std::vector<std::pair<int, int>> config_heads_; // the config file's "alignment_heads" (empty: none): what n == 0 restores
  std::vector<std::pair<int, int>> alignment_heads() const;
  int align_env_ = -1;   // AX_WHISPER_WORD_ALIGN, read at first use: 0 the GPU route, 1 the host route
  int align_force_ = -1; // bench "word_align" / "word_align_host": that route for the call in progress
  int align_route();
  // token probabilities (kAlignLogProbRows / kAlignLogProbFused): AX_WHISPER_WORD_LOGPROB, read at first use (-1 unread, 0 none,
  // 1 rows, 2 fused), overrides what a request asks for
  int logprob_env_ = -1;
  int logprob_route(int requested);
  // lp[i] = log p(id[i]) over the ids below eot from the final residual row x[row[i]] (row == nullptr: x[i]); all device memory
  void token_logprob_rows(const float* x, const int* row, const int* id, int n, float* lp, hipStream_t s);   // four rows per logits launch
  void token_logprob_fused(const float* x, const int* row, const int* id, int n, float* lp, hipStream_t s);  // vocab_logprob.hip
  float bench_word_logprob(const std::string& what, int batch, int arg, int iters);
  float bench_word_align(const std::string& what, int batch, int arg, int iters);
  int handle_lang_ = 0;  // index of the handle's language in the config's list
  // what an entry point asks before any GPU work: the mode rules of ctx (timestamp modes; under a language spec no open stream) and
  // the context plan of `batch` clips, which throws on a bad prompt, language or task
  void check_contexts(DecodeMode mode, const ClipContexts& ctx, int batch, bool force_context, const char* what) const;
  void require_lang_call(DecodeMode mode, const char* what) const;  // timestamp modes, no open stream
  void ensure_lang_buffers();  // prefill_.lang_tok (+ the per-clip arrays, with ensure_prefill_scratch)
  LangDetectParams detect_params(const float* x, int n_clips, bool want_logit) const;
  // prefill route: the layers of one decoder step at offset 0 (no vocabulary projection, no advance) and the detection kernel on
  // the detecting slots' final residual rows, all on the stream; d_ctx (or null) is patched at lang_row. Results stay on the device
  // until fetch_detected.
  void enqueue_detect_prefill(int batch, const std::vector<int>& slot, int* d_ctx, const std::vector<int>& lang_row, bool want_logit);
  void fetch_detected(int n, int* idx, float* lp, float* logit);
  // step-fed route: one decoder step at offset 0 with the logits dump, the pick on the host; leaves the decode state reset
  void detect_step_fed(int batch, const std::vector<int>& slot, int* idx, float* lp, float* logit);
  void prefill_step_fed(int batch, const std::vector<int>& slot, const std::vector<int>& len, const std::vector<int>& ctx,
                        const std::vector<int>& row0, bool want_no_speech);
  void ensure_prefill_scratch(int rows, int clips);
  int prefill_env_ = -1;           // the handle's route (AX_WHISPER_PREFILL; the step-fed route where the prefill kernels refuse the shape)
  int prefill_force_ = -1;         // bench "prefill_pass" / "prefill_step": that route for the call in progress
  int prefill_route();             // 0 the prefill pass, 1 the step-fed route (AX_WHISPER_PREFILL=step)
  bool prefill_supported() const;  // the prefill kernels take this decoder shape
  // batch 1: the whole loop as one persistent launch (decode_persistent.hip); returns steps run, -1 if it gave up
  // mode kDecodeTimestamps / kDecodeScored (one clip, slot 0): the launch's rules instantiation; scores: where a scored launch writes
  // (nullptr: the engine's own arrays), d_logits0: teacher forcing, the row of decode offset 0
  int run_persistent(int max_new, const int* d_forced, int n_forced, float* d_logits, int* d_argmax, int slot = 0, int max_new1 = -1, int max_new2 = -1,
                     DecodeMode mode = kDecodePlain, const TsScoreParams* scores = nullptr, float* d_logits0 = nullptr);
  // timestamp / scored mode of ONE clip without a context through that launch (AX_WHISPER_PERSIST_TS=1 turns the route on); asks persistent_usable()
  bool persistent_ts_route(DecodeMode mode, int batch, const ClipContexts& ctx);
  void fetch_ids(int batch, int32_t* ids, int* n_ids);
  // beam search (engine_beam.cpp)
  void ensure_beam_buffers();
  void beam_begin(int clips, int K);  // the start state of `clips` groups of K slots, on the stream
  void enqueue_beam_tail(int clips, int K, int off, int max_new, hipStream_t s);  // candidates, selection, reorder (off >= 2), advance
  void beam_spread_cross(int clips, int K);
  int beam_loop(int clips, int K, int max_new, const BeamResult& out, float* no_speech_logprob, BeamTrace* trace);

  ModelConfig cfg_;
  int sot_seq_[4] = {0, 0, 0, 0};
  std::vector<std::string> tokens_;
  std::unique_ptr<T2SConverter> t2s_;  // zh only
  // a handle of another language: the converter for clips decoded under zh (transcript_lang), looked for at first use
  std::string model_path_;
  mutable std::once_flag t2s_late_once_;
  mutable std::unique_ptr<T2SConverter> t2s_late_;
  std::string effective_lang_;
  bool feature_openai_ = false;  // feature_mode "openai" (engine.cpp load_config)
  int device_ = 0;
  bool device_set_ = false;
  hipStream_t user_stream_ = nullptr;  // the caller's (AX_WHISPER_SetStream): not owned
  bool graph_branch_shares_queue(hipGraphExec_t exec, hipStream_t other);
  int queue_probe_mask();  // bench "queue_probe" (engine_stream.cpp: beside the probe kernels, which step_graph needs)

  // weights
  h16 *conv1_w_ = nullptr, *conv2_w_ = nullptr, *w_cross_kv_ = nullptr, *tok_emb_ = nullptr;
  float *conv1_b_ = nullptr, *conv2_b_ = nullptr, *enc_pos_ = nullptr, *ln_post_w_ = nullptr, *ln_post_b_ = nullptr;
  float *b_cross_kv_ = nullptr, *dec_pos_ = nullptr, *dec_ln_w_ = nullptr, *dec_ln_b_ = nullptr;
  int conv1_k_ = 0;
  std::vector<EncLayer> enc_;
  std::vector<DecLayerW> dec_;       // per-layer views into the two arenas below
  h16* dec_w_arena_ = nullptr; float* dec_f_arena_ = nullptr;
  // w_qkv and w_cq are ONE buffer of 4 d rows ([W_qkv; W_cq]); w_o heads a buffer of 2 d rows whose second half takes the query
  // fold's M_hi, m_lo its lo halves (decode_gemm.hip "QUERY FOLD"; filled by build_cblock_fold)
  struct DecLayerWP { const h16 *w_qkv, *w_o, *w_cq, *w_co, *w_fc1, *w_fc2; h16 *m_hi, *m_lo; };
  struct CblockFold { float *b_qkv4, *b_o2; const float *s, *c; };  // per layer: [b_qkv; 0], [b_o; d], s = W_cq g, c = W_cq beta + b_cq
  std::vector<CblockFold> cfold_;      // empty: the clip-block step keeps the fused query projection
  bool cfold_all_ = false;             // AX_WHISPER_CBLOCK_QFOLD=2: also in multi-branch steps (A/B, tests)
  void build_cblock_fold();
  std::vector<DecLayerWP> dec_packed_;  // fragment-major copies for the batched decode path
  const h16* tok_emb_packed_ = nullptr;
  int nbs_ = 1;                         // allocated clip blocks of 16
  // front-end constants
  float *twiddle_ = nullptr, *window_ = nullptr, *mel_basis_t_ = nullptr;
  int* d_sot_ = nullptr;

  // capacity-dependent
  int cap_ = 0;
  int t_pad_ = 1536, mel_rows_ = 3004, h1_rows_ = 3002;
  long pcm_stride_ = 0;
  bool over_used_ = false;  // this call put clip tails into d_over_
  static constexpr int kEncPartClips = 2;  // split-K of the encoder's residual GEMMs pays for at most this many clips
  bool enc_split_k_ = true;
  float enc_rescale_thr_ = 8.f;  // launch_encoder_attention
  int gemv_max_ = 2;             // clips per call up to which the decoder step uses the GEMV family (AX_WHISPER_GEMV_MAX, <= 4)
  int cross_split_env_ = 0;      // AX_WHISPER_CROSS_SPLIT: workgroups per (clip, head) of the batched cross-attention, 0 = by clip count
  int n_amax_part_ = 0;
  int n_cu_ = 0;            // compute units of the device
  // slot refill (stream_*): a slot is idle -> encoding (admitted, encoder in flight on admit_stream_) -> active (decoding)
  // -> finished (done flag seen) -> idle again after stream_collect
  enum SlotState : int { kIdle = 0, kEncoding = 1, kActive = 2, kFinished = 3 };
  int stream_slots_ = 0;                 // > 0: a stream is open (slots of the step graph: at least 3)
  int stream_user_slots_ = 0;            // the n_slots the caller asked for: the slot indices it may use
  std::vector<int> slot_state_, slot_max_new_;
  int stream_mode_ = 0;                  // of the open stream: 0 plain, 1 scored timestamp mode
  std::vector<int> slot_lang_, slot_task_, slot_detect_;  // mode 1, per slot: language index, task id, detect flag of the admitted clip
  StepSpec stream_spec() const { StepSpec sp = step_spec(); if (stream_mode_ == 1) { sp.mode = kDecodeScored; sp.slots = true; } return sp; }
  int stream_n_prefix() const { return stream_mode_ == 1 ? 3 : 4; }
  void ensure_stream_ts();  // d_slot_ctx_ ... (SlotViews), the language id list
  StreamRulesParams stream_rules_params() const;
  long step_seq_ = 0;   // decoder steps enqueued on the open stream (ev_step_)
  long admit_seq_ = 0;  // admission passes of the open stream (h_admit_ring_, ev_ring_)
  void require_no_stream(const char* what) const;
  int split_self_ = 2, split_cross_ = 6;
  // FP8 cross K/V: the handle's mode (read at construction) and the cross-attention launches that took the fp8 kernel
  // ("cross_kv_fp8_launches"). The step sequences count what they enqueue in enq_fp8_launches_; a direct enqueue adds that to the
  // counter when it returns (enqueue_decode_step), a capture keeps it with its graph, and every replay of the graph adds it
  // (launch_step_graph, which all replays of a captured step go through).
  bool cross_fp8_ = false;
  long cross_fp8_launches_ = 0;
  int enq_fp8_launches_ = 0;
  bool in_step_capture_ = false;  // step_graph is capturing: what is enqueued runs at the replays
  void note_fp8_launches(long n) { if (n) { cross_fp8_launches_ += n; cfg_.ints["cross_kv_fp8_launches"] = (int)cross_fp8_launches_; } }
  void launch_step_graph(const StepGraphRef& g, hipStream_t s);  // hipGraphLaunch of a step_graph() exec
  void enqueue_cross_kv_quantize(int clips, const int* d_slot_map, hipStream_t s);
  // the fp8 cross-attention launch of layer l for clips [b0, b0 + nb) with a's query mode, splits and outputs
  void launch_cross_attention_fp8(const DecAttnParams& a, int l, int b0, hipStream_t s);
  float bench_cross_kv_quant(int batch, int iters);
  // bench "attn_stamp": every decode_attention launch of a captured step gets a {min begin, max end} slot (DecAttnParams::stamp)
  struct StampMeta { int layer, cross, b0, nb; };
  static constexpr size_t kStampWgs = 4096, kStampLaunches = 256;
  std::vector<StampMeta> stamp_meta_;
  unsigned long long* next_stamp(const StepSpec& spec, int layer, int cross, int b0, int nb);
  // persistent batch-1 decode
  bool batched_ln_ = false;         // batched decode: clip-block GEMM sequence (AX_WHISPER_BATCHED_LN=0 disables)
  bool persistent_ok_ = false;      // model shape supported and not disabled (AX_WHISPER_DECODE=graph)
  int persist_max_clips_ = 1;       // clips per persistent launch: up to 3 for d_model <= 768 (AX_WHISPER_PERSIST2=<n> caps it, 0 = 1)
  h16 *d_self_k1_ = nullptr, *d_self_v1_ = nullptr; size_t self1_bytes_ = 0;  // the later clips' self-attention caches of that launch
  int persist_skip_ = 0, persist_backoff_ = 0, persist_giveups_ = 0;  // re-arming after a give-up (engine_decode.cpp)
  bool persistent_usable();
  void persistent_gave_up();
  void persistent_succeeded();
  int persist_grid_ = 0;
  bool persistent_ts_ = false;         // the rules instantiation serves this handle's one-clip timestamp and scored decodes ("persistent_ts")
  long persist_ts_launches_ = 0;       // such launches that finished without a give-up ("persistent_ts_launches")
  int vocab_resident_rows_ = 0;        // one-clip launch: vocabulary rows per workgroup held in the poller waves (0: AX_WHISPER_VOCAB_RESIDENT=0 or unsupported width)
  u64* d_gran_ = nullptr; size_t gran_bytes_ = 0;
  float* d_qfold_ = nullptr;  // query-fold arena of the one-clip launch (d_model <= 768), nullptr = unfolded
  // bench hooks (engine_bench.cpp): one private function per target, each returns what bench() returns
  float bench_decode_step(const std::string& what, int batch, int arg, int iters);
  float bench_decode_step_beam(int slots, int beam_size, int iters);
  float bench_attn_stamp(int batch, int arg, int iters);
  float bench_encoder(int batch, int iters);
  float bench_frontend(int batch, int iters);
  float bench_frontend_long(int batch, int arg, int iters);
  float bench_long_cut_plan(int batch, int arg, int iters);
  float bench_prefill(const std::string& what, int batch, int arg, int iters);
  float bench_detect_language(int batch, int arg, int iters);
};

}  // inline namespace AXW_NS
}  // namespace axw
