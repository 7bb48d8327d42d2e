/**
 * ax_whisper_api.h — C ABI of libax_whisper.so, MI355X (gfx950) build.
 *
 * Drop-in boundary of the reference (paths relative to the reference tree):
 *   AX_WHISPER_Init     replaces cpp/src/api/ax_whisper_api.h:54  (impl ax_whisper_api.cpp:48)
 *   AX_WHISPER_Uninit   replaces cpp/src/api/ax_whisper_api.h:67  (impl :69)
 *   AX_WHISPER_RunFile  replaces cpp/src/api/ax_whisper_api.h:81  (impl :88)
 *   AX_WHISPER_RunPCM   replaces cpp/src/api/ax_whisper_api.h:98  (impl :139)
 * Same names, argument meaning, ownership (malloc'd result, caller free()s) and error
 * behaviour (NULL / -1). The application no longer calls AX_SYS_Init / AX_ENGINE_Init
 * (whisper_cli.cpp:37-61): the library initialises HIP inside Init.
 *
 * Everything below the four legacy symbols is an ADDITION with no reference counterpart:
 * batched entry points (the reference is strictly batch 1, Whisper.hpp:15-25), token-id
 * variants for parity tests, device-resident inputs for benchmarking, and stage-level
 * entry points so each stage can be checked against the CPU oracle.
 *
 * Plain C types only: pointers, ints, sizes. No C++ or torch types cross this boundary.
 */
#ifndef _AX_WHISPER_API_H_
#define _AX_WHISPER_API_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AX_WHISPER_API __attribute__((visibility("default")))

typedef void* AX_WHISPER_HANDLE;

/* ---- legacy (byte-compatible with the reference) ------------------------------------ */

/** model files: {model_path}/{model_type}/{model_type}.safetensors (replaces the two
 *  .axmodel NPU blobs), {model_type}-tokens.txt, {model_type}_config.json.
 *  language not in the config falls back to "zh" (Whisper.cpp:241-251). NULL on failure. */
AX_WHISPER_API AX_WHISPER_HANDLE AX_WHISPER_Init(const char* model_type, const char* model_path,
                                                 const char* language);
AX_WHISPER_API void AX_WHISPER_Uninit(AX_WHISPER_HANDLE handle);
/** 16 kHz WAV (int16/int24/int32/float32 PCM) or AIFF / uncompressed AIFF-C (the reference's AudioFile reads both,
 *  AudioFile.h:450-501); stereo is averaged. 0 ok, -1 error. */
AX_WHISPER_API int AX_WHISPER_RunFile(AX_WHISPER_HANDLE handle, const char* wav_file, char** result);
/** 16 kHz mono f32 PCM in [-1, 1]. *result is malloc'd; caller frees. 0 ok, -1 error. */
AX_WHISPER_API int AX_WHISPER_RunPCM(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples,
                                     char** result);

/* ---- additions: init / info ---------------------------------------------------------- */

/** device: HIP device ordinal (-1: env AX_WHISPER_DEVICE, else 0). max_batch: number of
 *  utterance slots to allocate (<=0: env AX_WHISPER_MAX_BATCH, else 1; grows on demand). */
AX_WHISPER_API AX_WHISPER_HANDLE AX_WHISPER_InitEx(const char* model_type, const char* model_path,
                                                   const char* language, int device, int max_batch);
/** One engine per device behind ONE handle (utterance-level data parallelism, SURVEY 8e: the reference is one
 *  utterance at a time, Whisper.cpp:186-239). devices: n_devices HIP ordinals; NULL / n_devices <= 0: the list in env
 *  AX_WHISPER_DEVICES ("0,1,4" or "all"), else every visible device. Weights are replicated; RunPCMBatch /
 *  RunPCMBatchTokens split a batch into contiguous blocks of ceil(batch / devices) clips, run every block on its
 *  device from its own host thread and return when all have finished (no collective: each device copies its ids
 *  back itself). Every other entry point uses the first device. The legacy AX_WHISPER_Init does the same when
 *  AX_WHISPER_DEVICES is set, so existing callers need no source change. NULL on failure. */
AX_WHISPER_API AX_WHISPER_HANDLE AX_WHISPER_InitMulti(const char* model_type, const char* model_path,
                                                      const char* language, const int* devices, int n_devices,
                                                      int max_batch_per_device);
/** HIP devices this process can see (0 when there is none): lets a host program that links only this C ABI
 *  (whisper_srv) create one handle per device. */
AX_WHISPER_API int AX_WHISPER_VisibleDeviceCount(void);
/** Engines (devices) behind the handle; -1 for a NULL handle. */
AX_WHISPER_API int AX_WHISPER_GetDeviceCount(AX_WHISPER_HANDLE handle);
/** Integer config value by the key names of {type}_config.json (n_mels, n_vocab, eot, ...),
 *  plus "sot_seq0".."sot_seq3". Returns INT32_MIN for an unknown key.
 *  Test hook: "live_hip_objects" = the device and pinned buffers, streams, events and graphs that the handles of this
 *  process hold right now (all of them, not this handle's alone): closing a handle, or an Init that fails, leaves the
 *  count where it was before that handle. */
AX_WHISPER_API int AX_WHISPER_GetConfigInt(AX_WHISPER_HANDLE handle, const char* key);
/** Last error text of this handle (or of the last failed Init when handle is NULL). */
AX_WHISPER_API const char* AX_WHISPER_LastError(AX_WHISPER_HANDLE handle);
/** Run all device work of this handle on the caller's hipStream_t (NULL: the library's own). */
AX_WHISPER_API int AX_WHISPER_SetStream(AX_WHISPER_HANDLE handle, void* hip_stream);

/* ---- additions: batched / token-id entry points -------------------------------------- */

/** ids: [batch][n_text_ctx] int32 (row b holds n_ids[b] generated ids, eot excluded);
 *  max_new <= 0 means "until eot or context" (Whisper.cpp:219-222). */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTokens(AX_WHISPER_HANDLE handle, const float* const* pcm,
                                                const int* num_samples, int batch, int max_new,
                                                int32_t* ids, int* n_ids);
/** results: caller-provided array of `batch` char*; each entry malloc'd, caller frees. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatch(AX_WHISPER_HANDLE handle, const float* const* pcm,
                                          const int* num_samples, int batch, char** results);
/** PCM already resident in HBM: d_pcm is a DEVICE pointer to [batch][stride] f32. */
AX_WHISPER_API int AX_WHISPER_RunDeviceBatchTokens(AX_WHISPER_HANDLE handle, const float* d_pcm,
                                                   int stride, const int* num_samples, int batch,
                                                   int max_new, int32_t* ids, int* n_ids);
/** The same with a per-clip id budget (host [batch], may be NULL; <= 0: none), each capped by max_new: a RAGGED batch in one
 *  call — front-end, encoder and the loop — whose clips leave the loop at different steps the way real utterances reach eot
 *  at different steps (bench.py's realistic-length leg: synthetic weights never emit eot by themselves). */
AX_WHISPER_API int AX_WHISPER_RunDeviceBatchTokensRagged(AX_WHISPER_HANDLE handle, const float* d_pcm, int stride,
                                                         const int* num_samples, int batch, int max_new,
                                                         const int* max_new_clip, int32_t* ids, int* n_ids);
/** ids -> bytes (base64 table of {type}-tokens.txt, Whisper.cpp:224-229); ids >= the table
 *  size are skipped. A table entry ends at its first NUL byte, as in the reference (its table load strcpy's the decoded
 *  entry, Whisper.cpp:115-127, and appends it as a C string): the bytes of an entry from a NUL onward are dropped
 *  (id 188 and the like decode to nothing). *result malloc'd. */
AX_WHISPER_API int AX_WHISPER_Detokenize(AX_WHISPER_HANDLE handle, const int32_t* ids, int n, char** result);
/** The zh post-pass of Whisper::run (cpp/src/Whisper.cpp:231-236: opencc::SimpleConverter("t2s.json").Convert)
 *  on its own: config_path names an OpenCC JSON configuration (cpp/t2s.json) whose .ocd2 dictionaries sit next
 *  to it; text is UTF-8. *result malloc'd. Run* apply it themselves for language "zh" when t2s.json is found in
 *  $AX_WHISPER_OPENCC_DIR, the working directory (the reference's rule) or the model directory. Host-only. */
AX_WHISPER_API int AX_WHISPER_ConvertT2S(const char* config_path, const char* text, char** result);

/** The file decode of AX_WHISPER_RunFile on its own, host only (no handle, no GPU): WAV / AIFF -> the mono f32 samples RunFile
 *  feeds the engine (cpp/src/AudioFile.h:450-501,1241-1243 + the stereo average of ax_whisper_api.cpp:105-113). *samples is
 *  malloc'd, the caller frees it; info (may be NULL): [0] sample rate, [1] channels. 0 ok, -1 error. */
AX_WHISPER_API int AX_WHISPER_LoadAudioFile(const char* path, float** samples, int* n_samples, int* info);
/** ids -> bytes through a {type}-tokens.txt file alone, host only (Whisper.cpp:115-127 table load, :224-229 + base64.cpp:84-120
 *  decode): the bytes AX_WHISPER_Detokenize returns, with their count (entries end at their first NUL as there, so the
 *  result holds none; n_bytes saves the caller a strlen). *result malloc'd. */
AX_WHISPER_API int AX_WHISPER_DetokenizeWithTable(const char* tokens_path, const int32_t* ids, int n, char** result, int* n_bytes);

/* ---- additions: stage-level entry points (parity tests, profiling) ------------------- */

/** Whisper::preprocess (Whisper.cpp:151-184) on the GPU. mel_out: host [n_mels*3000] f32. */
AX_WHISPER_API int AX_WHISPER_ComputeMel(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples,
                                         float* mel_out);
/** Encoder + cross-KV projection for `batch` clips given host mels [batch][n_mels*3000];
 *  results stay in the handle's slots 0..batch-1. */
AX_WHISPER_API int AX_WHISPER_EncodeMel(AX_WHISPER_HANDLE handle, const float* mel, int batch);
/** Copy slot's cross K/V back as fp32 [n_text_layer][1500][n_text_state] (reference layout). */
AX_WHISPER_API int AX_WHISPER_GetCrossKV(AX_WHISPER_HANDLE handle, int slot, float* k_out, float* v_out);
/** FP8 cross K/V (opt-in): a handle made while the environment variable AX_WHISPER_CROSS_KV is "fp8" also keeps the cross K/V as
 *  OCP e4m3fn codes with one power-of-two scale per (layer, slot, head, K or V, head dimension), written by a quantise kernel at the
 *  end of the encoder, and the cross-attention launches of decoder steps of more than two clips read the codes. Absent or "h16":
 *  today's behaviour; any other value fails Init with an error text. AX_WHISPER_GetConfigInt: "cross_kv_fp8" (0 / 1),
 *  "cross_kv_fp8_launches" (cross-attention launches that took the fp8 kernel).
 *  GetCrossKVFp8: the slot's raw codes de-blocked to [n_text_layer][1500][n_text_state] bytes (value = code * scale) and its scales
 *  [n_text_layer][n_text_head][2][64] (K's 64, then V's). CrossKVQuantize: the quantise kernel alone on every slot of the handle.
 *  Both return -1 on a handle without the mode. */
AX_WHISPER_API int AX_WHISPER_GetCrossKVFp8(AX_WHISPER_HANDLE handle, int slot, uint8_t* k_codes, uint8_t* v_codes, float* scales);
AX_WHISPER_API int AX_WHISPER_CrossKVQuantize(AX_WHISPER_HANDLE handle);
/** Parity aid: scan every 16-bit tensor the engine keeps between kernels (encoder activations of clips 0..batch-1, cross and
 *  self K/V caches, the decoder's activation pairs) after EncodeMel / Decode*: names [n_max][32] chars, nonfinite [n_max]
 *  (NaN or Inf elements), maxabs [n_max] (largest finite |x|), *n_out buffers reported. A trained model's outlier channels
 *  and FFN peaks must stay inside the storage type's range (65504 for the fp16 build). */
AX_WHISPER_API int AX_WHISPER_ScanStored16(AX_WHISPER_HANDLE handle, int batch, int n_max, char* names, int64_t* nonfinite,
                                           float* maxabs, int* n_out);
/** Teacher-forced decode over the slots filled by EncodeMel: after the 4 SOT steps feed
 *  forced[b][0..n_forced-1]; logits: host [batch][n_forced+1][n_vocab] f32 (may be NULL);
 *  argmax_ids: host [batch][n_forced+1] (may be NULL). */
AX_WHISPER_API int AX_WHISPER_DecodeForced(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced,
                                           int n_forced, float* logits, int32_t* argmax_ids);
/** Greedy decode over the slots filled by EncodeMel (same loop as RunPCM*). */
AX_WHISPER_API int AX_WHISPER_DecodeGreedy(AX_WHISPER_HANDLE handle, int batch, int max_new,
                                           int32_t* ids, int* n_ids);
/** The same loop over a RAGGED batch: max_new_clip[b] (host, may be NULL; <= 0: none) caps the ids of clip b, so
 *  clips leave the loop at different steps the way real utterances reach eot at different steps
 *  (Whisper.cpp:219-222). A finished clip keeps its slot but no longer streams its K/V. */
AX_WHISPER_API int AX_WHISPER_DecodeGreedyRagged(AX_WHISPER_HANDLE handle, int batch, int max_new,
                                                 const int* max_new_clip, int32_t* ids, int* n_ids);
/** ids -> the text RunPCM* would have returned for them: detokenised bytes + the reference's zh post-pass (OpenCC t2s,
 *  Whisper.cpp:224-236) when its data files were found. *result is malloc'd; the caller frees it. */
AX_WHISPER_API int AX_WHISPER_Transcript(AX_WHISPER_HANDLE handle, const int32_t* ids, int n, char** result);

/* ---- additions: utterance slots that are refilled while the others decode (continuous batching) ---------------
 * The reference decodes ONE utterance per call and stops it at its own eot (Whisper.cpp:207-222); its server hands
 * requests to the handle one by one (WhisperHTTPServer.hpp:37-100). Here every utterance slot has its own decode offset,
 * so a slot whose clip has finished can take the next clip while the other slots decode on: no clip waits for the
 * slowest one of a micro-batch. Primary engine of the handle (one handle per GPU, as whisper_srv --devices runs them).
 *   StreamOpen(n_slots)  all slots idle; the batched entry points above are refused until StreamClose
 *   StreamAdmit(slot..)  front-end + encoder of one clip on a second stream into an idle slot's cross-K/V; the slot joins
 *                        the decode loop at the first StreamStep after its encoder has finished
 *   StreamStep(n_steps)  up to n decoder steps over all slots (captured step graph); finished slots are seen through
 *                        host-mapped flags between two steps (no wait), their successors join at once; returns the slots
 *                        that have finished
 *   StreamCollect(slot)  ids of a finished slot; the slot is idle again */
AX_WHISPER_API int AX_WHISPER_StreamOpen(AX_WHISPER_HANDLE handle, int n_slots);
/** max_new <= 0: until eot or the end of the context. pcm is copied before the call returns. -1 if the slot is busy. */
AX_WHISPER_API int AX_WHISPER_StreamAdmit(AX_WHISPER_HANDLE handle, int slot, const float* pcm, int num_samples, int max_new);
/** `count` clips at once into `count` idle slots (any slots, any order): one front-end + encoder pass for all of them —
 *  a batched pass costs a fraction of count one-clip passes. max_new may be NULL. -1 if any slot is busy (none admitted). */
AX_WHISPER_API int AX_WHISPER_StreamAdmitBatch(AX_WHISPER_HANDLE handle, const int* slots, const float* const* pcm,
                                               const int* num_samples, const int* max_new, int count);
/** finished_slots: host [n_slots]; *n_finished: how many were written. Slots stay "finished" until collected. */
AX_WHISPER_API int AX_WHISPER_StreamStep(AX_WHISPER_HANDLE handle, int n_steps, int* finished_slots, int* n_finished);
/** ids: host [n_text_ctx]. */
AX_WHISPER_API int AX_WHISPER_StreamCollect(AX_WHISPER_HANDLE handle, int slot, int32_t* ids, int* n_ids);
AX_WHISPER_API int AX_WHISPER_StreamClose(AX_WHISPER_HANDLE handle);

/* ---- segment timestamps (DESIGN.md "Segment timestamps")
 * Timestamp mode feeds [sot, <language>, transcribe] (no <|notimestamps|>) and applies Whisper's timestamp rules on the GPU at
 * every sampled step; ids then hold timestamp tokens: id timestamp_begin + k means k * 0.02 s, timestamp_begin =
 * AX_WHISPER_GetConfigInt(h, "timestamp_begin"). Needs n_vocab - timestamp_begin == 1501 (else -1, AX_WHISPER_LastError). */
/** RunPCMBatchTokens in timestamp mode; max_new_clip: optional [batch] per-clip budgets (<= 0: none), may be NULL. Sharded
 *  over the handle's devices. ids: host [batch][n_text_ctx]. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampTokens(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                         int batch, int max_new, const int* max_new_clip, int32_t* ids, int* n_ids);
/** DecodeForced in timestamp mode over the slots EncodeMel filled: logits (may be NULL) = the raw logits before the rules,
 *  [batch][n_forced+1][n_vocab]; chosen = the id the rules pick at each step, [batch][n_forced+1]. */
AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestamps(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                                     float* logits, int32_t* chosen);
/** The rules kernel alone on host data: logits [batch][n_vocab], hist [batch][n_text_ctx] with n_hist[b] sampled ids of clip b
 *  (prefix excluded) -> chosen [batch]. */
AX_WHISPER_API int AX_WHISPER_ApplyTimestampRules(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                                  int batch, int32_t* chosen);
/** Host only (no handle, no GPU): one clip's ids (eot excluded) -> at most n_max segments [start[k], end[k]] in seconds, text ids
 *  ids[tok_begin[k] .. tok_end[k]) (Transcript of that range is the segment's text); *n_seg = segments written.
 *  clip_seconds = min(num_samples / 16000, 30). n_max = n / 2 + 1 always suffices. */
AX_WHISPER_API int AX_WHISPER_SplitSegments(const int32_t* ids, int n, int timestamp_begin, int eot, float clip_seconds, int n_max,
                                            float* start, float* end, int* tok_begin, int* tok_end, int* n_seg);

/* ---- long-form: audio longer than 30 s (DESIGN.md "Long-form")
 * The file's log-mel is computed once over the whole file (reflect pad at the file's two ends, one maximum over all of its
 * frames) and kept in HBM; the window at `seek` (frames of 10 ms) is frames [seek, seek + 3000) of it, zero past the file's last
 * frame. The loop: while seek < num_samples / 160, decode the window in timestamp mode (every window starts fresh: no
 * conditioning on earlier text), cut it with the window rule, seek += advance. One pass decodes the current window of every
 * unfinished file side by side, in slots 0..A-1; more files than the handle's slots (max_batch of Init) wait for a place.
 * AX_WHISPER_FEATURE_MODE=openai has no long-form meaning: these calls refuse it. The PCM and log-mel stores of a call are
 * capped at AX_WHISPER_LONG_MAX_BYTES (default 4 GiB); a call beyond it returns -1 (AX_WHISPER_LastError). */
/** Host only (no handle, no GPU): the window rule. One window's ids (eot excluded), window_frames = min(3000, num_samples / 160 -
 *  seek) -> at most n_max segments (start / end in seconds relative to the window, text ids ids[tok_begin[k] .. tok_end[k]) as in
 *  SplitSegments) and *advance, the frames the next window starts later (1 .. window_frames). Consecutive timestamp pairs close
 *  segments; ids after the last pair belong to no segment (the next window decodes that audio again); an advance <= 0 (a pair
 *  closing at 0.00 s) becomes window_frames. n_max = n / 2 + 1 always suffices. */
AX_WHISPER_API int AX_WHISPER_SplitWindow(const int32_t* ids, int n, int timestamp_begin, int eot, int window_frames, int n_max,
                                          float* start, float* end, int* tok_begin, int* tok_end, int* n_seg, int* advance);
/** Stage level: whole-file front-end + window kernel for one file. mel_out: host [n_mels*3000] f32; seek 0 is bit-equal to
 *  AX_WHISPER_ComputeMel of the same input. */
AX_WHISPER_API int AX_WHISPER_ComputeMelWindow(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, int seek, float* mel_out);
/** The loop over n_files files; returns the raw log of every decoded window. Window k: win_info[k*7 .. k*7+6] = file index, seek,
 *  window_frames, advance, n_ids, pass, encoder slot; ids[k*n_text_ctx ..] = its n_ids ids (all of them, also those after the last
 *  boundary). max_new: per-window id budget (<= 0: until eot or the context end). max_passes (<= 0: none) stops after that many
 *  passes: the call returns 0 with the windows decoded so far, and slot s still holds the cross K/V of the last pass's window
 *  in slot s (AX_WHISPER_GetCrossKV). win_cap: windows the two arrays can take; too small -> -1 with the needed count in the
 *  error text and nothing written. With several devices the files are split in contiguous blocks, one per engine: the log holds
 *  the first engine's windows first, pass and slot are the engine's own. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindows(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                int max_new, int max_passes, int win_cap, int* win_info, int32_t* ids, int* n_windows);
/** Text of a whole file: the transcripts of the loop's segments, concatenated (zh post-pass as in Transcript). *result malloc'd. */
AX_WHISPER_API int AX_WHISPER_RunPCMLong(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, char** result);
AX_WHISPER_API int AX_WHISPER_RunFileLong(AX_WHISPER_HANDLE handle, const char* wav_file, char** result);

/* ---- confidence: token log-probabilities, no-speech, silent-window skipping (DESIGN.md "Confidence")
 * All in timestamp mode, natural logarithms, float32. At a sampled step the rules leave a final allowed set A (rules 1-5); the chosen
 * id c is the one timestamp mode picks, and its log-probability is x[c] - logsumexp(x[A]) (nothing finite left: -inf; x[c] = +inf: 0).
 * A clip that kept n ids has n + 1 decisions: one per id, plus the one that ended it (eot, or the id dropped at the budget / the
 * context end; ended_eot says which). avg_logprob = (sum of the n kept ids' values + the last one if it was eot) / (n + 1).
 * no_speech_logprob = x[no_speech] - logsumexp of the WHOLE row (NaN entries left out) at the step that fed sot;
 * no_speech = AX_WHISPER_GetConfigInt(h, "no_speech") (the config file's key, default no_timestamps - 1). The device value is the
 * LOG; the probability the thresholds compare is exp() of it, taken on the host. */
/** RunPCMBatchTimestampTokens (the same ids) + token_logprob [batch][n_text_ctx] (entries 0 .. n_ids[b], the rest 0), avg_logprob,
 *  no_speech_logprob, ended_eot [batch]. Sharded over the handle's devices. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampScores(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                         int batch, int max_new, const int* max_new_clip, int32_t* ids, int* n_ids,
                                                         float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot);
/** DecodeForcedTimestamps + logprob [batch][n_forced+1] of each step's chosen id, no_speech_logprob [batch] and (may be NULL)
 *  logits0 [batch][n_vocab]: the raw row of decode offset 0, which the no-speech value was taken from (`logits` starts at offset 2). */
AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampScores(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                                          float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob,
                                                          float* logits0);
/** ApplyTimestampRules + logprob [batch]: the scored rules kernel alone on host data. */
AX_WHISPER_API int AX_WHISPER_ScoreTimestampRules(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                                  int batch, int32_t* chosen, float* logprob);
/** The no-speech kernel alone on host data: logits [batch][n_vocab] -> out [batch]. */
AX_WHISPER_API int AX_WHISPER_NoSpeechLogProb(AX_WHISPER_HANDLE handle, const float* logits, int batch, float* out);
/** Host only (no handle, no GPU): the silent-window rule. 1 iff exp(no_speech_logprob) > no_speech_threshold and NOT
 *  (avg_logprob > logprob_threshold), else 0. logprob_threshold = +inf: no-speech alone decides; a NaN no_speech_threshold: never.
 *  openai-whisper's values are 0.6 and -1.0. */
AX_WHISPER_API int AX_WHISPER_LongWindowIsSilent(float no_speech_logprob, float avg_logprob, float no_speech_threshold,
                                                 float logprob_threshold);
/** RunPCMLongWindows under the silent-window rule: a window the rule calls silent emits no segment and advances by its
 *  window_frames. win_score[k*3 .. k*3+2] = no_speech_logprob, avg_logprob, skipped (0 / 1) of window k. A NaN
 *  no_speech_threshold switches the rule off: the windows are RunPCMLongWindows' own, with their scores. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsScored(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                      int n_files, int max_new, int max_passes, float no_speech_threshold,
                                                      float logprob_threshold, int win_cap, int* win_info, int32_t* ids, float* win_score,
                                                      int* n_windows);
/** RunPCMLong / RunFileLong under the silent-window rule (skipped windows add no text). */
AX_WHISPER_API int AX_WHISPER_RunPCMLongOpts(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                             float logprob_threshold, char** result);
AX_WHISPER_API int AX_WHISPER_RunFileLongOpts(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold,
                                              float logprob_threshold, char** result);

/* ---- temperature fallback: seeded sampling in the rules kernel, long-form retry (DESIGN.md "Temperature fallback")
 * Sampled decode mode is scored mode with a temperature t[b] and a random stream id per clip, and one seed per call. At a sampled
 * step of a clip with t > 0 the decision is drawn from softmax(x[A] / t) over the final allowed set A of rules 1-5 (openai-whisper's
 * Categorical(logits / temperature)), by Gumbel-max: c = argmax over A of x[i] / t - log(-log(u_i)), lowest id on ties, NaN logits
 * masked. u_i = ((w >> 9) + 0.5) * 2^-23 where w is word i & 3 of Philox4x32-10 with key (seed low, seed high) and counter
 * (i >> 2, n, stream low, stream high), n = the clip's history length: equal (seed, stream, n) give equal noise at any batch position,
 * in any batch, on any device. The rules themselves are decided on the untempered logits, and the recorded log-probability stays
 * the untempered x[c] - logsumexp(x[A]). A clip with t = 0 decides as scored mode does. Temperatures must be 0, or finite and >= 1e-6 (below that x / t
 * overflows float32 for ordinary logits; at any t a quotient that does overflow has key +-inf, and equal keys go to the lowest id). */
/** ScoreTimestampRules with temperature [batch], stream [batch] and seed: the sampled rules kernel alone on host data. Unlike
 *  ScoreTimestampRules, a batch above the handle's current capacity grows it: the slots' cross K/V of earlier calls is then lost. */
AX_WHISPER_API int AX_WHISPER_SampleTimestampRules(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                                   int batch, const float* temperature, const uint64_t* stream, uint64_t seed,
                                                   int32_t* chosen, float* logprob);
/** DecodeForcedTimestampScores in sampled mode: chosen [batch][n_forced+1] are the ids drawn at each step. */
AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampSampled(AX_WHISPER_HANDLE handle, int batch, const int32_t* forced, int n_forced,
                                                           const float* temperature, const uint64_t* stream, uint64_t seed,
                                                           float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob,
                                                           float* logits0);
/** RunPCMBatchTimestampScores in sampled mode. Sharded over the handle's devices; the stream ids are the caller's, so the
 *  results do not depend on the sharding. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampSampled(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                          int batch, int max_new, const int* max_new_clip, const float* temperature,
                                                          const uint64_t* stream, uint64_t seed, int32_t* ids, int* n_ids,
                                                          float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot);
/** Host only (no handle, no GPU): *ratio = n / (bytes of zlib's compress() at its default level), openai-whisper's
 *  compression_ratio; n = 0 gives 0 / 8 = 0. zlib's runtime library (libz.so.1) is loaded at first use; -1 (AX_WHISPER_LastError(NULL))
 *  when it is missing. */
AX_WHISPER_API int AX_WHISPER_CompressionRatio(const unsigned char* bytes, int n, float* ratio);
/** Host only: openai-whisper's fallback rule, in float32. 1 iff compression_ratio > compression_ratio_threshold or avg_logprob <
 *  logprob_threshold — but 0 when exp(no_speech_logprob) > no_speech_threshold and avg_logprob < logprob_threshold (a silent window
 *  is left to the silent-window rule). A NaN threshold switches its part off. openai-whisper's values are 2.4, -1.0 and 0.6. */
AX_WHISPER_API int AX_WHISPER_WindowNeedsFallback(float compression_ratio, float avg_logprob, float no_speech_logprob,
                                                  float compression_ratio_threshold, float logprob_threshold, float no_speech_threshold);
/** RunPCMLongWindowsScored with temperature fallback. Attempt a of a window is decoded at temperatures[a] (1 .. 16 values, the first
 *  usually 0; openai-whisper: 0, 0.2, .. 1.0), one sample each. The window's text is the raw bytes of its ids below eot with ASCII
 *  whitespace stripped at both ends; a window whose text and scores need fallback (WindowNeedsFallback) and that has attempts left
 *  does not advance: it is encoded and decoded again in the next pass. The last attempt is kept whatever it gives; the silent-window
 *  rule and the window rule then apply to the kept attempt. Every attempt is a log entry: win_score[k*7 .. k*7+6] = no_speech_logprob,
 *  avg_logprob, skipped, attempt, temperature, compression_ratio, kept (0 / 1); an attempt that is not kept has advance 0. The random
 *  stream of a window is (seek, file id * 16 + attempt). file_ids [n_files] (each 0 .. 2^27 - 1) are the caller's names for its files;
 *  NULL: a file's id is its index in this call. Equal (seed, file id) give a file the same windows beside any other files, at any
 *  position in the call and on any number of devices; with NULL that holds for a file at the same index only (a file moved to
 *  another index draws other noise). RunPCMLongFallback / RunFileLongFallback use file id 0. Not covered: best_of > 1, beam search inside this loop (RunPCMBatchBeam decodes single windows), the Stream* calls. Prompt conditioning and the prompt reset: RunPCMLongWindowsPrompted. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsFallback(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                        int n_files, int max_new, int max_passes, float no_speech_threshold,
                                                        float logprob_threshold, float compression_ratio_threshold,
                                                        const float* temperatures, int n_temperatures, uint64_t seed, const int* file_ids,
                                                        int win_cap, int* win_info, int32_t* ids, float* win_score, int* n_windows);
/** RunPCMLongOpts / RunFileLongOpts with temperature fallback: the text of the kept attempts. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongFallback(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                                 float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                 int n_temperatures, uint64_t seed, char** result);
AX_WHISPER_API int AX_WHISPER_RunFileLongFallback(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold,
                                                  float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                  int n_temperatures, uint64_t seed, char** result);

/* ---- prompt conditioning: prompt ids, a prefill pass, previous-text carry (DESIGN.md "Prompt conditioning")
 * A prompt is a list of ids (there is no text encoder here): text ids below eot and timestamp ids; any other id is an error. Of a
 * longer prompt the last n_text_ctx / 2 - 1 = 223 ids are used (openai-whisper's rule). A clip with P > 0 prompt ids decodes from the
 * context [sot_prev, p_1 .. p_P, sot, language, transcribe] instead of [sot, language, transcribe]; P = 0 means no prompt at all (no
 * sot_prev either): that clip decodes exactly as the unprompted calls decode it. Timestamp modes only. The context in front of
 * `transcribe` is computed in one prefill pass (AX_WHISPER_PREFILL=step: fed one position per decoder step instead, as is
 * every decoder shape the prefill kernels do not take; GetConfigInt "prefill" = the route the handle's prompted calls take, 0 the
 * pass, 1 step-fed; a value other than prefill / step makes the first prompted call fail); the decisions come from the same steps as without a prompt. A prompted clip ends at eot, at its budget, or
 * at the context end: at most n_text_ctx - 4 - P ids. Its no_speech_logprob is taken at the sot position of its context.
 * Not covered: prompts under beam search, in the Stream* calls and whisper_srv, best_of > 1, encoding prompt TEXT to ids. */
/** RunPCMBatchTimestampScores with prompt_ids [batch][prompt_stride] and n_prompt [batch] (0 .. prompt_stride). Sharded over the
 *  handle's devices; the prompts travel with their clips. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampPrompted(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                           int batch, int max_new, const int* max_new_clip, const int32_t* prompt_ids,
                                                           int prompt_stride, const int* n_prompt, int32_t* ids, int* n_ids,
                                                           float* token_logprob, float* avg_logprob, float* no_speech_logprob,
                                                           int* ended_eot);
/** Stage level (after EncodeMel of `batch` clips): the decode state of slots 0 .. batch-1 as the prompted loop finds it before its
 *  first step: reset, then every prompted slot's context cached and `transcribe` about to be fed. no_speech_logprob (may be NULL):
 *  [batch], 0 for slots without a prompt; sot_logits (may be NULL): [batch][n_vocab], the raw logits row of the sot position that
 *  value was taken from (zeros for slots without a prompt). */
AX_WHISPER_API int AX_WHISPER_PrefillPrompts(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids, int prompt_stride,
                                             const int* n_prompt, float* no_speech_logprob, float* sot_logits);
/** Rows 0 .. n_rows-1 of the slot's self-attention cache, de-blocked: k_out, v_out fp32 [n_text_layer][n_rows][n_text_state]. */
AX_WHISPER_API int AX_WHISPER_GetSelfKV(AX_WHISPER_HANDLE handle, int slot, int n_rows, float* k_out, float* v_out);
/** The self-attention cache of a later clip of the last two- or three-clip persistent launch (DecodeGreedy of 2 or 3 clips; clip 0's
 *  cache never leaves the chip). clip: 1 or 2, the clip's position in that launch. k_out, v_out: fp32
 *  [n_text_layer][512][n_text_state], all 8 blocks x 64 keys of every (layer, head) de-blocked, the 16-bit values widened exactly;
 *  rows no step of the launch wrote are zero. -1 with an error text when the handle holds no such cache
 *  (GetConfigInt "persistent_max_clips" <= clip). */
AX_WHISPER_API int AX_WHISPER_GetPersistentSelfKV(AX_WHISPER_HANDLE handle, int clip, float* k_out, float* v_out);
/** DecodeForcedTimestampScores under prompts (every clip needs one): forced [batch][n_forced] follow each clip's own context, row i
 *  of logits / chosen / logprob [batch][n_forced+1] is the step that decides id i. There is no row of decode offset 0. */
AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampPrompted(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids,
                                                            int prompt_stride, const int* n_prompt, const int32_t* forced, int n_forced,
                                                            float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob);
/** Host only (no handle, no GPU): one step of the previous-text carry, after a kept window. State: all_ids [n_all] (starts as the
 *  initial prompt ids) and reset_since. Unless `skipped`, the ids of the window's emitted segments are appended, timestamps
 *  included, from each segment's opening timestamp to its closing one (the ranges SplitWindow cuts; ids after the last closed pair
 *  and segments without text add nothing). Then, if condition_on_previous_text is 0 or temperature > 0.5, reset_since becomes the
 *  new length. all_out (cap >= n_all + n_window ids) takes the new list, *n_all_out its length; *n_prompt_next =
 *  min(*n_all_out - *reset_since_out, keep): the ids the next window is prompted with are the last that many (keep: 223). */
AX_WHISPER_API int AX_WHISPER_CarryPrompt(const int32_t* all_ids, int n_all, int reset_since, const int32_t* window_ids, int n_window,
                                          int timestamp_begin, int eot, int window_frames, int skipped, int condition_on_previous_text,
                                          float temperature, int keep, int cap, int32_t* all_out, int* n_all_out, int* reset_since_out,
                                          int* n_prompt_next);
/** RunPCMLongWindowsFallback under prompt conditioning, per file: all_ids starts as the file's initial prompt
 *  (initial_prompt_ids [n_files][prompt_stride], n_initial [n_files]; both may be NULL), a window's prompt is all_ids[reset_since:]
 *  (its last 223 ids; every fallback attempt of a window gets the same one), and CarryPrompt runs after every kept window with the
 *  kept attempt's temperature — the prompt reset of openai-whisper's loop. n_temperatures = 0 (temperatures may be NULL): no fallback,
 *  the scored loop, win_score rows have 3 entries; else 7 as in RunPCMLongWindowsFallback. win_prompt (may be NULL): [win_cap], the
 *  prompt length of every log entry. With no initial prompt and condition_on_previous_text = 0 the log is that of the unprompted call.
 *  "Emitted segment" differs from openai-whisper's list in one place: a segment is dropped here when it has no text id, there when
 *  its decoded text is blank or its start equals its end. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsPrompted(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples,
                                                        int n_files, int max_new, int max_passes, float no_speech_threshold,
                                                        float logprob_threshold, float compression_ratio_threshold,
                                                        const float* temperatures, int n_temperatures, uint64_t seed, const int* file_ids,
                                                        const int32_t* initial_prompt_ids, int prompt_stride, const int* n_initial,
                                                        int condition_on_previous_text, int win_cap, int* win_info, int32_t* ids,
                                                        float* win_score, int* win_prompt, int* n_windows);
/** RunPCMLongFallback / RunFileLongFallback under prompt conditioning (initial_prompt_ids [n_initial], may be NULL / 0). */
AX_WHISPER_API int AX_WHISPER_RunPCMLongPrompted(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                                 float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                 int n_temperatures, uint64_t seed, const int32_t* initial_prompt_ids, int n_initial,
                                                 int condition_on_previous_text, char** result);
AX_WHISPER_API int AX_WHISPER_RunFileLongPrompted(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold,
                                                  float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                                  int n_temperatures, uint64_t seed, const int32_t* initial_prompt_ids, int n_initial,
                                                  int condition_on_previous_text, char** result);

/* ---- language and task per clip: detection on the GPU, a language and a task per clip (DESIGN.md "Language and task per clip")
 * Languages are numbered by the config's all_language_codes, in file order: index j (0 .. n_lang-1, GetConfigInt "n_lang"; the
 * handle's own: GetConfigInt "lang_index"). A request is lang [batch]: >= 0 an index, -1 the handle's language, -2 detect it from the
 * clip; and task [batch]: 0 transcribe, 1 translate (refused when the config has no translate id). A NULL array means all -1 / all 0.
 * Detection is openai-whisper's detect_language: the logits of the position that fed sot (context [sot] alone, no prompt in front),
 * restricted to the language ids; lang_logprob [n_lang] = the language logits minus their logsumexp (float32, natural log; NaN
 * entries are left out and get -inf), the detected index is the first maximum in file order; when nothing is finite the handle's
 * language is detected and every value is -inf. A clip that detects, asks for another language than the handle's, for translate, or
 * has a prompt decodes behind the context ([sot_prev, prompt] +) [sot, language] with its task id fed next, through the prefill
 * hand-over of the prompted calls (AX_WHISPER_PREFILL=step: the step-fed route, detection included); any other clip decodes exactly
 * as the calls without a language decode it. Timestamp modes only.
 * Not covered: a language per request in whisper_srv and the Stream* calls (refused while a stream is open), under beam search and
 * in plain mode; detection from more than the first 30 s.
 * Text: the *Lang calls that return text run the zh Traditional-to-Simplified pass iff the CLIP's (file's) language is zh, whatever
 * the handle's language is (a handle of another language looks for t2s.json when its first zh text arrives). */
/** Host only. The index of a language code ("en", "zh", ...), -1 if the config does not list it. */
AX_WHISPER_API int AX_WHISPER_LanguageIndex(AX_WHISPER_HANDLE handle, const char* code);
/** Host only. The code of language `index` (valid until Uninit), NULL outside 0 .. n_lang-1. */
AX_WHISPER_API const char* AX_WHISPER_LanguageCode(AX_WHISPER_HANDLE handle, int index);
/** Front-end, encoder and detection of `batch` clips, nothing is decoded: lang_out [batch], lang_logprob (may be NULL)
 *  [batch][n_lang]. Sharded over the handle's devices. */
AX_WHISPER_API int AX_WHISPER_DetectLanguage(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                             int* lang_out, float* lang_logprob);
/** RunPCMBatchTimestampPrompted with lang / task [batch] (either may be NULL); n_prompt may be NULL (no clip is prompted). lang_out
 *  (may be NULL) [batch]: the index every clip was decoded under; lang_logprob (may be NULL) [batch][n_lang]: detecting clips, zeros
 *  for the others. Sharded over the handle's devices. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchTimestampLang(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                                       int max_new, const int* max_new_clip, const int32_t* prompt_ids, int prompt_stride,
                                                       const int* n_prompt, const int* lang, const int* task, int32_t* ids, int* n_ids,
                                                       float* token_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot,
                                                       int* lang_out, float* lang_logprob);
/** Stage level (after EncodeMel of `batch` clips): detection of slots 0 .. batch-1; lang_logprob and lang_logit (the raw language
 *  logits) [batch][n_lang] may be NULL. The decode state is left reset. */
AX_WHISPER_API int AX_WHISPER_DetectLanguageStage(AX_WHISPER_HANDLE handle, int batch, int* lang_out, float* lang_logprob, float* lang_logit);
/** The detection kernel alone on host rows [n][n_text_state] of the decoder's final residual stream (before the final LayerNorm):
 *  lang_logprob [n][n_lang], lang_index [n], lang_logit (may be NULL) [n][n_lang]. */
AX_WHISPER_API int AX_WHISPER_LanguageLogProbRows(AX_WHISPER_HANDLE handle, const float* rows, int n, float* lang_logprob, int* lang_index,
                                                  float* lang_logit);
/** PrefillPrompts with lang / task [batch] (n_prompt, lang, task may be NULL): every clip that needs a context has it cached and its
 *  task id about to be fed at offset L (2 without a prompt, P + 3 with one); check with GetSelfKV. lang_out, lang_logprob as above. */
AX_WHISPER_API int AX_WHISPER_PrefillContexts(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids, int prompt_stride, const int* n_prompt,
                                              const int* lang, const int* task, float* no_speech_logprob, float* sot_logits, int* lang_out,
                                              float* lang_logprob);
/** DecodeForcedTimestampPrompted with lang / task [batch]; here EVERY clip is handed over behind its context (prompted or not), so
 *  row i of logits / chosen / logprob [batch][n_forced+1] is the step that decides id i for all of them. */
AX_WHISPER_API int AX_WHISPER_DecodeForcedTimestampLang(AX_WHISPER_HANDLE handle, int batch, const int32_t* prompt_ids, int prompt_stride,
                                                        const int* n_prompt, const int* lang, const int* task, const int32_t* forced, int n_forced,
                                                        float* logits, int32_t* chosen, float* logprob, float* no_speech_logprob, int* lang_out);
/** Long-form under a language and task per FILE. RunPCMLongWindowsPrompted (always scored; fallback and prompts only if asked for:
 *  n_temperatures 0, n_initial NULL, NaN thresholds switch each part off) with lang / task [n_files] (either may be NULL) and
 *  lang_out (may be NULL) [n_files]: the index every file was decoded under. -2 detects on the file's window at seek 0 (as
 *  openai-whisper: once, on the first 30 s, also when that window is then skipped as silent); every later window of the file, and
 *  every further attempt of the first, uses the result. The window log is that of RunPCMLongWindowsPrompted (win_prompt may be
 *  NULL). A file without a window reports the index it asked for (the handle's where it asked for detection). */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsLang(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                    int max_new, int max_passes, float no_speech_threshold, float logprob_threshold,
                                                    float compression_ratio_threshold, const float* temperatures, int n_temperatures,
                                                    uint64_t seed, const int* file_ids, const int32_t* initial_prompt_ids, int prompt_stride,
                                                    const int* n_initial, int condition_on_previous_text, const int* lang, const int* task,
                                                    int win_cap, int* win_info, int32_t* ids, float* win_score, int* win_prompt,
                                                    int* n_windows, int* lang_out);
/** RunPCMLongPrompted / RunFileLongPrompted of one file under `lang` (>= 0, -1, -2) and `task` (0, 1); lang_out (may be NULL): the
 *  file's language index. The text follows that language (zh pass). */
AX_WHISPER_API int AX_WHISPER_RunPCMLongLang(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, float no_speech_threshold,
                                             float logprob_threshold, float compression_ratio_threshold, const float* temperatures,
                                             int n_temperatures, uint64_t seed, const int32_t* initial_prompt_ids, int n_initial,
                                             int condition_on_previous_text, int lang, int task, int* lang_out, char** result);
AX_WHISPER_API int AX_WHISPER_RunFileLongLang(AX_WHISPER_HANDLE handle, const char* wav_file, float no_speech_threshold, float logprob_threshold,
                                              float compression_ratio_threshold, const float* temperatures, int n_temperatures, uint64_t seed,
                                              const int32_t* initial_prompt_ids, int n_initial, int condition_on_previous_text, int lang,
                                              int task, int* lang_out, char** result);
/** Host only. The text of ids decoded under language `lang_index`: AX_WHISPER_Transcript whose zh pass follows that language. */
AX_WHISPER_API int AX_WHISPER_TranscriptLang(AX_WHISPER_HANDLE handle, const int32_t* ids, int n, int lang_index, char** result);

/** ---- Beam search (DESIGN.md "Beam search"): openai-whisper's BeamSearchDecoder over this project's timestamp rules.
 *  K = beam_size (1 .. 8) hypotheses ("ranks") per clip, each in a decoder slot of its own: clip c owns slots [c*K, c*K+K), so
 *  batch * K must not exceed the handle's max_batch (per device). Per step every live rank proposes the K+1 best ids of scored
 *  mode's final allowed set with x[c] - logsumexp(x[A]); the clip's candidates are ordered by float32 sum_logprob + logprob
 *  (descending; then parent rank, then position) and walked: the first K that are not eot become the new ranks, eot candidates met
 *  before the K-th become finished records (the parent's ids, the score) while the clip's pool holds fewer than K. A clip whose pool
 *  is full, or that has no live rank left, is complete; the loop ends when every clip is, or after max_new ids (one budget per call;
 *  0 or above n_text_ctx - 3: n_text_ctx - 3). Then live ranks fill a pool that is not full, in rank order, and the winner is the
 *  first record with the largest score / max(len, 1). K = 1 gives scored greedy mode's ids.
 *  Per clip: ids [batch][n_text_ctx] / n_ids (the winner's, no eot), sum_logprob, avg_logprob = sum_logprob / (n_ids + 1),
 *  no_speech_logprob (scored mode's, from the clip's first slot), ended_eot (1: the winner finished with eot, 0: it was cut at the
 *  budget). A clip without any record: n_ids 0, -inf. Sharded over the handle's devices like RunPCMBatchTokens.
 *  Not covered: best_of > 1, patience, a length penalty, per-clip budgets, the long-form loop, the Stream* calls. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchBeam(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                              int beam_size, int max_new, int32_t* ids, int* n_ids, float* sum_logprob,
                                              float* avg_logprob, float* no_speech_logprob, int* ended_eot);
/** Stage level (after EncodeMel of `batch` clips): the same decode over the encoded slots. Also every record of every clip, in
 *  pool order then fill order (each may be NULL): rec_ids [batch][K][n_text_ctx], rec_len / rec_score / rec_pool [batch][K]
 *  (rec_pool 1: from the pool), n_rec [batch], winner [batch] (index among the clip's records, -1: none).
 *  Trace (trace_cap > 0; every array may be NULL), for sampled step n < trace_cap over S = batch * K slots: tr_rows
 *  [trace_cap][S][n_vocab] the raw rows, tr_cand_id / tr_cand_logprob [trace_cap][S][K+1] and tr_n_cand [trace_cap][S] the
 *  candidates by slot, and after the step's selection tr_S / tr_slot [trace_cap][S] by rank (sum_logprob, -inf: dead; the rank's
 *  slot), tr_src [trace_cap][S] by slot (the slot its history and cache were taken from), tr_tok [trace_cap][S] by slot (the id
 *  appended to its history), tr_pool_n [trace_cap][batch]. *n_steps (may be NULL): sampled steps the loop ran (the completion
 *  counter is polled every 8 steps, so up to 16 steps run past the last completion; complete clips no longer change).
 *  With beam_size > 1 the call OVERWRITES the encoded slots: clip c's cross K/V is copied into slots c*K .. c*K+K-1, so slots
 *  1 .. batch*K-1 no longer hold what EncodeMel put there. Unlike the other stage-level Decode* calls it cannot be followed by
 *  another Decode* (DecodeBeam included) on the same encoder output: call EncodeMel again first. */
AX_WHISPER_API int AX_WHISPER_DecodeBeam(AX_WHISPER_HANDLE handle, int batch, int beam_size, int max_new, int32_t* ids, int* n_ids,
                                         float* sum_logprob, float* avg_logprob, float* no_speech_logprob, int* ended_eot,
                                         int32_t* rec_ids, int* rec_len, float* rec_score, int* rec_pool, int* n_rec, int* winner,
                                         int trace_cap, float* tr_rows, int32_t* tr_cand_id, float* tr_cand_logprob, int* tr_n_cand,
                                         float* tr_S, int* tr_slot, int* tr_src, int32_t* tr_tok, int* tr_pool_n, int* n_steps);
/** The candidates kernel alone: logits [rows][n_vocab], hist [rows][n_text_ctx] with n_hist[b] ids each -> the n_cand_max (1 .. 9)
 *  best ids of each row's final allowed set, value descending, lower id first on equal values: cand_id / cand_logprob
 *  [rows][n_cand_max] (entries from n_cand[b] on: eot, -inf), n_cand [rows]. */
AX_WHISPER_API int AX_WHISPER_BeamCandidates(AX_WHISPER_HANDLE handle, const float* logits, const int32_t* hist, const int* n_hist,
                                             int rows, int n_cand_max, int32_t* cand_id, float* cand_logprob, int* n_cand);
/** The selection kernel alone, on the caller's beam state (the handle gives the device only). n: history length before the step;
 *  stride: row stride of hist and pool_ids (n < stride). In: cand_id / cand_logprob [clips*K][K+1] and n_cand [clips*K] by slot, hist
 *  [clips*K][stride] by slot. In / out: S and slot [clips*K] by rank (slot: the ranks of clip c hold each of c*K .. c*K+K-1 once),
 *  pool_n [clips], pool_ids [clips*K][stride], pool_len / pool_score [clips*K], complete [clips]. Out: tok, src, slot_score
 *  [clips*K] by slot (the id for the history's index n; the reorder's source; S of the rank in the slot), *n_completed: clips that
 *  completed in this step. A surviving parent's best child stays in the parent's slot; the other children, then the dead ranks,
 *  take the clip's remaining slots in ascending order: no slot is both a source and a destination. */
AX_WHISPER_API int AX_WHISPER_BeamSelect(AX_WHISPER_HANDLE handle, int clips, int beam_size, int eot, int n, int stride,
                                         const int32_t* cand_id, const float* cand_logprob, const int* n_cand, const int32_t* hist,
                                         float* S, int* slot, int* pool_n, int32_t* pool_ids, int* pool_len, float* pool_score,
                                         int* complete, int32_t* tok, int* src, float* slot_score, int* n_completed);
/** Host only (no handle, no GPU): the fill and the ranking. In: the state after the loop (n: the histories' length; arrays as in
 *  BeamSelect). Out (each may be NULL): the records rec_ids [clips*K][stride], rec_len / rec_score / rec_pool [clips*K], n_rec
 *  [clips], winner [clips], and the winner's ids [clips][stride], n_ids, sum_logprob, avg_logprob, ended_eot [clips]. */
AX_WHISPER_API int AX_WHISPER_BeamFinalize(int clips, int beam_size, int n, int stride, const int32_t* hist, const float* S,
                                           const int* slot, const int* pool_n, const int32_t* pool_ids, const int* pool_len,
                                           const float* pool_score, int32_t* rec_ids, int* rec_len, float* rec_score, int* rec_pool,
                                           int* n_rec, int* winner, int32_t* ids, int* n_ids, float* sum_logprob, float* avg_logprob,
                                           int* ended_eot);

/** Host only (no handle, no GPU): the decode path Init picks for a decoder shape on a device with n_cu compute units, and the
 *  persistent launch's cross-attention role assignment, from the engine's own functions. plan4[0] = workgroups of the
 *  persistent launch, [1] = 1 iff the shape gets it (GetConfigInt "persistent_decode"), [2] = clips per launch
 *  ("persistent_max_clips"; 0 when [1] is 0), [3] = workgroups that own no self-attention head. units (may be NULL):
 *  [n_slots][plan4[0]], the cross-attention unit (clip * 3 * n_head + head * 3 + key range, or -1) of every workgroup in layer
 *  slots t0 .. t0 + n_slots - 1 (slot = step * n_layer + layer) of a launch with n_clips clips. -1 on bad arguments, or when
 *  units are asked for a launch the shape does not get. */
AX_WHISPER_API int AX_WHISPER_PersistentDecodePlan(int d_model, int n_head, int n_layer, int n_cu, int n_clips, int t0, int n_slots,
                                                   int* plan4, int* units);

/* ---- Word-level timestamps (DESIGN.md "Word-level timestamps"): openai-whisper's word_timestamps=True for one window. The cross-attention
 *  weights of a teacher-forced pass over [sot, language, task, notimestamps, text ids, eot] are normalised, median-filtered and averaged
 *  over the alignment heads; dynamic time warping on the result gives the frame (20 ms) at which every text token begins. */
/** Clips in, words out. ids [batch][n_text_ctx], n_ids [batch]: the greedy timestamp decode (AX_WHISPER_RunPCMBatchTimestampTokens'
 *  ids; under lang / task, either may be NULL, AX_WHISPER_RunPCMBatchTimestampLang's, lang_out [batch] or NULL the language index each
 *  clip was decoded under). Per clip b, with row stride n_max: n_segments[b] segments (AX_WHISPER_SplitSegments' of the ids), seg_start / seg_end [batch][n_max] in
 *  seconds AFTER the word rule has moved them; n_words[b] words: word_segment (index among those segments), word_start, word_end
 *  (seconds, rounded to 0.01), word_prob, and word_text_end: word w's bytes are text[b][word_text_end[w-1] .. word_text_end[w]) (0 for
 *  w = 0); text[b] is malloc'ed, the caller frees every non-NULL entry, also after a failure. jump [batch][n_text_ctx] and
 *  token_logprob [batch][n_text_ctx] (either may be NULL): what the words were made from, as AX_WHISPER_AlignTokens returns them for
 *  the clip's text ids (the ids below eot of its segments, in order). -1 when a clip has more than n_max words or segments. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchWordTimestamps(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int batch,
                                                        int max_new, const int* lang, const int* task, int32_t* ids, int* n_ids, int* lang_out,
                                                        int n_max, int* n_segments, double* seg_start, double* seg_end, int* n_words,
                                                        int* word_segment, int* word_text_end, double* word_start, double* word_end,
                                                        float* word_prob, char** text, int* jump, float* token_logprob);
/** Stage level, after AX_WHISPER_EncodeMel: the alignment of slots [0, batch). Clip b: n_ids[b] text ids (below eot) at ids + b * stride,
 *  num_frames[b] mel frames of its own (min(samples / 160, 3000): it aligns against num_frames[b] / 2 encoder frames), lang[b] (an index
 *  of the language list, -1 or a NULL array: the handle's), task[b] (0 transcribe, 1 translate; NULL: 0). Out: jump [batch][stride + 1]
 *  (n_ids[b] + 1 entries: the frame at which each text token, and the closing eot, begins), token_logprob [batch][stride] (log-softmax
 *  over the ids below eot), matrix (or NULL) [batch][m_rows][m_ld]: rows [0, n_ids[b] + 5) x frames [0, num_frames[b] / 2), the rest is
 *  not touched. A clip with n_ids[b] == 0 gets nothing; n_ids[b] + 5 > n_text_ctx is an error. The slots' self-attention caches are
 *  overwritten, nothing else a later decode reads. AX_WHISPER_WORD_ALIGN=host: normalisation, median and path on the host (the
 *  yardstick); GetConfigInt "word_align" = 0 the kernels, 1 the host. */
AX_WHISPER_API int AX_WHISPER_AlignTokens(AX_WHISPER_HANDLE handle, int batch, const int32_t* ids, int stride, const int* n_ids,
                                          const int* num_frames, const int* lang, const int* task, int* jump, float* token_logprob,
                                          float* matrix, int m_rows, int m_ld);
/** The token probabilities alone on host data (csrc/vocab_logprob.hip; DESIGN.md "Fused vocabulary log-probabilities"). x fp32
 *  [n_rows][n_text_state]: rows of the decoder's final residual stream (before the final LayerNorm); ids [n_rows], each in [0, eot).
 *  out[r] = logit[r][ids[r]] - logsumexp over columns [0, eot) of logit[r][.], logit = LayerNorm(x) . tied embedding^T.
 *  route 0 ("rows"): the logits launch four rows at a time, 64 logits rows written and one number read out of each, what AlignTokens
 *  and every one-window call use. route 1 ("fused"): LayerNorm into the 16-bit type, one MFMA launch over row tiles x vocabulary splits
 *  that keeps an online (max, sum) per row and never writes a logit, one merge launch; bit-identical from run to run; what the
 *  long-form word calls use. AX_WHISPER_WORD_LOGPROB=rows|fused overrides the route of every alignment (not of this call; a mistyped
 *  value fails the first alignment call); GetConfigInt "word_logprob" = 0 no override, 1 rows, 2 fused. */
AX_WHISPER_API int AX_WHISPER_VocabLogProbRows(AX_WHISPER_HANDLE handle, const float* x, int n_rows, const int32_t* ids, float* out, int route);
/** Host only: the fused route's tiling of n_rows rows of d_model over eot columns: plan3[0] rows per row tile, [1] vocabulary splits,
 *  [2] columns per split (split s covers columns [s * plan3[2], min((s + 1) * plan3[2], eot))). -1: a shape the kernel does not take
 *  (d_model a multiple of 128 up to 2048). */
AX_WHISPER_API int AX_WHISPER_VocabLogProbPlan(int d_model, int n_rows, int eot, int* plan3);
/** The alignment heads of a handle: n (layer, head) pairs; n == 0 restores what the handle was constructed with. That is the optional
 *  key "alignment_heads": [[layer, head], ...] of {type}_config.json (tools/convert_weights.py --hf copies it from the checkpoint's
 *  generation_config.json), else every head of the upper half of the layers. GetConfigInt "n_alignment_heads" counts the list in use. */
AX_WHISPER_API int AX_WHISPER_SetAlignmentHeads(AX_WHISPER_HANDLE handle, const int* pairs, int n);
/** Host only: the list a handle constructed from this config file starts with, as n (layer, head) pairs (at most n_max); -1 on a
 *  list that names a head the decoder does not have, names one twice or is not a list of pairs. */
AX_WHISPER_API int AX_WHISPER_ConfigAlignmentHeads(const char* config_path, int n_max, int* pairs, int* n);
/** Token suppression (DESIGN.md "Token suppression"): the handle's suppress set, n vocabulary ids (duplicates are fine). At every
 *  sampled step of timestamp mode an id of the set counts exactly as if its logit were -inf, before rules 2 to 5 and before
 *  anything is normalised: it is never rule 5's best text id, never part of the log-probabilities' normaliser, never drawn and never
 *  a beam candidate. Every timestamp-mode entry point picks the set up from the handle: the batch, scored, sampled, prompted, language,
 *  beam, long-form, chunked and word calls, a stream opened in mode 1, and the stage-level ApplyTimestampRules, ScoreTimestampRules,
 *  SampleTimestampRules, BeamCandidates, StreamRulesStage and DecodeForced*. Not filtered: no_speech_logprob, language detection,
 *  the word-timestamp token probabilities, plain mode. Ids of [0, eot) matter; ids of (eot, timestamp_begin) are accepted and have
 *  no effect (rule 1 masks them); -1 with an error text for eot, a timestamp id, an id outside the vocabulary, more than n_vocab
 *  entries, or while a stream is open (a stream opened afterwards uses the set). n == 0 restores what the handle was constructed
 *  with: the optional key "suppress_tokens": [ids ...] of {type}_config.json, where an entry -1 stands for NonSpeechTokens of the
 *  model's tokens file; absent or []: no set, and nothing this library computes or launches differs from a build without the
 *  feature. GetConfigInt "n_suppress_tokens" counts the set in use. With several devices every engine gets the set. */
AX_WHISPER_API int AX_WHISPER_SetSuppressTokens(AX_WHISPER_HANDLE handle, const int* ids, int n);
/** The set in use, sorted, duplicates dropped (at most n_max ids; -1 if there are more). */
AX_WHISPER_API int AX_WHISPER_GetSuppressTokens(AX_WHISPER_HANDLE handle, int n_max, int* ids, int* n);
/** Host only: openai-whisper's non_speech_tokens (what its suppress_tokens = -1 stands for) from a {type}-tokens.txt, sorted: the
 *  first id of " -" and " '", and for every symbol of its list the first id of the symbol and of " " + symbol where that is the
 *  whole encoding or the symbol is one of the musical signs; 82 ids for the multilingual vocabulary. -1 with an error text
 *  (AX_WHISPER_LastError(NULL)) where the file gives a needed byte no id. */
AX_WHISPER_API int AX_WHISPER_NonSpeechTokens(const char* tokens_path, int n_max, int* ids, int* n);
/** Host only: the set a handle constructed from this config file starts with (tokens_path is read only where the list holds -1 and
 *  may be NULL otherwise); -1 on a key that is not a list of ids or names an id that SetSuppressTokens refuses. */
AX_WHISPER_API int AX_WHISPER_ConfigSuppressTokens(const char* config_path, const char* tokens_path, int n_max, int* ids, int* n);
/** One alignment kernel alone on host data (the handle gives the device and the 16-bit type). Clip c has len[c] rows and n_keys[c] frames.
 *  QKSoftmax: q fp32 [rows][64 n_head] (clip c's rows from row0[c]), k fp32 [n_slots][n_head][keys_pad][64] (clip c reads slot[c]), both
 *  narrowed to the 16-bit type; heads [n_align]; P [n_clips][n_align][rows_pad][f_pad] in and out (f_pad a multiple of 64): row i < len[c],
 *  frames up to the end of the last 64-frame block are written, the rest keeps what it held.
 *  Normalize: matrix [n_clips][m_rows][m_ld] += inv_heads * (normalised, median-filtered P) summed over the n_align heads.
 *  DTW: jump [n_clips][jump_ld], len[c] - 4 entries per clip: the path over -matrix[c][3 .. len[c] - 2]. */
AX_WHISPER_API int AX_WHISPER_AlignQKSoftmax(AX_WHISPER_HANDLE handle, int n_clips, const int* len, const int* n_keys, const float* q, int rows,
                                             int n_head, const int* row0, const float* k, int n_slots, int keys_pad, const int* slot,
                                             const int* heads, int n_align, float* P, int rows_pad, int f_pad);
AX_WHISPER_API int AX_WHISPER_AlignNormalize(AX_WHISPER_HANDLE handle, int n_clips, const int* len, const int* n_keys, const float* P, int n_align,
                                             int rows_pad, int f_pad, float inv_heads, float* matrix, int m_rows, int m_ld);
AX_WHISPER_API int AX_WHISPER_AlignDTW(AX_WHISPER_HANDLE handle, int n_clips, const int* len, const int* n_keys, const float* matrix, int m_rows,
                                       int m_ld, int* jump, int jump_ld);
/** Host only: matrix [n_rows][n_frames] (row stride ld floats) -> jump [n_rows], the frame of the first path point of every row:
 *  dynamic time warping on -matrix with fp32 accumulation (one add per cell; ties go left), openai-whisper's dtw + backtrace. */
AX_WHISPER_API int AX_WHISPER_AlignPath(const float* matrix, int n_rows, int n_frames, int ld, int* jump);
/** Host only: openai-whisper's split_to_word_tokens over a tokens file. ids + language code -> word_tokens [n_words] (ids per word) and
 *  the words' bytes (text malloc'ed, word w ends at byte word_text_end[w]). An id at or above eot has no text and starts a word. */
AX_WHISPER_API int AX_WHISPER_SplitWords(const char* tokens_path, const int32_t* ids, int n, int eot, const char* language, int n_max,
                                         int* word_tokens, int* word_text_end, int* n_words, char** text, int* n_bytes);
/** Host only: the words of one window from its alignment: word split, word times from jump [n + 1], probabilities from token_logprob [n],
 *  merge_punctuations and the heuristics of openai-whisper's add_word_timestamps. ids: the n text ids of the window's n_seg segments
 *  in order, seg_tokens[s] of them in segment s; seg_start / seg_end are updated in place. Outputs as AX_WHISPER_RunPCMBatchWordTimestamps'. */
AX_WHISPER_API int AX_WHISPER_WordsFromAlignment(const char* tokens_path, const int32_t* ids, int n, int eot, const char* language,
                                                 const int* seg_tokens, double* seg_start, double* seg_end, int n_seg, const int* jump,
                                                 const float* token_logprob, double last_speech_timestamp, int n_max, int* word_segment,
                                                 int* word_text_end, double* word_start, double* word_end, float* word_prob, int* n_words,
                                                 char** text, int* n_bytes);

/** Host only: AX_WHISPER_WordsFromAlignment for a window that starts time_offset seconds into its file (long-form: seek / 100).
 *  Word times are round2(time_offset + jump / 50); seg_start / seg_end, last_speech_timestamp and the rule's max(0, .) clamps are all
 *  in FILE time, as openai-whisper's add_word_timestamps sees them inside transcribe(). time_offset 0: AX_WHISPER_WordsFromAlignment. */
AX_WHISPER_API int AX_WHISPER_WordsFromAlignmentAt(const char* tokens_path, const int32_t* ids, int n, int eot, const char* language,
                                                   const int* seg_tokens, double* seg_start, double* seg_end, int n_seg, const int* jump,
                                                   const float* token_logprob, double last_speech_timestamp, double time_offset, int n_max,
                                                   int* word_segment, int* word_text_end, double* word_start, double* word_end,
                                                   float* word_prob, int* n_words, char** text, int* n_bytes);

/* ---- Word timestamps in long-form (DESIGN.md "Word-level timestamps", "Words in the seek loop"): openai-whisper's
 *  transcribe(word_timestamps=True). After the decisions of a pass (fallback kept / not kept, silent skip, AX_WHISPER_SplitWindow)
 *  every kept, non-skipped window is aligned, one AlignTokens call per pass over the pass's slots, under the file's language and
 *  task, with the fused token probabilities (AX_WHISPER_VocabLogProbRows, route 1; AX_WHISPER_WORD_LOGPROB overrides). The word rule
 *  runs in file time with the file's last_speech_timestamp (0.0 at first, then the end of the last word of the last window that had
 *  one), and the seek moves by AX_WHISPER_LongWordAdvance. The prompt carry is unchanged: it takes ids, not times.
 *  Known limit: the alignment's GEMMs may add in another order when a pass holds more rows. Where a window's alignment matrix has
 *  near-ties, its word times can differ by a few frames between a file decoded alone and the same file beside others, and since the
 *  last word's end moves the seek, the file's later windows can then differ too ("Known limit").
 *  Not covered: hallucination_silence_threshold; words under beam search, in the Stream* calls and whisper_srv; the one-window calls
 *  (RunPCMBatchWordTimestamps, AlignTokens) keep the rows route of the token probabilities. */
/** Host only: the seek rule. ids [n]: one window's ids (eot excluded); seek, window_frames: the window's start and length in frames
 *  of 10 ms; split_advance: AX_WHISPER_SplitWindow's advance; has_word / last_word_end: whether the window yielded a word and the
 *  end of its last one in FILE time. Unless the ids end in a single timestamp (last id >= timestamp_begin, the one before below):
 *  if last_word_end > seek / 100, the new seek is round(last_word_end * 100) (nearest frame, ties to even). An advance <= 0 or
 *  > window_frames keeps split_advance (progress guard). *advance: the frames to move by; *by_word_end: 1 iff the word end was taken. */
AX_WHISPER_API int AX_WHISPER_LongWordAdvance(const int32_t* ids, int n, int timestamp_begin, int seek, int window_frames, int split_advance,
                                              int has_word, double last_word_end, int* advance, int* by_word_end);
/** The options of the long-form calls below: those of AX_WHISPER_RunPCMLongWindowsLang, under the same names and with the same
 *  meaning (NaN thresholds, n_temperatures 0, NULL arrays switch each part off; arrays hold one entry per file), plus word_timestamps
 *  (0: the loop as RunPCMLongWindowsLang runs it). */
typedef struct AX_WHISPER_LONG_OPTIONS {
  float no_speech_threshold, logprob_threshold, compression_ratio_threshold;
  const float* temperatures; int n_temperatures; uint64_t seed; const int* file_ids;
  const int32_t* initial_prompt_ids; int prompt_stride; const int* n_initial; int condition_on_previous_text;
  const int* lang; const int* task;
  int word_timestamps;
} AX_WHISPER_LONG_OPTIONS;
/** The word part of the window log, row k = window k of win_info. win_words [win_cap][4]: text ids aligned, segments, words, 1 iff
 *  the advance is the word-end seek. text_ids / token_logprob [win_cap][n_text_ctx] and jump [win_cap][n_text_ctx + 1]: the aligned
 *  ids (those below eot of SplitWindow's segments), the alignment's raw log-probabilities and jumps (ids + 1 entries). Packed in
 *  window order: seg_tokens / seg_start / seg_end [seg_cap] (ids of the segment among text_ids; the times the word rule left, FILE
 *  time), word_segment (index among the window's segments) / word_text_end / word_start / word_end / word_prob [word_cap]; word w's
 *  bytes are text[word_text_end[w-1] .. word_text_end[w]) (0 for the first word of the call). text is malloc'ed (the caller frees
 *  it, also after a failure). Windows that were skipped, not kept, or decoded with word_timestamps 0 have a zero row. */
typedef struct AX_WHISPER_LONG_WORD_LOG {
  int seg_cap, word_cap;
  int* win_words; int32_t* text_ids; int* jump; float* token_logprob;
  int* seg_tokens; double* seg_start; double* seg_end;
  int* word_segment; int* word_text_end; double* word_start; double* word_end; float* word_prob;
  char* text;
} AX_WHISPER_LONG_WORD_LOG;
/** RunPCMLongWindowsLang under `opts` with the full log: win_info, ids, win_score, win_prompt (may be NULL), n_windows, lang_out (may be
 *  NULL) as there; words (may be NULL when opts->word_timestamps is 0): the word log. -1 with "N windows were decoded" / "N segments" /
 *  "N words" in LastError when a capacity is too small; nothing but text is then written. Sharded over the handle's devices. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWindowsWords(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                     int max_new, int max_passes, const AX_WHISPER_LONG_OPTIONS* opts, int win_cap, int* win_info,
                                                     int32_t* ids, float* win_score, int* win_prompt, int* n_windows, int* lang_out,
                                                     AX_WHISPER_LONG_WORD_LOG* words);
/** One file's segments and words. Every array is malloc'ed by the call and released by AX_WHISPER_FreeLongWords. Segment k: seg_start /
 *  seg_end (seconds in the file, after the word rule), its text (the transcript of its ids, under the file's language) the bytes
 *  seg_text[seg_text_end[k-1] .. seg_text_end[k]); word w: word_segment (index among the file's segments), word_start, word_end,
 *  word_prob, its bytes in word_text likewise. */
typedef struct AX_WHISPER_LONG_WORDS {
  int n_segments, n_words;
  double* seg_start; double* seg_end; int* seg_text_end; char* seg_text;
  int* word_segment; double* word_start; double* word_end; float* word_prob; int* word_text_end; char* word_text;
} AX_WHISPER_LONG_WORDS;
/** Long-form transcription of one file (16 kHz mono PCM, or a wav file) with word timestamps, under `opts` (its arrays hold one entry;
 *  word_timestamps is taken as 1); lang_out (may be NULL): the file's language index. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongWords(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, const AX_WHISPER_LONG_OPTIONS* opts,
                                              int* lang_out, AX_WHISPER_LONG_WORDS* out);
AX_WHISPER_API int AX_WHISPER_RunFileLongWords(AX_WHISPER_HANDLE handle, const char* wav_file, const AX_WHISPER_LONG_OPTIONS* opts, int* lang_out,
                                               AX_WHISPER_LONG_WORDS* out);
AX_WHISPER_API void AX_WHISPER_FreeLongWords(AX_WHISPER_LONG_WORDS* out);

/** Stage timings of the last Run* / DecodeGreedy* call, ms (hipEvent): [0] front-end, [1] encoder,
 *  [2] decode loop, [3] whole call (wall), [4] decode steps executed. */
AX_WHISPER_API int AX_WHISPER_GetTimings(AX_WHISPER_HANDLE handle, float* out5);
/** Time `iters` launches of one named piece on the handle's stream with hipEvents; returns
 *  total ms in *ms_total. what: "decode_step" (one captured step graph at decode offset
 *  `arg`), "decode_step_ts" (the same step in timestamp mode), "decode_step_ts_scored" (in scored mode), "decode_step_ts_sampled" (in sampled mode, every clip at temperature
 *  $AX_WHISPER_BENCH_TEMPERATURE, default 1), "decode_step_beam" (the beam-search step of `batch` slots in groups of beam size `arg`,
 *  from decode offset 224 on, one offset further per iteration; afterwards GetConfigInt "beam_bench_moved_slots" / "beam_bench_iters" /
 *  "beam_bench_complete_clips" say how many slots the reorder launches copied in all, over how many iterations, and how many clips
 *  had completed), "encoder", "frontend", "frontend_long" (whole-file front-end of `batch`
 *  files of `arg` seconds + one window kernel), "long_cut_plan" (chunked long-form: levels kernel + plan kernels over `batch` resident
 *  files of `arg` seconds, default parameters), "prefill" (reset + PrefillPrompts of `batch` slots with prompts of arg - 3 ids each,
 *  i.e. context length L = arg, by the handle's route), "word_align" / "word_align_host" (AlignTokens of `batch` slots with `arg` text ids
 *  each against all frames, by the kernels / by the host route; host wall time), "word_logprob" / "word_logprob_rows" (the token
 *  probabilities of batch * arg residual rows alone, by the fused kernel / four rows per logits launch; host wall time), "resample" (the resample kernel over `batch` clips
 *  of 30 s at `arg` Hz into the staging rows), or a kernel name listed in DESIGN.md. */
AX_WHISPER_API int AX_WHISPER_Bench(AX_WHISPER_HANDLE handle, const char* what, int batch, int arg,
                                    int iters, float* ms_total);

/* ---- additions: audio at any sample rate (DESIGN.md "Sample rates") ------------------- */
/* Every entry point above takes 16 kHz mono PCM. The calls below take clips at their own rate and convert them to 16 kHz on the GPU
 * with a polyphase Kaiser-windowed sinc (csrc/resample.hpp: the definition; csrc/resample.hip: the kernel). Accepted: 1000 <= rate <=
 * 384000 Hz whose filter table has at most 2^22 entries (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000 all do;
 * 44101 does not), clips of at most 2^29 samples before and after. Everything else is refused with -1 and an error text
 * (AX_WHISPER_LastError) before any GPU work. A clip at 16000 Hz takes the path it always took. */

/** Host only: the length at 16 kHz of a clip of n samples at `rate`, ceil(n * 16000 / rate); -1 when the rate or the length is refused. */
AX_WHISPER_API long long AX_WHISPER_ResampledLength(long long n, int rate);
/** Host only: the filter of `rate` as the kernel uses it. *L phases, decimation *M, *K (2 K taps per phase); table (may be NULL: the
 *  sizes alone) receives the L * 2 K float32 coefficients [L][2 K] when cap >= L * 2 K. 0 ok, -1 refused rate or a table beyond cap. */
AX_WHISPER_API int AX_WHISPER_ResampleFilter(int rate, int* L, int* M, int* K, float* table, int cap);
/** The resample kernel alone on host data: out[b] (capacity out_cap[b] samples) receives the n_out[b] samples of clip b at 16 kHz.
 *  A clip at 16000 Hz is copied bit for bit. Batch-of-one calls serve long files. Refuses an open Stream*. */
AX_WHISPER_API int AX_WHISPER_ResampleBatch(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, const int* rates,
                                            int batch, float* const* out, const int* out_cap, int* n_out);
/** AX_WHISPER_ComputeMel of a clip at `rate`: upload, resample kernel into the staging row, front-end (the fused path of the calls below). */
AX_WHISPER_API int AX_WHISPER_ComputeMelRate(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, int rate, float* mel_out);
/** AX_WHISPER_RunPCMBatchTokens (mode 0) / AX_WHISPER_RunPCMBatchTimestampTokens (mode 1) with a sample rate per clip; sharded over
 *  the handle's devices like them, the rates travelling with their clips. */
AX_WHISPER_API int AX_WHISPER_RunPCMBatchRate(AX_WHISPER_HANDLE handle, int mode, const float* const* pcm, const int* num_samples,
                                              const int* rates, int batch, int max_new, int32_t* ids, int* n_ids);
/** AX_WHISPER_StreamAdmitBatch with a sample rate per clip (rates NULL: 16000 Hz). */
AX_WHISPER_API int AX_WHISPER_StreamAdmitBatchRate(AX_WHISPER_HANDLE handle, const int* slots, const float* const* pcm,
                                                   const int* num_samples, const int* rates, const int* max_new, int count);
/** AX_WHISPER_RunFile that resamples by the file's own rate (and prints no warning); a 16 kHz file gives what RunFile gives. */
AX_WHISPER_API int AX_WHISPER_RunFileResampled(AX_WHISPER_HANDLE handle, const char* wav_file, char** result);
/** File decode (AX_WHISPER_LoadAudioFile) + GPU resampling: *samples is a malloc'd 16 kHz mono buffer that every PCM entry point
 *  takes (long-form, fallback, prompted, language, beam, words); info (may be NULL): [0] the file's sample rate, [1] channels,
 *  [2] samples per channel in the file. */
AX_WHISPER_API int AX_WHISPER_LoadAudioFile16k(AX_WHISPER_HANDLE handle, const char* path, float** samples, int* n_samples, int* info);

/* ---- additions: chunked long-form (DESIGN.md "Chunked long-form"; csrc/long_cuts.hpp: the definitions) ------------------- */
/* The seek loop above decodes a file's windows one after the other, so one file fills one decoder slot. The calls below choose
 * every window of a file BEFORE decoding and decode them side by side, min(slots, remaining) per pass. A cut goes to the quietest
 * frame of a search range, chosen on the GPU from the file's own log-mel store (no voice-activity model):
 *   level of frame f        e[f] = mean over the mels of what the encoder will see, (max(S[f][m], G - 8) + 4) / 4
 *   smoothed level          s[f] = mean of e over [f - R, f + R], the index clamped to the file's 1 + num_samples / 160 frames
 *   cut rule                seek = 0; while content - seek > max_frames: among the even f in [seek + min_frames, seek + max_frames] the
 *                           smallest s[f] (fp32, exact; a tie goes to the largest f) ends the window (seek, f - seek), seek = f;
 *                           the last window is (seek, content - seek). content = num_samples / 160.
 * min_frames and max_frames are even, 2 <= min_frames <= max_frames <= 3000; smooth_frames R is 0 .. 64. A window's features are its
 * frames, zero from frame len on. The trade-off is that of every batched Whisper pipeline: windows are decoded independently (no
 * text of an earlier window, no seek feedback), and where a search range holds no quiet frame a word may straddle a cut. The seek
 * loop stays the default. Not covered, refused with a text in AX_WHISPER_LastError: language detection (lang -2), temperatures and
 * fallback, prompts and condition_on_previous_text, word timestamps, beam search, AX_WHISPER_FEATURE_MODE=openai. */
typedef struct AX_WHISPER_CHUNK_OPTIONS {
  int max_frames;     /* W_max, default 3000 */
  int min_frames;     /* W_min, default 2000 */
  int smooth_frames;  /* R, default 25 */
  int beam_size;      /* 1 (anything else is refused) */
} AX_WHISPER_CHUNK_OPTIONS;
/** Host only (no handle, no GPU): the cut rule on a caller's levels s [content] (finite). seek / len [win_cap] receive the windows,
 *  *n_windows their number (at most ceil(content / min_frames) + 1; content 0: none). -1 on bad parameters, non-finite levels or a
 *  win_cap too small (nothing written; the text in AX_WHISPER_LastError(NULL)). */
AX_WHISPER_API int AX_WHISPER_LongCutPlanHost(const float* s, int content, int min_frames, int max_frames, int win_cap, int* seek, int* len,
                                              int* n_windows);
/** Host only: one window's ids (eot excluded) -> its segments in FILE time. The split is AX_WHISPER_SplitSegments' with clip_seconds =
 *  len / 100 (the trailing piece is kept: no later window decodes that audio again); every time t becomes seek / 100 + min(t, len / 100). */
AX_WHISPER_API int AX_WHISPER_ChunkedSegments(const int32_t* ids, int n, int timestamp_begin, int eot, int seek, int len, int n_max, double* start,
                                              double* end, int* tok_begin, int* tok_end, int* n_seg);
/** Stage level: whole-file front-end + levels kernel over n_files files in one launch. e[b] / s[b] (either array, or an entry, may be
 *  NULL): host [1 + num_samples[b] / 160]. */
AX_WHISPER_API int AX_WHISPER_LongFrameLevels(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                              int smooth_frames, float* const* e, float* const* s);
/** Stage level: the plan kernel alone on a caller's levels, as AX_WHISPER_LongCutPlanHost (content >= 1). */
AX_WHISPER_API int AX_WHISPER_LongCutPlanFromLevels(AX_WHISPER_HANDLE handle, const float* s, int content, int min_frames, int max_frames,
                                                    int win_cap, int* seek, int* len, int* n_windows);
/** Stage level: front-end + levels + plan of n_files files in one call (chunk NULL: the defaults). n_windows [n_files]: windows per
 *  file; win_file / win_seek / win_len [win_cap]: all of them in the order file-then-seek; s (may be NULL, as may its entries): the
 *  levels the plan was made from, as in LongFrameLevels. -1 with "N windows were planned" in LastError when win_cap is too small. */
AX_WHISPER_API int AX_WHISPER_LongCutPlan(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                          const AX_WHISPER_CHUNK_OPTIONS* chunk, int win_cap, int* n_windows, int* win_file, int* win_seek,
                                          int* win_len, float* const* s);
/** Stage level: AX_WHISPER_ComputeMelWindow for a window of `len` frames (0 .. 3000): bit-equal to it on frames below len, zero from
 *  there on. */
AX_WHISPER_API int AX_WHISPER_ComputeMelWindowCut(AX_WHISPER_HANDLE handle, const float* pcm, int num_samples, int seek, int len, float* mel_out);
/** The chunked call over n_files files; the log is RunPCMLongWindows': window k: win_info[k*7 .. k*7+6] = file index, seek, window_frames,
 *  advance (both the window's length), n_ids, pass, encoder slot; ids[k*n_text_ctx ..]. Windows come in the order file-then-seek; pass p
 *  holds windows p * slots .. of that order in slots 0 .. A-1. chunk (NULL: the defaults); opts (NULL: none): no_speech_threshold /
 *  logprob_threshold (either not NaN, or win_score not NULL: the scored decode mode; win_score [win_cap][3] = no_speech_logprob,
 *  avg_logprob, 1 iff AX_WHISPER_LongWindowIsSilent drops the window's segments), lang (>= 0 or -1) and task per file; every other
 *  member must be off (see above). max_new, max_passes, win_cap and the sharding over several devices as in RunPCMLongWindows. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongChunkedWindows(AX_WHISPER_HANDLE handle, const float* const* pcm, const int* num_samples, int n_files,
                                                       int max_new, int max_passes, const AX_WHISPER_CHUNK_OPTIONS* chunk,
                                                       const AX_WHISPER_LONG_OPTIONS* opts, int win_cap, int* win_info, int32_t* ids,
                                                       float* win_score, int* n_windows);
/** Text of a whole file by the chunked call: the transcripts of AX_WHISPER_ChunkedSegments' segments of every window that was not
 *  dropped as silent, concatenated (under opts->lang[0] when given). *result malloc'd. */
AX_WHISPER_API int AX_WHISPER_RunPCMLongChunked(AX_WHISPER_HANDLE handle, float* pcm_data, int num_samples, const AX_WHISPER_CHUNK_OPTIONS* chunk,
                                                const AX_WHISPER_LONG_OPTIONS* opts, char** result);
AX_WHISPER_API int AX_WHISPER_RunFileLongChunked(AX_WHISPER_HANDLE handle, const char* wav_file, const AX_WHISPER_CHUNK_OPTIONS* chunk,
                                                 const AX_WHISPER_LONG_OPTIONS* opts, char** result);

/* ---- additions: the slot stream in timestamp mode (DESIGN.md "Slot stream in timestamp mode") --------------------------------- */
/* A stream opened in mode 1 decodes every slot in the scored timestamp mode: the prefix is the slot's own [sot, language, task]
 * (no <|notimestamps|>: the id budget without max_new is n_text_ctx - 3), the ids carry their timestamp tokens, and every slot keeps
 * the log-probability of each decision, log p(<|nospeech|>) and its language. A slot walks its own prefix step by step; with
 * lang -2 the language is picked on the GPU from the logits row of the step that fed sot (openai-whisper's detect_language) and
 * fed by the same step. One mode per open stream. Refused with a text in AX_WHISPER_LastError, the handle and an open stream staying
 * usable: an unknown mode; lang / task arrays or StreamCollectScored on a mode-0 stream; a language index outside [-2, n_lang); a
 * task other than 0 or 1; translate without a `translate` id in the config; detection on a config that lists one language.
 * Not covered in slots: sampling and fallback, prompts, beam search, word timestamps. GetConfigInt "stream_mode": the open stream's. */
/** AX_WHISPER_StreamOpen with a mode: 0 the plain greedy decode in the handle's language (exactly StreamOpen), 1 scored timestamps. */
AX_WHISPER_API int AX_WHISPER_StreamOpenMode(AX_WHISPER_HANDLE handle, int n_slots, int mode);
/** AX_WHISPER_StreamAdmitBatchRate with a language and task per clip (mode-1 stream): lang[i] >= 0 an index of the config's language
 *  list, -1 the handle's language, -2 detect; task[i] 0 transcribe, 1 translate. rates, max_new, lang and task may each be NULL
 *  (16000 Hz, no budget, all -1, all 0). None admitted when any clip is refused. */
AX_WHISPER_API int AX_WHISPER_StreamAdmitBatchLang(AX_WHISPER_HANDLE handle, const int* slots, const float* const* pcm, const int* num_samples,
                                                   const int* rates, const int* max_new, const int* lang, const int* task, int count);
/** AX_WHISPER_StreamCollect of a mode-1 stream with the slot's scores: token_logprob host [n_text_ctx] (entries 0 .. *n_ids: one per
 *  kept id and the decision that ended the clip; the rest 0), *avg_logprob, *no_speech_logprob, *ended_eot as
 *  AX_WHISPER_RunPCMBatchTimestampScores defines them; *lang_out the language index the clip was decoded under; lang_logprob host
 *  [n_lang]: a detecting clip's language log-probabilities, zeros otherwise. Everything but ids and n_ids may be NULL. */
AX_WHISPER_API int AX_WHISPER_StreamCollectScored(AX_WHISPER_HANDLE handle, int slot, int32_t* ids, int* n_ids, float* token_logprob,
                                                  float* avg_logprob, float* no_speech_logprob, int* ended_eot, int* lang_out,
                                                  float* lang_logprob);
/** Stage level: the stream's rules kernel alone on host data, n slots. rows [n][n_vocab]; off, done, detect [n]; hist [n][n_text_ctx]
 *  with n_hist [n] ids each. In/out, written only where the kernel writes (a caller's sentinel stays elsewhere): slot_ctx [n][4],
 *  chosen and logprob [n] (a slot at offset >= 2: AX_WHISPER_ScoreTimestampRules' decision), no_speech [n], lang_out [n],
 *  lang_logprob [n][n_lang]. A slot with done set is not touched; offset 0 writes no_speech and, with detect, the language outputs and
 *  slot_ctx[4 b + 1]; offset 1 writes nothing. Refuses an open Stream*. */
AX_WHISPER_API int AX_WHISPER_StreamRulesStage(AX_WHISPER_HANDLE handle, int n, const float* rows, const int* off, const int* done,
                                               const int* detect, const int32_t* hist, const int* n_hist, int* slot_ctx, int32_t* chosen,
                                               float* logprob, float* no_speech, int* lang_out, float* lang_logprob);

#ifdef __cplusplus
}
#endif

#endif /* _AX_WHISPER_API_H_ */
