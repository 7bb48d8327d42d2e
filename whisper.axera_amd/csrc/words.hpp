// words.hpp — the host side of word-level timestamps (DESIGN.md "Word-level timestamps"): the alignment path of a token x frame
// matrix (openai-whisper timing.py's dtw + the jump times of find_alignment), the word split of its tokenizer, merge_punctuations and
// the heuristics of add_word_timestamps. Host only, dtype-independent: api.cpp (AX_WHISPER_AlignPath, AX_WHISPER_SplitWords,
// AX_WHISPER_WordsFromAlignment) uses it; tests/word_reference.py states the same rules in Python.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "align_path.hpp"
#include "host_io.hpp"

namespace axw {

// matrix [n_rows][n_frames] (row stride ld) -> jump [n_rows]: dynamic time warping on -matrix, costs accumulated in fp32 with one
// add per cell, so the result is that of a numpy float32 evaluation.
inline void align_path(const float* matrix, int n_rows, int n_frames, long ld, int* jump) {
  if (n_rows < 1 || n_frames < 1) throw std::runtime_error("align_path: the matrix needs a row and a frame");
  const long W = (long)n_frames + 1;
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float> prev(W, inf), cur(W, inf);
  std::vector<uint8_t> trace((size_t)(n_rows + 1) * W, kTraceLeft);
  prev[0] = 0.f;
  for (int i = 1; i <= n_rows; ++i) {
    cur[0] = inf;
    const float* x = matrix + (long)(i - 1) * ld;
    for (int j = 1; j <= n_frames; ++j) {
      const float c0 = prev[j - 1], c1 = prev[j], c2 = cur[j - 1];
      const uint8_t t = dtw_choice(c0, c1, c2);
      cur[j] = -x[j - 1] + (t == kTraceDiag ? c0 : t == kTraceUp ? c1 : c2);
      trace[(long)i * W + j] = t;
    }
    std::swap(prev, cur);
  }
  dtw_backtrace(trace.data(), n_rows, n_frames, jump);
}

// What align_normalize_kernel (decode_align.hip) does for one clip and the heads of one layer, in its order of operations (four
// partial sums by row % 4, fused multiply-adds where the kernel has them), so that both routes build the same matrix:
// matrix[i][f] += inv_heads * median of 7 along f (reflect padding; skipped at F <= 3) of (P[a][i][f] - mean_f) / std_f.
inline void align_normalize_host(const float* P, int rows_pad, int f_pad, int n_align, int L, int F, float* matrix, long m_ld, float inv_heads) {
  std::vector<float> mean(F), sd(F);
  for (int a = 0; a < n_align; ++a) {
    const float* Pa = P + (long)a * rows_pad * f_pad;
    for (int f = 0; f < F; ++f) {
      float part[4] = {0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < L; ++r) part[r & 3] += Pa[(long)r * f_pad + f];
      mean[f] = (part[0] + part[1] + part[2] + part[3]) / (float)L;
      float sq[4] = {0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < L; ++r) {
        const float d = Pa[(long)r * f_pad + f] - mean[f];
        sq[r & 3] = std::fma(d, d, sq[r & 3]);
      }
      sd[f] = std::sqrt((sq[0] + sq[1] + sq[2] + sq[3]) / (float)L);
    }
    for (int r = 0; r < L; ++r)
      for (int f = 0; f < F; ++f) {
        float z;
        if (F > 3) {
          float v[7];
          for (int k = 0; k < 7; ++k) {
            int q = f + k - 3;
            if (q < 0) q = -q;
            if (q >= F) q = 2 * (F - 1) - q;
            v[k] = (Pa[(long)r * f_pad + q] - mean[q]) / sd[q];
          }
          std::nth_element(v, v + 3, v + 7);
          z = v[3];
        } else {
          z = (Pa[(long)r * f_pad + f] - mean[f]) / sd[f];
        }
        float& out = matrix[(long)r * m_ld + f];
        out = std::fma(z, inv_heads, out);
      }
  }
}

// ------------------------------------------------------------------------------ alignment heads
// The (layer, head) pairs the alignment averages over, sorted; every pair a head of the decoder, none twice.
inline std::vector<std::pair<int, int>> checked_alignment_heads(const int* pairs, int n, int n_layer, int n_head, const char* what) {
  std::vector<std::pair<int, int>> v;
  for (int i = 0; i < n; ++i) {
    const int l = pairs[2 * i], h = pairs[2 * i + 1];
    if (l < 0 || l >= n_layer || h < 0 || h >= n_head)
      throw std::runtime_error(std::string(what) + ": (" + std::to_string(l) + ", " + std::to_string(h) + ") is not a head of the decoder");
    v.emplace_back(l, h);
  }
  std::sort(v.begin(), v.end());
  if (std::adjacent_find(v.begin(), v.end()) != v.end()) throw std::runtime_error(std::string(what) + ": a head is listed twice");
  return v;
}
// openai-whisper's default for a checkpoint that names none: every head of the upper half of the layers
inline std::vector<std::pair<int, int>> default_alignment_heads(int n_layer, int n_head) {
  std::vector<std::pair<int, int>> v;
  for (int l = 0; l < n_layer; ++l)
    if (2 * l >= n_layer)
      for (int h = 0; h < n_head; ++h) v.emplace_back(l, h);
  return v;
}
// The optional key "alignment_heads": [[layer, head], ...] of {type}_config.json (tools/convert_weights.py --hf copies it from the
// checkpoint's generation_config.json) -> the checked list; absent or empty: an empty list (the default applies).
inline std::vector<std::pair<int, int>> config_alignment_heads(const JsonValue& j, int n_layer, int n_head) {
  if (!j.has("alignment_heads")) return {};
  const JsonValue& a = j.at("alignment_heads");
  if (a.kind != JsonValue::Array) throw std::runtime_error("config: alignment_heads must be a list of [layer, head] pairs");
  std::vector<int> flat;
  for (const JsonValue& p : a.arr) {
    if (p.kind != JsonValue::Array || p.arr.size() != 2 || p.arr[0].kind != JsonValue::Number || p.arr[1].kind != JsonValue::Number)
      throw std::runtime_error("config: alignment_heads must be a list of [layer, head] pairs");
    flat.push_back((int)p.arr[0].as_int());
    flat.push_back((int)p.arr[1].as_int());
  }
  return checked_alignment_heads(flat.data(), (int)flat.size() / 2, n_layer, n_head, "config: alignment_heads");
}

// ------------------------------------------------------------------------------ text
// Strict UTF-8, as Python's bytes.decode("utf-8"): no overlong forms, no surrogates, nothing above U+10FFFF, nothing cut short.
inline bool utf8_well_formed(const std::string& s) {
  const size_t n = s.size();
  for (size_t i = 0; i < n;) {
    const unsigned char c = (unsigned char)s[i];
    int len;
    unsigned lo = 0x80, hi = 0xBF;
    if (c < 0x80) { ++i; continue; }
    else if (c >= 0xC2 && c <= 0xDF) len = 2;
    else if (c >= 0xE0 && c <= 0xEF) { len = 3; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { len = 4; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    else return false;
    if (i + len > n) return false;
    for (int k = 1; k < len; ++k) {
      const unsigned char b = (unsigned char)s[i + k];
      if (b < (k == 1 ? lo : 0x80u) || b > (k == 1 ? hi : 0xBFu)) return false;
    }
    i += len;
  }
  return true;
}

// the code points of well-formed UTF-8
inline std::vector<uint32_t> utf8_code_points(const std::string& s) {
  std::vector<uint32_t> out;
  for (size_t i = 0; i < s.size();) {
    const unsigned char c = (unsigned char)s[i];
    const int len = c < 0x80 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
    uint32_t v = len == 1 ? c : c & (0xFF >> (len + 1));
    for (int k = 1; k < len && i + k < s.size(); ++k) v = (v << 6) | ((unsigned char)s[i + k] & 0x3F);
    out.push_back(v);
    i += len;
  }
  return out;
}

// what Python's str.strip() removes
inline bool is_py_space(uint32_t c) {
  return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20) || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
         c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

// The one code point that is left of `text` after Python's strip() (strip = false: of `text` as it is), or 0 when that is not
// exactly one code point.
inline uint32_t single_code_point(const std::string& text, bool strip) {
  std::vector<uint32_t> cp = utf8_code_points(text);
  size_t a = 0, b = cp.size();
  if (strip) {
    while (a < b && is_py_space(cp[a])) ++a;
    while (b > a && is_py_space(cp[b - 1])) --b;
  }
  return b - a == 1 ? cp[a] : 0;
}

inline bool in_set(uint32_t c, const uint32_t* set, size_t n) { return c != 0 && std::find(set, set + n, c) != set + n; }

inline bool is_ascii_punctuation(uint32_t c) { return (c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E); }

// "'“¿([{-   and   "'.。,，!！?？:：”)]}、   and   .。!！?？
constexpr uint32_t kPrependPunct[] = {0x22, 0x27, 0x201C, 0xBF, 0x28, 0x5B, 0x7B, 0x2D};
constexpr uint32_t kAppendPunct[] = {0x22, 0x27, 0x2E, 0x3002, 0x2C, 0xFF0C, 0x21, 0xFF01, 0x3F, 0xFF1F, 0x3A, 0xFF1A, 0x201D, 0x29, 0x5D, 0x7D, 0x3001};
constexpr uint32_t kSentenceEnd[] = {0x2E, 0x3002, 0x21, 0xFF01, 0x3F, 0xFF1F};
template <size_t N>
inline bool in_set(uint32_t c, const uint32_t (&set)[N]) { return in_set(c, set, N); }

struct WordTokens {
  std::string text;
  std::vector<int32_t> tokens;
};

inline bool language_without_spaces(const std::string& lang) {
  for (const char* l : {"zh", "ja", "th", "lo", "my", "yue"})
    if (lang == l) return true;
  return false;
}

// openai-whisper's split_to_word_tokens. An id at or above eot (or outside the table) has no text. The unicode split extends a group
// of consecutive ids until its bytes are well-formed UTF-8 (ids left over at the end are dropped); for a language written with
// spaces a group joins the word before it unless its first id is >= eot, its text starts with a space, its stripped text is one
// ASCII punctuation character, or it is the first group.
inline std::vector<WordTokens> split_words(const std::vector<std::string>& table, const int32_t* ids, int n, int eot, const std::string& lang) {
  std::vector<WordTokens> groups;
  WordTokens cur;
  for (int i = 0; i < n; ++i) {
    cur.tokens.push_back(ids[i]);
    if (ids[i] >= 0 && ids[i] < eot && (size_t)ids[i] < table.size()) cur.text += table[(size_t)ids[i]];
    if (utf8_well_formed(cur.text)) {
      groups.push_back(std::move(cur));
      cur = WordTokens{};
    }
  }
  if (language_without_spaces(lang)) return groups;
  std::vector<WordTokens> words;
  for (WordTokens& g : groups) {
    const bool special = g.tokens[0] >= eot, with_space = !g.text.empty() && g.text[0] == ' ';
    const bool punctuation = is_ascii_punctuation(single_code_point(g.text, true));
    if (special || with_space || punctuation || words.empty()) {
      words.push_back(std::move(g));
    } else {
      words.back().text += g.text;
      words.back().tokens.insert(words.back().tokens.end(), g.tokens.begin(), g.tokens.end());
    }
  }
  return words;
}

struct WordTiming {
  std::string text;
  std::vector<int32_t> tokens;
  double start = 0, end = 0, probability = 0;
};

// openai-whisper's merge_punctuations: text and tokens move, times do not
inline void merge_punctuations(std::vector<WordTiming>& a) {
  const int n = (int)a.size();
  for (int i = n - 2, j = n - 1; i >= 0; --i) {
    WordTiming &prev = a[i], &next = a[j];
    if (!prev.text.empty() && prev.text[0] == ' ' && in_set(single_code_point(prev.text, true), kPrependPunct)) {
      next.text = prev.text + next.text;
      next.tokens.insert(next.tokens.begin(), prev.tokens.begin(), prev.tokens.end());
      prev.text.clear();
      prev.tokens.clear();
    } else {
      j = i;
    }
  }
  for (int i = 0, j = 1; j < n; ++j) {
    WordTiming &prev = a[i], &next = a[j];
    if (!(!prev.text.empty() && prev.text.back() == ' ') && in_set(single_code_point(next.text, false), kAppendPunct)) {
      prev.text += next.text;
      prev.tokens.insert(prev.tokens.end(), next.tokens.begin(), next.tokens.end());
      next.text.clear();
      next.tokens.clear();
    } else {
      i = j;
    }
  }
}

// Python's round(x, 2): the nearest two-decimal number to the exact binary value, ties to even, read back as a double
inline double round2(double x) {
  if (!std::isfinite(x)) return x;
  char buf[512];
  snprintf(buf, sizeof buf, "%.2f", x);
  return strtod(buf, nullptr);
}

struct WordOut {
  int segment;
  std::string text;
  double start, end, probability;
};

// find_alignment's words from the path + add_word_timestamps of one window. ids: the n text ids (< eot) of the window's segments
// in order, seg_tokens[s] of them in segment s; jump [n + 1] frames of 20 ms, logprob [n]; seg_start / seg_end are updated in place.
// time_offset: the window's start in the file, seconds (long-form: seek / 100). Word times are round2(time_offset + jump / 50);
// seg_start / seg_end, last_speech_timestamp and the max(0, .) clamps are then all in file time, as openai-whisper's
// add_word_timestamps sees them inside transcribe(). The word durations (median, sentence-end cut) are taken before the offset.
inline std::vector<WordOut> words_from_alignment(const std::vector<std::string>& table, const int32_t* ids, int n, int eot, const std::string& lang,
                                                 const int* seg_tokens, double* seg_start, double* seg_end, int n_seg, const int* jump,
                                                 const float* logprob, double last_speech_timestamp, double time_offset = 0.0) {
  std::vector<WordOut> out;
  if (n_seg == 0) return out;
  long total = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (seg_tokens[s] < 0) throw std::runtime_error("words_from_alignment: negative token count");
    total += seg_tokens[s];
  }
  if (total != n) throw std::runtime_error("words_from_alignment: the segments' token counts do not add up to the ids");
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= eot) throw std::runtime_error("words_from_alignment: id " + std::to_string(ids[i]) + " is not text");
  std::vector<WordTiming> al;
  if (n > 0) {
    std::vector<int32_t> with_eot(ids, ids + n);
    with_eot.push_back(eot);
    std::vector<WordTokens> words = split_words(table, with_eot.data(), n + 1, eot, lang);
    // the eot pseudo-word closes the list unless the ids end in an unfinished character: that group swallows eot and is dropped
    if (!words.empty() && words.back().tokens[0] == eot) words.pop_back();
    if (!words.empty()) {
      int b = 0;
      for (WordTokens& w : words) {
        const int e = b + (int)w.tokens.size();
        WordTiming t;
        t.start = jump[b] / 50.0;
        t.end = jump[e] / 50.0;
        double sum = 0;
        for (int i = b; i < e; ++i) sum += std::exp((double)logprob[i]);
        t.probability = sum / (e - b);
        t.text = std::move(w.text);
        t.tokens = std::move(w.tokens);
        al.push_back(std::move(t));
        b = e;
      }
    }
  }
  std::vector<double> dur;
  for (const WordTiming& t : al)
    if (t.end - t.start != 0) dur.push_back(t.end - t.start);
  double median = 0;
  if (!dur.empty()) {
    std::sort(dur.begin(), dur.end());
    const size_t m = dur.size() / 2;
    median = dur.size() % 2 ? dur[m] : (dur[m - 1] + dur[m]) / 2;
  }
  median = std::min(0.7, median);
  const double max_duration = median * 2;
  if (!dur.empty())
    for (size_t i = 1; i < al.size(); ++i)
      if (al[i].end - al[i].start > max_duration) {
        if (in_set(single_code_point(al[i].text, false), kSentenceEnd)) al[i].end = al[i].start + max_duration;
        else if (in_set(single_code_point(al[i - 1].text, false), kSentenceEnd)) al[i].start = al[i].end - max_duration;
      }
  merge_punctuations(al);

  size_t wi = 0;
  for (int s = 0; s < n_seg; ++s) {
    int saved = 0;
    const size_t first = out.size();
    while (wi < al.size() && saved < seg_tokens[s]) {
      const WordTiming& t = al[wi];
      if (!t.text.empty()) out.push_back(WordOut{s, t.text, round2(time_offset + t.start), round2(time_offset + t.end), t.probability});
      saved += (int)t.tokens.size();
      ++wi;
    }
    const size_t nw = out.size() - first;
    if (nw == 0) continue;
    WordOut* w = out.data() + first;
    WordOut& last = w[nw - 1];
    // the first and second word after a pause are not longer than twice the median word duration
    if (w[0].end - last_speech_timestamp > median * 4 &&
        (w[0].end - w[0].start > max_duration || (nw > 1 && w[1].end - w[0].start > max_duration * 2))) {
      if (nw > 1 && w[1].end - w[1].start > max_duration) {
        const double boundary = std::max(w[1].end / 2, w[1].end - max_duration);
        w[0].end = w[1].start = boundary;
      }
      w[0].start = std::max(0.0, w[0].end - max_duration);
    }
    // prefer the segment-level start if the first word is too long
    if (seg_start[s] < w[0].end && seg_start[s] - 0.5 > w[0].start) w[0].start = std::max(0.0, std::min(w[0].end - median, seg_start[s]));
    else seg_start[s] = w[0].start;
    // prefer the segment-level end if the last word is too long
    if (seg_end[s] > last.start && seg_end[s] + 0.5 < last.end) last.end = std::max(last.start + median, seg_end[s]);
    else seg_end[s] = last.end;
    last_speech_timestamp = seg_end[s];
  }
  return out;
}

}  // namespace axw
