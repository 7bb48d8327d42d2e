// suppress.hpp — token suppression on the host (DESIGN.md "Token suppression"): which ids a suppress set may hold, the list that
// openai-whisper's suppress_tokens = -1 stands for, the config key, and the bitmask the rules kernels read (decode_rules.hpp).
// Header-only and free of HIP: the engine, the path-based entry points of api.cpp and the host tests use the same functions.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_io.hpp"

namespace axw {

// ------------------------------------------------------------------------------ byte-level BPE over ONE piece
// byte string -> rank (= id) of a token table (host_io.hpp: parse_token_table); of equal strings the lowest id
inline std::map<std::string, int> token_ranks(const std::vector<std::string>& table) {
  std::map<std::string, int> ranks;
  for (size_t i = 0; i < table.size(); ++i)
    if (!table[i].empty()) ranks.emplace(table[i], (int)i);
  return ranks;
}

// The ids of one piece of the GPT-2 split (the callers' strings are single pieces: an optional space followed by characters that are
// neither letters, digits nor white space; no regex here): single bytes, then the adjacent pair whose concatenation has the
// lowest rank is merged, the leftmost of equal ranks, until no pair has a rank. Throws if a byte has no rank.
inline std::vector<int> bpe_one_piece(const std::map<std::string, int>& ranks, const std::string& piece) {
  std::vector<std::string> parts;
  for (char c : piece) parts.emplace_back(1, c);
  for (;;) {
    int best = -1, best_rank = 0;
    for (size_t i = 0; i + 1 < parts.size(); ++i) {
      const auto it = ranks.find(parts[i] + parts[i + 1]);
      if (it != ranks.end() && (best < 0 || it->second < best_rank)) { best = (int)i; best_rank = it->second; }
    }
    if (best < 0) break;
    parts[best] += parts[best + 1];
    parts.erase(parts.begin() + best + 1);
  }
  std::vector<int> ids;
  for (const std::string& p : parts) {
    const auto it = ranks.find(p);
    if (it == ranks.end()) throw std::runtime_error("non_speech_tokens: the token table has no entry for a byte of '" + piece + "'");
    ids.push_back(it->second);
  }
  return ids;
}

// ------------------------------------------------------------------------------ the list that -1 stands for
// openai-whisper's Tokenizer.non_speech_tokens over a token table: the first id of " -" and of " '", and for every symbol of its
// list the first id of the symbol and of " " + symbol where that encoding is one id or the symbol is a musical sign. Sorted.
inline std::vector<int> non_speech_tokens(const std::vector<std::string>& table) {
  static const char* const kSymbols[] = {
      "\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
      "\xE3\x80\x8C", "\xE3\x80\x8D", "\xE3\x80\x8E", "\xE3\x80\x8F",  // 「 」 『 』
      "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]", "{{", "}}",
      "\xE2\x99\xAA\xE2\x99\xAA", "\xE2\x99\xAA\xE2\x99\xAA\xE2\x99\xAA"};  // ♪♪ ♪♪♪
  static const char* const kMusic[] = {"\xE2\x99\xA9", "\xE2\x99\xAA", "\xE2\x99\xAB", "\xE2\x99\xAC",
                                       "\xE2\x99\xAD", "\xE2\x99\xAE", "\xE2\x99\xAF"};  // ♩ ♪ ♫ ♬ ♭ ♮ ♯
  const std::map<std::string, int> ranks = token_ranks(table);
  std::vector<int> out = {bpe_one_piece(ranks, " -").at(0), bpe_one_piece(ranks, " '").at(0)};
  auto add = [&](const std::string& sym, bool always) {
    for (const std::string& s : {sym, " " + sym}) {
      const std::vector<int> ids = bpe_one_piece(ranks, s);
      if (ids.size() == 1 || always) out.push_back(ids.at(0));
    }
  };
  for (const char* s : kSymbols) add(s, false);
  for (const char* s : kMusic) add(s, true);
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return out;
}

// ------------------------------------------------------------------------------ which ids a set may hold
// Sorted, duplicates dropped. Ids of [0, eot) are the ones that matter; ids of (eot, ts_begin) are accepted and have no effect
// (rule 1 masks them anyway; transformers checkpoints list them). eot, timestamp ids, ids outside the vocabulary and more than
// n_vocab entries are refused.
inline std::vector<int> checked_suppress_tokens(const int* ids, int n, int n_vocab, int eot, int ts_begin, const char* what) {
  if (n < 0 || (n > 0 && !ids)) throw std::runtime_error(std::string(what) + ": bad arguments");
  if (n > n_vocab) throw std::runtime_error(std::string(what) + ": " + std::to_string(n) + " entries for a vocabulary of " + std::to_string(n_vocab));
  std::vector<int> v(ids, ids + n);
  for (int id : v) {
    if (id < 0 || id >= n_vocab) throw std::runtime_error(std::string(what) + ": id " + std::to_string(id) + " is outside the vocabulary [0, " + std::to_string(n_vocab) + ")");
    if (id == eot) throw std::runtime_error(std::string(what) + ": eot (" + std::to_string(id) + ") cannot be suppressed");
    if (id >= ts_begin) throw std::runtime_error(std::string(what) + ": timestamp id " + std::to_string(id) + " cannot be suppressed");
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// The optional key "suppress_tokens": [ids ...] of {type}_config.json; an entry -1 expands in place to non_speech_tokens of the
// table that `table` returns (called only when a -1 is met). Absent or []: none.
template <class TableFn>
inline std::vector<int> config_suppress_tokens(const JsonValue& j, int n_vocab, int eot, int ts_begin, TableFn&& table) {
  if (!j.has("suppress_tokens")) return {};
  const JsonValue& a = j.at("suppress_tokens");
  if (a.kind != JsonValue::Array) throw std::runtime_error("config: suppress_tokens must be a list of ids");
  std::vector<int> flat, derived;
  bool have_derived = false;
  for (const JsonValue& e : a.arr) {
    if (e.kind != JsonValue::Number || e.num != (double)(long)e.num || e.num < -1 || e.num > 2147483647.0)
      throw std::runtime_error("config: suppress_tokens must be a list of ids");
    if (e.num == -1) {
      if (!have_derived) { derived = non_speech_tokens(table()); have_derived = true; }
      flat.insert(flat.end(), derived.begin(), derived.end());
    } else {
      flat.push_back((int)e.num);
    }
  }
  // (a list with duplicates may be longer than the vocabulary and still name a valid set)
  std::sort(flat.begin(), flat.end());
  flat.erase(std::unique(flat.begin(), flat.end()), flat.end());
  return checked_suppress_tokens(flat.data(), (int)flat.size(), n_vocab, eot, ts_begin, "config: suppress_tokens");
}

// ------------------------------------------------------------------------------ the device form
// Words of the mask of a vocabulary: one bit per id, whole 16-byte groups
inline size_t suppress_mask_words(int n_vocab) { return ((size_t)n_vocab + 127) / 128 * 4; }
// bit i & 31 of word i >> 5 set iff id i < eot is in the set: no bit from eot up, so no kernel has a case for eot
inline std::vector<uint32_t> suppress_mask(const std::vector<int>& ids, int n_vocab, int eot) {
  std::vector<uint32_t> m(suppress_mask_words(n_vocab), 0u);
  for (int id : ids)
    if (id >= 0 && id < eot && id < n_vocab) m[(size_t)id >> 5] |= 1u << (id & 31);
  return m;
}

}  // namespace axw
