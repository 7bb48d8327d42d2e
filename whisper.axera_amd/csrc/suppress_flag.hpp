// suppress_flag.hpp — the value of --suppress_tokens as whisper_cli and whisper_srv take it, through the C ABI alone:
// "-1": the non-speech ids derived from the model's tokens file (AX_WHISPER_NonSpeechTokens, host only); "1,2,3": those ids.
#pragma once
#include <cstdlib>
#include <string>
#include <vector>

#include "ax_whisper_api.h"

// -> ids (at least one), or false with the reason in err
inline bool suppress_flag_ids(const std::string& arg, const std::string& model_path, const std::string& model_type, std::vector<int>& ids,
                              std::string& err) {
  ids.clear();
  if (arg == "-1") {
    ids.resize(4096);
    int n = 0;
    if (AX_WHISPER_NonSpeechTokens((model_path + "/" + model_type + "/" + model_type + "-tokens.txt").c_str(), (int)ids.size(), ids.data(), &n) != 0) {
      err = std::string("--suppress_tokens -1 failed! ") + AX_WHISPER_LastError(nullptr);
      return false;
    }
    ids.resize(n);
  }
  for (size_t p = 0; arg != "-1" && p < arg.size();) {
    char* end = nullptr;
    const long v = strtol(arg.c_str() + p, &end, 10);
    if (end == arg.c_str() + p || v < 0 || v > 2147483647L || (*end && *end != ',')) {
      err = "bad value: --suppress_tokens " + arg + " (-1, or ids 1,2,3)";
      return false;
    }
    ids.push_back((int)v);
    p = (size_t)(end - arg.c_str()) + (*end ? 1 : 0);
  }
  if (ids.empty()) { err = "bad value: --suppress_tokens " + arg + " (no ids)"; return false; }
  return true;
}
