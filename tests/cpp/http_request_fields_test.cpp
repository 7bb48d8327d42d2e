// Host only, stand-alone (its own main; built with -fsanitize=address,undefined by tests/test_stream_ts_host.py): the X-Timestamps,
// X-Language and X-Task parse of csrc/http_request.hpp (whisper_srv --timestamps) on request heads as bytes.
// Prints one line per case: "<name> ts=<-1|0|1> lang=<code or -> task=<-1|0|1> plain=<error or -> slots=<error or ->" (plain: a
// server without --timestamps, slots: one with it); a head without the three headers must parse as it did before they existed.
#include <cstdio>
#include <string>

#include "http_request.hpp"

static int failures = 0;

static void run(const char* name, const std::string& headers) {
  const std::string head = "POST /asr HTTP/1.1\r\nHost: x\r\nContent-Type: application/octet-stream\r\n" + headers + "Content-Length: 8\r\n\r\n";
  axw::HttpHead h;
  if (!axw::parse_http_head(head + "12345678", h)) { printf("%s incomplete\n", name); return; }
  const char* a = axw::asr_slot_fields_error(h, false);
  const char* b = axw::asr_slot_fields_error(h, true);
  printf("%s ts=%d lang=%s task=%d plain=%s slots=%s\n", name, h.timestamps, h.language.empty() ? "-" : h.language.c_str(), h.task, a ? a : "-", b ? b : "-");
  // what the head held before these fields existed is parsed as before, whatever they say
  if (h.first != "POST /asr HTTP/1.1" || h.content_type != "application/octet-stream" || h.content_length != 8 || !h.length_ok ||
      h.expect_continue || h.sample_rate != 16000 || !h.rate_ok || h.header_end != head.size() - 4 || axw::asr_request_error(h, 8) ||
      axw::http_route(h) != axw::HttpRoute::Asr) {
    printf("%s: the rest of the head changed\n", name);
    ++failures;
  }
}

int main() {
  run("absent", "");
  run("all", "X-Timestamps: 1\r\nX-Language: en\r\nX-Task: translate\r\n");
  run("case-and-blanks", "x-TIMESTAMPS:   0  \r\nX-LANGUAGE:\t Auto \r\nx-task:   TRANSCRIBE\t\r\n");
  run("other-headers", "X-Foo-Language: en\r\nXX-Timestamps: 1\r\nNot-X-Task: translate\r\n");
  run("language-only", "X-Language: yue\r\n");
  run("ts-2", "X-Timestamps: 2\r\n");
  run("ts-empty", "X-Timestamps:\r\n");
  run("ts-word", "X-Timestamps: yes\r\n");
  run("ts-signed", "X-Timestamps: +1\r\n");
  run("lang-empty", "X-Language:  \r\n");
  run("lang-digits", "X-Language: e1\r\n");
  run("lang-long", "X-Language: abcdefghijklm\r\n");
  run("lang-two", "X-Language: en, de\r\n");
  run("task-empty", "X-Task:\r\n");
  run("task-other", "X-Task: summarise\r\n");
  run("task-prefix", "X-Task: translated\r\n");
  {  // a head that ends inside a field's line, and one field repeated: the first line counts, nothing is read past the head
    axw::HttpHead h;
    const std::string cut = "POST /asr HTTP/1.1\r\nX-Language: en";
    if (axw::parse_http_head(cut, h)) { printf("cut head parsed\n"); ++failures; }
    const std::string twice = "POST /asr HTTP/1.1\r\nX-Task: translate\r\nX-Task: transcribe\r\nX-Language: de\r\n\r\n";
    if (!axw::parse_http_head(twice, h) || h.task != 1 || h.language != "de") { printf("repeated header\n"); ++failures; }
    const std::string last = "POST /asr HTTP/1.1\r\nX-Timestamps: 1\r\n\r\n";  // the value ends where the head ends
    if (!axw::parse_http_head(last, h) || h.timestamps != 1) { printf("last header\n"); ++failures; }
  }
  return failures ? 1 : 0;
}
