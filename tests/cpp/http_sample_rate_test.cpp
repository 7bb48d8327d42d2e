// Host only: the X-Sample-Rate parse of csrc/http_request.hpp (whisper_srv) on request heads as bytes, for tests/test_resample_abi.py.
// Prints one line per case: "<name> rate=<Hz> rate_ok=<0|1> error=<text or ->"; exit status 0.
#include <cstdio>
#include <string>

#include "http_request.hpp"

static void run(const char* name, const std::string& rate_header) {
  const std::string head = "POST /asr HTTP/1.1\r\nHost: x\r\nContent-Type: application/octet-stream\r\n" + rate_header + "Content-Length: 8\r\n\r\n";
  axw::HttpHead h;
  if (!axw::parse_http_head(head + "12345678", h)) { printf("%s incomplete\n", name); return; }
  const char* err = axw::asr_request_error(h, 8);
  printf("%s rate=%d rate_ok=%d error=%s\n", name, h.sample_rate, h.rate_ok ? 1 : 0, err ? err : "-");
}

int main() {
  run("absent", "");
  run("8000", "X-Sample-Rate: 8000\r\n");
  run("spaces", "x-sample-rate:   48000  \r\n");
  run("non-numeric", "X-Sample-Rate: 44.1k\r\n");
  run("zero", "X-Sample-Rate: 0\r\n");
  run("negative", "X-Sample-Rate: -8000\r\n");
  run("empty", "X-Sample-Rate:\r\n");
  run("long", "X-Sample-Rate: 12345678\r\n");
  run("other-header", "X-Not-Sample-Rate: 8000\r\nXX-Sample-Rate: 8000\r\n");
  return 0;
}
