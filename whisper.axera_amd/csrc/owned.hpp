// owned.hpp — one move-only owner for every handle the engine has to give back (device and pinned memory, streams, events,
// graphs). Header-only and free of HIP on purpose: tests/cpp/owned_test.cpp checks it under plain g++ with a counting Release;
// engine_impl.hpp names the HIP aliases and is the only place their handles are made.
#pragma once

#include <atomic>

namespace axw {

// handles held by owners right now, over the bfloat16 and the half build of the engine alike (AX_WHISPER_GetConfigInt
// "live_hip_objects": a handle that was closed, or whose Init failed, leaves this where it was)
inline std::atomic<long> live_owned{0};

// Release: default-constructible, callable with a Handle; what it returns is ignored (a failed release has no remedy)
template <class Handle, class Release>
class Owned {
 public:
  Owned() = default;
  explicit Owned(Handle h) : h_(h) { count(+1); }
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = Handle{}; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = Handle{};
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }

  Handle get() const { return h_; }
  operator Handle() const { return h_; }
  void reset(Handle h = Handle{}) {
    if (h_ != Handle{}) {
      (void)Release{}(h_);
      count(-1);
    }
    h_ = h;
    count(+1);
  }
  Handle release() {  // gives the handle up without releasing it
    count(-1);
    Handle h = h_;
    h_ = Handle{};
    return h;
  }

 private:
  void count(long by) const { if (h_ != Handle{}) live_owned.fetch_add(by, std::memory_order_relaxed); }
  Handle h_{};
};

}  // namespace axw
