// engine_impl.hpp — what the translation units of axw::Engine share (engine.cpp: construction, weights, front-end, encoder, the
// entry points; engine_decode.cpp: the decode paths; engine_stream.cpp: utterance slots, the queue-placement probe;
// engine_long.cpp: long-form; engine_bench.cpp: the bench and scan hooks): the HIP owners, and through engine.hpp the class.
#pragma once
#include "common.hpp"
#include "owned.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>

namespace axw {
inline namespace AXW_NS {

#define HIP_CHECK(expr)                                                                                  \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess)                                                                                \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr);       \
  } while (0)

// ------------------------------------------------------------------------------ HIP objects and their owners
// The ONLY place the engine creates or destroys a HIP object: everything below hands out an owner (owned.hpp) that gives its
// handle back on every path out of its scope, a HIP_CHECK throw included.
template <auto Fn> struct Release { template <class H> hipError_t operator()(H h) const { return Fn(h); } };
template <class T> using DeviceArray = Owned<T*, Release<hipFree>>;  // a typed view of device memory: converts to T*
template <class T> using PinnedArray = Owned<T*, Release<hipHostFree>>;
using DeviceMem = DeviceArray<void>;
using PinnedMem = PinnedArray<void>;
using Stream = Owned<hipStream_t, Release<hipStreamDestroy>>;
using Event = Owned<hipEvent_t, Release<hipEventDestroy>>;
using Graph = Owned<hipGraph_t, Release<hipGraphDestroy>>;
using GraphExec = Owned<hipGraphExec_t, Release<hipGraphExecDestroy>>;

// at least 256 bytes; zero: filled, and the fill has finished when this returns
inline DeviceMem device_alloc(size_t bytes, bool zero = false) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 256)));
  DeviceMem mem(p);
  if (zero) {
    // the engine's streams are non-blocking (not ordered against the null stream): finish the fill before any
    // kernel on them can touch the buffer
    hipError_t e = hipMemset(p, 0, std::max<size_t>(bytes, 256));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) + " zero-filling a device buffer");
  }
  return mem;
}
template <class T> DeviceArray<T> device_array(size_t n, bool zero = false) {
  return DeviceArray<T>(static_cast<T*>(device_alloc(n * sizeof(T), zero).release()));
}

inline PinnedMem pinned_alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
  void* p = nullptr;
  HIP_CHECK(hipHostMalloc(&p, bytes, flags));
  return PinnedMem(p);
}
template <class T> PinnedArray<T> pinned_array(size_t n, unsigned flags = hipHostMallocDefault) {
  return PinnedArray<T>(static_cast<T*>(pinned_alloc(n * sizeof(T), flags).release()));
}

inline Stream make_stream() {  // non-blocking, like every stream of the engine
  hipStream_t s = nullptr;
  HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return Stream(s);
}
inline Event make_event(unsigned flags = hipEventDefault) {
  hipEvent_t e = nullptr;
  HIP_CHECK(hipEventCreateWithFlags(&e, flags));
  return Event(e);
}

// host: the bits of one stored h16 value -> float (bfloat16: the upper half of the fp32 pattern; half: IEEE binary16)
inline float h16_bits_to_float(uint16_t bits) {
#if AXW_F16
  _Float16 h;
  memcpy(&h, &bits, 2);
  return (float)h;
#else
  const uint32_t u = (uint32_t)bits << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
#endif
}

// `slot` holds `value` until the guard leaves scope, then what it held before (a bench hook's route for its call: Engine::prefill_force_)
template <class T> class ScopedSet {
 public:
  ScopedSet(T& slot, T value) : slot_(slot), old_(slot) { slot = value; }
  ~ScopedSet() { slot_ = old_; }
  ScopedSet(const ScopedSet&) = delete;
 private:
  T& slot_;
  T old_;
};

// Launch-per-row-block form of the batched vocabulary projection (used where the register-resident form does not fit:
// d_model 1280 beyond 48 clips): weight-row tiles of 16 rows per workgroup, two per wave (1 / 2 / 4 measured alike).
static int logits_rt() { return 2; }

}  // inline namespace AXW_NS
}  // namespace axw

#include "engine.hpp"  // (its members are the owners above)
