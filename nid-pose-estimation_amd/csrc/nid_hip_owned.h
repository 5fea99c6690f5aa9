// nid_hip_owned.h -- one owner per device resource of the host layer (nid_capi.hip and its .inc files): device memory,
// pinned host memory, events and streams as move-only members that release themselves, each buffer knowing its own size.
// Only the HIP runtime's API header and the standard library: a host compiler builds it alone
// (tests/cpp/hip_owned_check.cpp, with counting fakes for the dozen hip* entry points used here).
//
// THE FAILURE RULE of every alloc / grow / create / ensure: the owner is empty afterwards (size() == 0, null handle),
// the error is returned, and no HIP error is left pending for the next hipGetLastError() behind a kernel launch.
// None of the types selects a device or retires a resident kernel: the caller does both, in front of what frees.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

namespace nid {

inline hipError_t owned_result(hipError_t e) {
  if (e != hipSuccess) (void)hipGetLastError();  // (the one place a failed creation's pending error is taken away)
  return e;
}

// device memory: n elements of T
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~DevBuf() { reset(); }
  // what it holds is freed first; then exactly n
  hipError_t alloc(size_t n) {
    reset();
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) { p_ = static_cast<T *>(p); n_ = n; }
    return owned_result(e);
  }
  hipError_t grow(size_t n) { return n_ >= n ? hipSuccess : alloc(n); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; n_ = 0;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t size() const { return n_; }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};

// pinned host memory: n elements of T; with hipHostMallocMapped also the address the device writes it at
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  PinnedBuf &operator=(PinnedBuf &&o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); d_ = std::exchange(o.d_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~PinnedBuf() { reset(); }
  hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
    reset();
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, n * sizeof(T), flags);
    if (e == hipSuccess && (flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) (void)hipHostFree(h);
    if (e == hipSuccess) { h_ = static_cast<T *>(h); d_ = static_cast<T *>(d); n_ = n; }
    return owned_result(e);
  }
  hipError_t grow(size_t n, unsigned flags = hipHostMallocDefault) { return n_ >= n ? hipSuccess : alloc(n, flags); }
  void reset() {
    if (h_) (void)hipHostFree(h_);
    h_ = d_ = nullptr; n_ = 0;
  }
  T *host() const { return h_; }
  T *dev() const { return d_; }  // (null unless mapped)
  operator T *() const { return h_; }
  size_t size() const { return n_; }

 private:
  T *h_ = nullptr, *d_ = nullptr;
  size_t n_ = 0;
};

// A ring of buffers whose entries all hold at least n: the capacity is the smallest entry's own size, so an entry that a
// failed growth left empty is never taken for one that suffices.
template <typename B, size_t N>
size_t ring_size(const B (&ring)[N]) {
  size_t n = ring[0].size();
  for (const B &b : ring) n = std::min(n, b.size());
  return n;
}
template <typename B, size_t N, typename... Flags>
hipError_t ring_grow(B (&ring)[N], size_t n, Flags... flags) {
  for (B &b : ring) {
    const hipError_t e = b.grow(n, flags...);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// an event or a stream: one handle, one way to give it back
template <typename H, void (*Release)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle &operator=(Handle &&o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h_) Release(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};
inline void release_event(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void release_stream(hipStream_t s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }

// create: what it holds goes first; ensure: created on first use
struct Event : Handle<hipEvent_t, release_event> {
  hipError_t create(unsigned flags = hipEventDefault) { reset(); return owned_result(hipEventCreateWithFlags(&h_, flags)); }
  hipError_t ensure(unsigned flags = hipEventDefault) { return h_ ? hipSuccess : create(flags); }
};
// a non-blocking stream; given back behind a synchronisation
struct Stream : Handle<hipStream_t, release_stream> {
  hipError_t create() { reset(); return owned_result(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking)); }
  hipError_t ensure() { return h_ ? hipSuccess : create(); }
};

}  // namespace nid
