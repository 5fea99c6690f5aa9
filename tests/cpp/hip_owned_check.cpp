// hip_owned_check.cpp -- csrc/nid_hip_owned.h (DevBuf, PinnedBuf, Event, Stream, ring_size / ring_grow) against counting
// fakes of the HIP entry points it calls: nothing of the HIP runtime is linked.  Every fake object is a malloc'ed block,
// so AddressSanitizer reports a double release or a use after one; the fakes count what is live per kind, count the
// calls, fail the k-th creation on request and keep the runtime's "last error" the way the runtime does (set by a failed
// call, read and cleared by hipGetLastError).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "nid_hip_owned.h"

namespace {
int g_live_dev = 0, g_live_pinned = 0, g_live_event = 0, g_live_stream = 0;
int g_calls = 0;         // every fake entry point
int g_creations = 0;     // hipMalloc, hipHostMalloc, hipHostGetDevicePointer, hipEventCreateWithFlags, hipStreamCreateWithFlags
int g_fail_at = 0;       // the creation with this number (1-based) fails; 0: none
int g_synced_streams = 0;
hipError_t g_pending = hipSuccess;
int g_failures = 0;

int live() { return g_live_dev + g_live_pinned + g_live_event + g_live_stream; }
bool creation_fails() { return ++g_creations == g_fail_at; }
hipError_t failed(hipError_t e) { g_pending = e; return e; }

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); g_failures++; } \
  } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
  g_calls++;
  if (creation_fails()) { *p = nullptr; return failed(hipErrorOutOfMemory); }
  *p = std::malloc(bytes ? bytes : 1);
  g_live_dev++;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  g_calls++;
  if (p) { std::free(p); g_live_dev--; }
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) {
  g_calls++;
  if (creation_fails()) { *p = nullptr; return failed(hipErrorOutOfMemory); }
  *p = std::malloc(bytes ? bytes : 1);
  g_live_pinned++;
  return hipSuccess;
}
hipError_t hipHostFree(void *p) {
  g_calls++;
  if (p) { std::free(p); g_live_pinned--; }
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) {
  g_calls++;
  if (creation_fails()) { *d = nullptr; return failed(hipErrorInvalidValue); }
  *d = h;
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
  g_calls++;
  if (creation_fails()) { *e = nullptr; return failed(hipErrorOutOfMemory); }
  *e = static_cast<hipEvent_t>(std::malloc(8));
  g_live_event++;
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  g_calls++;
  std::free(e);
  g_live_event--;
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  g_calls++;
  if (creation_fails()) { *s = nullptr; return failed(hipErrorOutOfMemory); }
  *s = static_cast<hipStream_t>(std::malloc(8));
  g_live_stream++;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  g_calls++;
  *reinterpret_cast<volatile char *>(s) = 1;  // (a destroyed stream: AddressSanitizer says so)
  g_synced_streams++;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  g_calls++;
  std::free(s);
  g_live_stream--;
  return hipSuccess;
}
hipError_t hipGetLastError(void) {
  g_calls++;
  return std::exchange(g_pending, hipSuccess);
}
}  // extern "C"

namespace {
using namespace nid;

// everything a context holds, in miniature: the order of its creations is the order the k-th failure walks through
struct Holder {
  Stream stream;
  DevBuf<double> dev;
  PinnedBuf<int> plain, mapped;
  Event event;
  DevBuf<char> ring[3];
  bool make() {
    return stream.create() == hipSuccess && dev.alloc(100) == hipSuccess && plain.alloc(7) == hipSuccess &&
           mapped.alloc(9, hipHostMallocMapped) == hipSuccess && event.create(hipEventDisableTiming) == hipSuccess &&
           ring_grow(ring, 5) == hipSuccess;
  }
};
constexpr int kHolderCreations = 1 + 1 + 1 + 2 + 1 + 3;  // (the mapped buffer: the allocation and the device-pointer query)

void scopes_and_moves() {
  {
    DevBuf<double> a;
    CHECK(a.get() == nullptr && a.size() == 0);
    CHECK(a.alloc(10) == hipSuccess && a.size() == 10 && a.get() != nullptr && g_live_dev == 1);
    a.get()[9] = 1.0;
    DevBuf<double> b(std::move(a));
    CHECK(a.get() == nullptr && a.size() == 0 && b.size() == 10 && g_live_dev == 1);
    DevBuf<double> c;
    CHECK(c.alloc(3) == hipSuccess && g_live_dev == 2);
    c = std::move(b);  // (c's own three go)
    CHECK(g_live_dev == 1 && c.size() == 10 && b.get() == nullptr && b.size() == 0);
    c = DevBuf<double>();
    CHECK(g_live_dev == 0 && c.size() == 0);
  }
  CHECK(live() == 0);
  {
    PinnedBuf<int> p, q;
    CHECK(p.alloc(4) == hipSuccess && p.host() != nullptr && p.dev() == nullptr && p.size() == 4);
    CHECK(q.alloc(4, hipHostMallocMapped) == hipSuccess && q.dev() == q.host() && q.host() != nullptr);
    PinnedBuf<int> r(std::move(q));
    CHECK(q.host() == nullptr && q.dev() == nullptr && q.size() == 0 && r.dev() != nullptr && g_live_pinned == 2);
    p = std::move(r);
    CHECK(g_live_pinned == 1 && p.dev() != nullptr && p.size() == 4);
  }
  CHECK(live() == 0);
  {
    Event e, f;
    CHECK(e.get() == nullptr && e.ensure(hipEventDisableTiming) == hipSuccess && g_live_event == 1);
    const hipEvent_t first = e.get();
    const int calls = g_calls;
    CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && e.get() == first && g_calls == calls);  // (first use only)
    CHECK(f.create() == hipSuccess && g_live_event == 2);
    f = std::move(e);
    CHECK(g_live_event == 1 && f.get() == first && e.get() == nullptr);
    Event g(std::move(f));
    CHECK(g_live_event == 1 && g.get() == first);
  }
  CHECK(live() == 0);
  {
    g_synced_streams = 0;
    Stream s, t;
    CHECK(s.create() == hipSuccess && t.ensure() == hipSuccess && g_live_stream == 2);
    t = std::move(s);  // (t's own stream: synchronised, then destroyed)
    CHECK(g_live_stream == 1 && g_synced_streams == 1 && s.get() == nullptr);
  }
  CHECK(live() == 0 && g_synced_streams == 2);
  {
    std::vector<DevBuf<float>> v(5);
    for (size_t i = 0; i < v.size(); i++) CHECK(v[i].alloc(i + 1) == hipSuccess);
    v.resize(40);  // (moved into new storage)
    CHECK(g_live_dev == 5 && v[4].size() == 5);
    v.erase(v.begin());
    CHECK(g_live_dev == 4 && v[0].size() == 2);
    std::vector<Holder> h(3);
    for (Holder &x : h) CHECK(x.make());
    h.resize(17);
    CHECK(g_live_stream == 3 && g_live_event == 3 && g_live_pinned == 6 && g_live_dev == 4 + 3 * 4);
    Event events[4];
    for (Event &e : events) CHECK(e.create() == hipSuccess);
  }
  CHECK(live() == 0 && g_pending == hipSuccess);
}

void alloc_and_grow() {
  DevBuf<double> a;
  CHECK(a.grow(8) == hipSuccess && a.size() == 8);
  int calls = g_calls;
  CHECK(a.grow(8) == hipSuccess && a.grow(3) == hipSuccess && a.grow(0) == hipSuccess && g_calls == calls && a.size() == 8);
  // alloc frees before it allocates: never two blocks live, and exactly n afterwards (also a smaller n)
  calls = g_calls;
  CHECK(a.alloc(3) == hipSuccess && a.size() == 3 && g_live_dev == 1 && g_calls == calls + 2);
  g_fail_at = g_creations + 1;  // (the old block is gone by the time the new one is refused)
  CHECK(a.alloc(1000) == hipErrorOutOfMemory && a.size() == 0 && a.get() == nullptr && g_live_dev == 0);
  CHECK(hipGetLastError() == hipSuccess);
  CHECK(a.grow(2) == hipSuccess && a.size() == 2);
  a.reset();
  CHECK(g_live_dev == 0 && a.size() == 0 && a.get() == nullptr);
  a.reset();

  PinnedBuf<double> p;
  CHECK(p.grow(8, hipHostMallocMapped) == hipSuccess && p.size() == 8 && p.dev() != nullptr);
  calls = g_calls;
  CHECK(p.grow(8, hipHostMallocMapped) == hipSuccess && p.grow(1) == hipSuccess && g_calls == calls);
  CHECK(p.alloc(2) == hipSuccess && p.size() == 2 && p.dev() == nullptr && g_live_pinned == 1);
  // the device-pointer query fails: the allocation is given back
  g_fail_at = g_creations + 2;
  CHECK(p.alloc(5, hipHostMallocMapped) == hipErrorInvalidValue && p.size() == 0 && p.host() == nullptr && p.dev() == nullptr && g_live_pinned == 0);
  CHECK(hipGetLastError() == hipSuccess);
  g_fail_at = 0;
  CHECK(live() == 0);
}

void every_creation_fails_in_turn() {
  for (int k = 1; k <= kHolderCreations; k++) {
    {
      Holder h;
      g_fail_at = g_creations + k;
      CHECK(!h.make());
      g_fail_at = 0;
      CHECK(hipGetLastError() == hipSuccess);  // nothing pending for the next launch's check
      // the one that failed is empty; what was made before it is whole, what comes behind it untouched
      CHECK((h.stream.get() != nullptr) == (k > 1));
      CHECK(h.dev.size() == (k > 2 ? 100u : 0u) && (h.dev.get() != nullptr) == (k > 2));
      CHECK(h.plain.size() == (k > 3 ? 7u : 0u) && (h.plain.host() != nullptr) == (k > 3));
      CHECK(h.mapped.size() == (k > 5 ? 9u : 0u) && (h.mapped.host() != nullptr) == (k > 5) && (h.mapped.dev() != nullptr) == (k > 5));
      CHECK((h.event.get() != nullptr) == (k > 6));
      for (int i = 0; i < 3; i++) CHECK(h.ring[i].size() == (k > 7 + i ? 5u : 0u) && (h.ring[i].get() != nullptr) == (k > 7 + i));
      CHECK(ring_size(h.ring) == 0);
      CHECK(g_live_stream == (k > 1) && g_live_event == (k > 6) && g_live_pinned == (k > 3) + (k > 5) && g_live_dev == (k > 2) + std::max(0, k - 7));
      CHECK(h.make() && ring_size(h.ring) == 5);  // the next call succeeds
    }
    CHECK(live() == 0);
  }
  {
    Event e;
    Stream s;
    g_fail_at = g_creations + 1;
    CHECK(e.ensure() != hipSuccess && e.get() == nullptr && hipGetLastError() == hipSuccess);
    g_fail_at = g_creations + 1;
    CHECK(s.ensure() != hipSuccess && s.get() == nullptr && hipGetLastError() == hipSuccess);
    g_fail_at = 0;
    CHECK(e.ensure() == hipSuccess && s.ensure() == hipSuccess);
  }
  CHECK(live() == 0);
}

// a ring of 4 grown to 8, then to 32 with the third allocation refused, then asked for 8 again: the entry that the
// failure left empty must be made, not taken for one that suffices
template <typename B>
void ring_after_a_failed_growth() {
  {
    B ring[4];
    CHECK(ring_size(ring) == 0 && ring_grow(ring, 8) == hipSuccess && ring_size(ring) == 8);
    int calls = g_calls;
    CHECK(ring_grow(ring, 8) == hipSuccess && ring_grow(ring, 5) == hipSuccess && g_calls == calls);
    g_fail_at = g_creations + 3;
    CHECK(ring_grow(ring, 32) == hipErrorOutOfMemory);
    g_fail_at = 0;
    CHECK(hipGetLastError() == hipSuccess);
    CHECK(ring[0].size() == 32 && ring[1].size() == 32 && ring[2].size() == 0 && ring[3].size() == 8);
    CHECK(ring_size(ring) == 0);  // "capacity suffices" is not on offer while an entry is empty
    calls = g_calls;
    CHECK(ring_grow(ring, 8) == hipSuccess && g_calls == calls + 1);  // (exactly the missing entry)
    CHECK(ring_size(ring) == 8);
    for (const B &b : ring) CHECK(static_cast<const void *>(b) != nullptr && b.size() >= 8);
    // ... and when that allocation is refused too, the request fails
    ring[1].reset();
    g_fail_at = g_creations + 1;
    CHECK(ring_grow(ring, 8) == hipErrorOutOfMemory && ring_size(ring) == 0 && hipGetLastError() == hipSuccess);
    g_fail_at = 0;
  }
  CHECK(live() == 0);
}
}  // namespace

int main() {
  scopes_and_moves();
  alloc_and_grow();
  every_creation_fails_in_turn();
  ring_after_a_failed_growth<DevBuf<double>>();
  ring_after_a_failed_growth<PinnedBuf<double>>();
  CHECK(live() == 0 && g_pending == hipSuccess);
  std::printf("hip owned: %d fake HIP calls, %d creations, %d failures\n", g_calls, g_creations, g_failures);
  return g_failures ? 1 : 0;
}
