// nid_buffer_watch.h -- the legacy operators' content watch over the caller's buffers: what a buffer held when it was
// uploaded (Key), the hashes behind it, the pool of worker threads that takes them (HashPool) and the rotating
// verification of one call (Verifier).  No HIP, no C-ABI, no I/O: the standard library and pthreads.  Included by
// host/legacy_ops.cpp and by tests/cpp/buffer_watch_check.cpp (stand-alone, under the sanitizers) and by NOTHING else:
// HashPool is a process singleton with fork handlers.  Which mode verifies what, how many slices a call takes and what
// is said on stderr is the operators' business: no mode and no environment variable but the pool's own two is read here.
#pragma once

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <pthread.h>
#include <thread>
#include <unistd.h>
#include <vector>

namespace nid_watch {

constexpr int kSlices = 128;  // a big buffer's content key: one hash per slice (legacy_ops.cpp asserts that this is its header's count)

// 64 samples spread over the array + its length, FNV-1a over their bytes (never 0)
template <typename T>
uint64_t fingerprint(const T *a, size_t n) {
  if (!a) return 1;
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t bytes) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 1099511628211ull; }
  };
  mix(&n, sizeof(n));
  const size_t samples = n < 64 ? n : 64;
  for (size_t k = 0; k < samples; k++) {
    const size_t i = samples > 1 ? (size_t)((unsigned __int128)k * (n - 1) / (samples - 1)) : 0;
    mix(&a[i], sizeof(T));
  }
  return h ? h : 2;
}

// ---- content hashes -------------------------------------------------------------------------------------------
// A frame pair's big buffers (points3d 7.4 MB, bs_value 9.8 MB at 640x480) are hashed once per pair in full and a few
// slices per call after that; one core does ~20 GB/s.  The slices go to a small pool of worker threads (created at the
// first use, parked on a condition variable in between) beside the caller.  The pool's size: NID_LEGACY_HASH_THREADS
// workers (default 3; 0: the caller hashes alone, no thread is created).  A job lives INSIDE one operator call: start()
// takes the pool, finish() -- always before the operator returns -- gives it back; no worker touches a caller buffer
// outside start() .. finish().
class HashPool {
 public:
  static HashPool &get() { static HashPool *p = new HashPool;  return *p; }  // (never destroyed: its parked workers end with the process)
  // start(n, job): job(0..n-1) is handed to the workers -- each takes the next part that nobody has taken -- and the
  // call returns; finish(): the caller takes what is left and waits for the rest.  One job at a time, started and
  // finished by the same thread; the job must stay valid until finish().
  // Parts are claimed with one atomic increment on the JOB's own counter (a worker that comes late holds the old job
  // object and finds nothing left in it: it can never touch the next job's parts); the mutex is for parking only.
  void start(int nparts, std::function<void(int)> fn) {
    call_.lock();
    auto j = std::make_shared<Job>();
    j->fn = std::move(fn);
    j->nparts = nparts;
    j->remaining.store(nparts, std::memory_order_relaxed);
    mine_ = j;
    std::atomic_store(&current_, j);
    generation_.fetch_add(1);  // (sequentially consistent with parked_: either this thread sees a parking worker, or the worker sees the new generation)
    if (parked_.load() > 0 && has_workers()) {  // (a fork()ed child has no workers: finish() does all parts)
      std::lock_guard<std::mutex> g(m_);
      wake_.notify_all();
    }
  }
  void finish() {
    Job &j = *mine_;
    help(j);
    while (j.remaining.load(std::memory_order_acquire) > 0) __builtin_ia32_pause();  // (parts in other threads' hands: microseconds)
    std::atomic_store(&current_, std::shared_ptr<Job>());
    mine_.reset();
    call_.unlock();
  }
  void run(int nparts, std::function<void(int)> job) { start(nparts, std::move(job)); finish(); }
  bool has_workers() const { return !workers_.empty() && getpid() == owner_; }

 private:
  struct Job {
    std::function<void(int)> fn;
    int nparts = 0;
    std::atomic<int> next{0}, remaining{0};
  };
  HashPool() : owner_(getpid()) {
    int n = 3;
    if (const char *e = getenv("NID_LEGACY_HASH_THREADS")) n = std::max(0, std::min(15, atoi(e)));
    if (const char *e = getenv("NID_LEGACY_HASH_SPIN_US")) spin_us_ = std::max(0, std::min(100000, atoi(e)));
    for (int w = 0; w < n; w++) workers_.emplace_back([this] { loop(); });
    // fork(): threads do not survive it, locks do -- a child forked while a worker held m_ would wait for it for ever.
    // The prepare handler takes call_ (free whenever no operator is inside start() .. finish(): a job never outlives
    // the call that started it, so a fork() between two calls finds it free; a fork() from another thread waits for
    // the running call's finish()) and then m_, so the child inherits both free, with no job in flight (and finds
    // itself without workers by its pid).
    pthread_atfork([] { HashPool &p = get(); p.call_.lock(); p.m_.lock(); },
                   [] { HashPool &p = get(); p.m_.unlock(); p.call_.unlock(); },
                   [] { HashPool &p = get(); p.m_.unlock(); p.call_.unlock(); });
  }
  static void help(Job &j) {  // take parts until none is left
    for (;;) {
      const int part = j.next.fetch_add(1, std::memory_order_acq_rel);
      if (part >= j.nparts) return;
      j.fn(part);
      j.remaining.fetch_sub(1, std::memory_order_release);
    }
  }
  // A worker that has just served a job keeps POLLING for the next one for spin_us_ microseconds before it parks on the
  // condition variable: the operators are called back to back by the LM (one call per 30-60 us), and a parked thread
  // takes 10-20 us to come back -- as long as the whole evaluation it is supposed to hide behind
  // (profiles/r06_legacy_call_cost.txt).  NID_LEGACY_HASH_SPIN_US (default 150; 0: park at once).
  void loop() {
    unsigned long seen = 0;
    for (;;) {
      const auto t0 = std::chrono::steady_clock::now();
      bool got = false;
      for (unsigned spins = 0; spin_us_ > 0; spins++) {
        if (generation_.load(std::memory_order_acquire) != seen) { got = true; break; }
        __builtin_ia32_pause();
        if ((spins & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us_)) break;
      }
      if (!got) {
        std::unique_lock<std::mutex> g(m_);
        parked_.fetch_add(1);
        wake_.wait(g, [&] { return generation_.load() != seen; });
        parked_.fetch_sub(1);
      }
      seen = generation_.load(std::memory_order_acquire);
      if (std::shared_ptr<Job> j = std::atomic_load(&current_)) help(*j);
    }
  }
  std::mutex call_, m_;
  std::condition_variable wake_;
  std::shared_ptr<Job> current_, mine_;
  std::vector<std::thread> workers_;
  std::atomic<unsigned long> generation_{0};
  std::atomic<int> parked_{0};
  int spin_us_ = 150;
  const pid_t owner_;
};

// one contiguous run of bytes, 64 bits: eight interleaved multiply-xor lanes over the 8-byte words (eight independent
// dependency chains keep the multiplier busy: memory-bound, ~0.05 ms/MB on one core)
inline uint64_t hash_run(const unsigned char *b, size_t bytes, uint64_t salt) {
  const size_t words = bytes / 8;
  constexpr int L = 8;
  uint64_t h[L] = {0x9E3779B97F4A7C15ull ^ salt, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull,
                   0x85EBCA77C2B2AE63ull, 0xD6E8FEB86659FD93ull, 0xA0761D6478BD642Full, 0xE7037ED1A0B428DBull};
  size_t i = 0;
  for (; i + L <= words; i += L) {
    uint64_t w[L];
    std::memcpy(w, b + 8 * i, 8 * L);
    for (int k = 0; k < L; k++) { h[k] = (h[k] ^ w[k]) * 0x9FB21C651E98DF25ull; h[k] ^= h[k] >> 29; }
  }
  for (; i < words; i++) { uint64_t w; std::memcpy(&w, b + 8 * i, 8); h[i % L] = (h[i % L] ^ w) * 0x9FB21C651E98DF25ull; h[i % L] ^= h[i % L] >> 29; }
  for (size_t t = 8 * words; t < bytes; t++) h[0] = (h[0] ^ b[t]) * 0x100000001B3ull;
  uint64_t r = h[0];
  for (int k = 1; k < L; k++) r = (r ^ h[k]) * 0xFF51AFD7ED558CCDull + k;
  r ^= r >> 32;
  return r;
}

// slice s of a buffer of `bytes` bytes: [lo, hi), split at multiples of 64 bytes (whole bs_value rows); the last slice
// takes the remainder (a buffer below 8 KB -- 128 slices of 64 bytes -- is its last slice alone)
inline void slice_range(size_t bytes, int s, size_t *lo, size_t *hi) {
  const size_t part = (bytes / kSlices) & ~(size_t)63;
  *lo = part * (size_t)s;
  *hi = s == kSlices - 1 ? bytes : part * (size_t)(s + 1);
}
inline uint64_t combine_slices(const uint64_t *h) {
  uint64_t r = h[0];
  for (int p = 1; p < kSlices; p++) r = (r ^ h[p]) * 0xFF51AFD7ED558CCDull + p;
  r ^= r >> 32;
  return r ? r : 2;
}
// the small per-cell arrays: one run, on the caller
template <typename T>
uint64_t small_hash(const T *a, size_t n) {
  if (!a) return 1;
  const uint64_t r = hash_run(reinterpret_cast<const unsigned char *>(a), n * sizeof(T), n * sizeof(T));
  return r ? r : 2;
}

// Slices [first, first + count) (mod kSlices) of up to four buffers as ONE pooled job: begin() hands the parts to the
// workers and returns, end() takes what is left, waits, and leaves every requested slice's hash in out[buffer][slice].
// Both are called inside one operator call.
class SliceHasher {
 public:
  struct Req { const void *data = nullptr; size_t bytes = 0; };
  void begin(const Req *reqs, int n, int first, int count) {
    parts_.clear();
    for (int r = 0; r < n && r < 4; r++) {
      const unsigned char *b = static_cast<const unsigned char *>(reqs[r].data);
      if (!b) continue;
      for (int c = 0; c < count && c < kSlices; c++) {
        const int s = (first + c) % kSlices;
        size_t lo, hi;
        slice_range(reqs[r].bytes, s, &lo, &hi);
        parts_.push_back({b + lo, hi - lo, (uint64_t)reqs[r].bytes + (uint64_t)s, &out[r][s]});
      }
    }
    running_ = true;
    HashPool::get().start((int)parts_.size(), [this](int k) {
      const Part &pt = parts_[(size_t)k];
      *pt.out = hash_run(pt.b, pt.bytes, pt.salt);
    });
  }
  bool running() const { return running_; }
  void end() {
    if (!running_) return;
    HashPool::get().finish();
    running_ = false;
  }
  uint64_t out[4][kSlices] = {};

 private:
  struct Part { const unsigned char *b; size_t bytes; uint64_t salt; uint64_t *out; };
  std::vector<Part> parts_;
  bool running_ = false;
};

// What a caller buffer held when it went to the device.  Big buffers: address, length, the quick fingerprint and the
// slices' hashes; the small per-cell arrays: address, length and one hash in `full`.
struct Key {
  const void *addr = nullptr;
  size_t n = 0;             // elements
  uint64_t quick = 0, full = 0;
  uint64_t slice[kSlices] = {};  // big buffers: the slices' hashes (`full` is their combination)
  bool valid = false;
  bool full_known = true;   // false: the hashes were never taken -- a full check then counts as "changed"

  // the cheap part: which buffer the hashes (taken before or after) belong to
  void stamp(const void *a, size_t count, uint64_t q) { addr = a; n = count; quick = q; valid = true; }
  template <typename T>
  void stamp(const T *a, size_t count) { stamp(a, count, fingerprint(a, count)); }
  // the cheap part alone: the first full check that reaches the key takes the hashes
  template <typename T>
  static Key cheap_only(const T *a, size_t count) { Key k; k.stamp(a, count); k.full_known = false; return k; }
  bool cheap_same(const void *a, size_t count, uint64_t q) const { return valid && addr == a && n == count && quick == q; }
};

// the whole content of one big buffer into its key (all slices, on the pool); begin / end so that the caller can do
// something else in between (the operators hash the points while they cross PCIe)
struct FullHash {
  SliceHasher sh;
  void begin(const void *data, size_t bytes) { SliceHasher::Req r; r.data = data; r.bytes = bytes; sh.begin(&r, 1, 0, kSlices); }
  void end(Key *k) {
    sh.end();
    std::memcpy(k->slice, sh.out[0], sizeof(k->slice));
    k->full = combine_slices(k->slice);
    k->full_known = true;
  }
};
template <typename T>
void full_hash_into(Key *k, const T *a, size_t n) {
  if (!a) { std::memset(k->slice, 0, sizeof(k->slice)); k->full = 1; k->full_known = true; return; }
  FullHash f;
  f.begin(a, n * sizeof(T));
  f.end(k);
}

// Does the caller's big buffer still hold what is resident?  Updates the key; `force`: recompute the hashes even if
// address, length and the quick fingerprint are unchanged.  *hashed: the key's hashes were taken by this call.
// `complete_unhashed`: a key whose hashes were never taken (Key::cheap_only) and whose cheap part still holds is
// completed by this check, not counted as changed.
template <typename T>
bool same_content(Key &k, const T *a, size_t n, bool force, bool complete_unhashed, bool *hashed) {
  const uint64_t q = fingerprint(a, n);
  const bool cheap_same = k.cheap_same(a, n, q);
  if (cheap_same && !force) return true;
  Key now;
  full_hash_into(&now, a, n);
  if (hashed) *hashed = true;
  bool same = k.valid && k.n == n && k.full_known && k.full == now.full;
  if (cheap_same && !k.full_known && complete_unhashed) same = true;
  now.stamp(a, n, q);
  k = now;
  return same;
}
template <typename T>
bool same_small(Key &k, const T *a, size_t n) {
  const uint64_t f = small_hash(a, n);
  const bool same = k.valid && k.addr == (const void *)a && k.n == n && k.full == f;
  k.stamp(a, n, 0); k.full = f; k.full_known = true;
  return same;
}
template <typename T>
void remember_small(Key &k, const T *a, size_t n) { (void)same_small(k, a, n); }
template <typename T>
void remember(Key &k, const T *a, size_t n) {
  full_hash_into(&k, a, n);
  k.stamp(a, n);
}

// ---- the rotating verification of one call ----------------------------------------------------------------------
// One watched big buffer as a call sees it: the key of what is resident, what the caller hands over now (elements as in
// the key, bytes per element), the part -- a bit of the operators' own -- it belongs to and its name for their message.
struct Watched { const Key *key; const void *addr; size_t n, elem; unsigned part; const char *name; };
using WatchTable = std::array<Watched, 4>;

// Slices [first, first + count) mod kSlices of the table's buffers against their keys: begin() hands them to the pool
// and returns (the operator evaluates meanwhile), end() joins and says what no longer matches.  A buffer is verified
// when its part is not among `fresh_parts` (keyed or uploaded by this very call), its key is valid with known hashes,
// the caller's address and length are the key's, and the address is not null.  Both inside one operator call; keys
// and buffers stay as they are in between.
class Verifier {
 public:
  struct Hit { const char *name; int slice; };
  struct Stale { unsigned parts = 0; int count = 0, n = 0; Hit at[4] = {}; };  // part bits; slices covered; per stale buffer its first stale slice
  bool begin(const WatchTable &table, unsigned fresh_parts, int first, int count) {  // false: nothing to verify, no job started
    SliceHasher::Req req[4];
    bool any = false;
    table_ = table;
    for (size_t b = 0; b < 4; b++) {
      Watched &w = table_[b];
      const bool on = !(fresh_parts & w.part) && w.key->valid && w.key->full_known && w.key->addr == w.addr && w.key->n == w.n && w.addr;
      if (!on) w.addr = nullptr;  // (left out of the job, and of end())
      req[b] = {w.addr, w.n * w.elem};
      any = any || on;
    }
    if (!any) return false;
    first_ = first; count_ = count;
    sh_.begin(req, 4, first, count);
    return true;
  }
  bool running() const { return sh_.running(); }
  Stale end() {
    Stale r;
    if (!sh_.running()) return r;
    sh_.end();
    r.count = count_;
    for (size_t b = 0; b < 4; b++)
      for (int c = 0; c < count_ && table_[b].addr; c++) {
        const int s = (first_ + c) % kSlices;
        if (sh_.out[b][s] == table_[b].key->slice[s]) continue;
        r.parts |= table_[b].part;
        r.at[r.n++] = {table_[b].name, s};
        break;
      }
    return r;
  }

 private:
  SliceHasher sh_;
  WatchTable table_ = {};
  int first_ = 0, count_ = 0;
};

}  // namespace nid_watch
