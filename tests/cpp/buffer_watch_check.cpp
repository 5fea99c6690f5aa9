// buffer_watch_check.cpp -- host/nid_buffer_watch.h alone (no operator, no HIP library, no stub): the slice arithmetic,
// the hashes, the pool of worker threads, fork(), the content keys and the rotating verification.  A stand-alone
// program: tests/test_host_cpu.py builds it under AddressSanitizer + UndefinedBehaviorSanitizer and under
// ThreadSanitizer and runs it once per pool setting (the pool reads NID_LEGACY_HASH_THREADS / NID_LEGACY_HASH_SPIN_US
// once per process).  Prints one line ending in "0 failures", or the failed checks and a non-zero exit status.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/wait.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "nid_buffer_watch.h"

using namespace nid_watch;

#if defined(__SANITIZE_THREAD__)
#define WATCH_CHECK_TSAN 1
#elif defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define WATCH_CHECK_TSAN 1
#endif
#endif

static long g_failures = 0, g_checks = 0;
#define CHECK(cond, ...)                                                                                   \
  do {                                                                                                     \
    g_checks++;                                                                                            \
    if (!(cond)) {                                                                                         \
      if (++g_failures <= 20) { std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                                                      \
  } while (0)

static int env_int(const char *name, int dflt, int lo, int hi) {
  const char *e = getenv(name);
  return e ? std::max(lo, std::min(hi, atoi(e))) : dflt;
}

static std::vector<unsigned char> pattern(size_t n, unsigned seed) {
  std::vector<unsigned char> b(n);
  uint32_t x = 2463534242u + seed;
  for (size_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; b[i] = (unsigned char)(x >> 11); }
  return b;
}

// ---- slices -------------------------------------------------------------------------------------------------------
static int check_slices() {
  std::vector<size_t> lens = {0, 1, 63, 64, 4096, 8191, 8192, 8193, (size_t)640 * 480 * 8, (size_t)640 * 480 * 24, (size_t)640 * 480 * 32};
  for (size_t k : {1, 2, 3, 7, 100, 1201})
    for (long d = -1; d <= 1; d++) lens.push_back((size_t)((long)(128 * 64 * k) + d));
  for (size_t bytes : lens) {
    size_t at = 0;
    for (int s = 0; s < kSlices; s++) {
      size_t lo = ~(size_t)0, hi = ~(size_t)0;
      slice_range(bytes, s, &lo, &hi);
      CHECK(lo == at && hi >= lo && hi <= bytes, "bytes %zu slice %d: [%zu, %zu) after %zu", bytes, s, lo, hi, at);
      if (s < kSlices - 1) CHECK(hi % 64 == 0, "bytes %zu slice %d ends at %zu", bytes, s, hi);
      if (bytes < 8192 && s < kSlices - 1) CHECK(hi == lo, "bytes %zu: slice %d is not empty", bytes, s);
      if (bytes >= 8192) CHECK(hi > lo, "bytes %zu: slice %d is empty", bytes, s);
      at = hi;
    }
    CHECK(at == bytes, "bytes %zu: the slices end at %zu", bytes, at);
  }
  return (int)lens.size();
}

// ---- hashes -------------------------------------------------------------------------------------------------------
// the combined hash of a buffer as SliceHasher takes it (slice s salted with bytes + s), on the calling thread
static uint64_t combined_alone(const unsigned char *b, size_t bytes, uint64_t *h) {
  for (int s = 0; s < kSlices; s++) {
    size_t lo, hi;
    slice_range(bytes, s, &lo, &hi);
    h[s] = hash_run(b + lo, hi - lo, (uint64_t)bytes + (uint64_t)s);
  }
  return combine_slices(h);
}

static long check_hashes() {
  long flips = 0;
  // every single bit of every length 1 .. 600 (75 words: nine rounds of the eight lanes, three `i % 8` tail words, and
  // all seven tail-byte counts); such a buffer is its last slice alone
  for (size_t len = 0; len <= 600; len++) {
    std::vector<unsigned char> b = pattern(len, (unsigned)len);
    uint64_t h[kSlices];
    const uint64_t all = combined_alone(b.data(), len, h), last = h[kSlices - 1];
    CHECK(all != 0 && small_hash(b.data(), len) != 0 && fingerprint(b.data(), len) != 0, "a zero digest at length %zu", len);
    CHECK(hash_run(b.data(), len, 1) != hash_run(b.data(), len, 2), "length %zu: the salt does not count", len);
    for (size_t bit = 0; bit < 8 * len; bit++) {
      b[bit / 8] ^= (unsigned char)(1u << (bit % 8));
      h[kSlices - 1] = hash_run(b.data(), len, (uint64_t)len + (uint64_t)(kSlices - 1));
      CHECK(h[kSlices - 1] != last, "length %zu bit %zu: the slice's hash stays", len, bit);
      CHECK(combine_slices(h) != all, "length %zu bit %zu: the combined hash stays", len, bit);
      b[bit / 8] ^= (unsigned char)(1u << (bit % 8));
      flips++;
    }
  }
  // a buffer of many slices: a bit of slice s changes slice s, no other, and the combination
  {
    const size_t bytes = 128 * 64 * 3 + 77;
    std::vector<unsigned char> b = pattern(bytes, 9);
    uint64_t h0[kSlices], h1[kSlices];
    const uint64_t all = combined_alone(b.data(), bytes, h0);
    for (int s = 0; s < kSlices; s++) {
      size_t lo, hi;
      slice_range(bytes, s, &lo, &hi);
      for (size_t at : {lo, lo + (hi - lo) / 2, hi - 1}) {
        b[at] ^= 0x10;
        CHECK(combined_alone(b.data(), bytes, h1) != all, "slice %d byte %zu: the combined hash stays", s, at);
        for (int t = 0; t < kSlices; t++) CHECK((h1[t] != h0[t]) == (t == s), "slice %d byte %zu: slice %d", s, at, t);
        b[at] ^= 0x10;
        flips++;
      }
    }
  }
  CHECK(fingerprint((const double *)nullptr, 5) == 1 && small_hash((const int *)nullptr, 5) == 1, "null arrays");
  // Digests of three fixed inputs, recorded from the functions as they stood in host/legacy_ops.cpp before they moved
  // here: a scratch program that compiled that text (fingerprint, hash_run, slice_range, combine_slices, small_hash of
  // the commit before this header existed, cut out by line number) printed hash_run(bytes, salt 5), small_hash,
  // fingerprint and the combination of the 128 slice hashes salted bytes + s for the inputs below (g++ -O1, x86-64).
  std::vector<unsigned char> A(1000);
  for (size_t i = 0; i < A.size(); i++) A[i] = (unsigned char)(i * 37 + 11);
  std::vector<double> B(20000);
  for (size_t i = 0; i < B.size(); i++) B[i] = 0.5 * (double)i - 3.0;
  std::vector<int32_t> C(77);
  for (size_t i = 0; i < C.size(); i++) C[i] = (int32_t)(i * i) - 1000;
  struct Gold { uint64_t run, small, quick, full; };
  const Gold gold[3] = {{0x95f71c147491d014ull, 0x8a056d8cd6a9d617ull, 0xd095a94986b079ebull, 0x4e365696f3f994f0ull},
                        {0x5ee5fe0fa4afc818ull, 0xc12c955307bc6ac4ull, 0xe24e14d7e1bbad1cull, 0xa086ed20c3f2a58bull},
                        {0x2848474f64a42a96ull, 0x09137c44ab27fb35ull, 0xf0ab332868c12446ull, 0xfc8131e89bac3f91ull}};
  auto digests = [&](int which, auto *a, size_t n) {
    const unsigned char *b = reinterpret_cast<const unsigned char *>(a);
    const size_t bytes = n * sizeof(*a);
    Key k;
    remember(k, a, n);  // (the pooled route: FullHash)
    uint64_t h[kSlices];
    const Gold &g = gold[which];
    CHECK(hash_run(b, bytes, 5) == g.run, "input %d: hash_run %016llx", which, (unsigned long long)hash_run(b, bytes, 5));
    CHECK(small_hash(a, n) == g.small, "input %d: small_hash %016llx", which, (unsigned long long)small_hash(a, n));
    CHECK(fingerprint(a, n) == g.quick && k.quick == g.quick, "input %d: fingerprint %016llx", which, (unsigned long long)fingerprint(a, n));
    CHECK(combined_alone(b, bytes, h) == g.full, "input %d: combined %016llx", which, (unsigned long long)combined_alone(b, bytes, h));
    CHECK(k.full == g.full && std::memcmp(h, k.slice, sizeof(h)) == 0, "input %d: the pooled hashes %016llx", which, (unsigned long long)k.full);
  };
  digests(0, A.data(), A.size());
  digests(1, B.data(), B.size());
  digests(2, C.data(), C.size());
  return flips;
}

// ---- pool ---------------------------------------------------------------------------------------------------------
// (what the parts write is plain memory, read behind finish(): under ThreadSanitizer that is the check)
static int check_pool(int threads, int spin_us) {
  HashPool &pool = HashPool::get();
  int jobs = 0;
  CHECK(pool.has_workers() == (threads > 0), "has_workers with %d threads", threads);
  for (int n : {0, 1, 2, 3, 7, 128, 512}) {
    std::vector<int> hits((size_t)n, 0);
    pool.run(n, [&](int k) { hits[(size_t)k]++; });
    for (int k = 0; k < n; k++) CHECK(hits[(size_t)k] == 1, "run(%d): part %d ran %d times", n, k, hits[(size_t)k]);
    jobs++;
  }
  // back to back, as the LM calls the operators: host work between start() and finish() and between the jobs
  const std::vector<unsigned char> work = pattern(512, 1);
  uint64_t sink = 0;
  long out[16];
  for (int it = 0; it < 3000; it++) {
    const int n = it % 13;
    for (int k = 0; k < 16; k++) out[k] = -1;
    pool.start(n, [&out, it](int k) { out[k] = 1000L * it + k; });
    sink += hash_run(work.data(), work.size() >> (it % 3), (uint64_t)it);
    pool.finish();
    for (int k = 0; k < 16; k++) CHECK(out[k] == (k < n ? 1000L * it + k : -1), "job %d of %d parts: part %d left %ld", it, n, k, out[k]);
    if (it % 5 == 0) sink += hash_run(work.data(), work.size(), sink);
    jobs++;
  }
  CHECK(sink != 0, "host work");
  // workers that have parked (nothing for longer than they poll) are woken by start(); a job started, left alone for
  // longer than they poll and finished late is complete
  const auto nap = std::chrono::microseconds(std::max(2000, 3 * spin_us));
  for (int it = 0; it < 10; it++) {
    std::vector<int> hits(40, 0);
    std::this_thread::sleep_for(nap);
    pool.start(40, [&](int k) { hits[(size_t)k]++; });
    std::this_thread::sleep_for(nap);
    pool.finish();
    for (int k = 0; k < 40; k++) CHECK(hits[(size_t)k] == 1, "late finish %d: part %d ran %d times", it, k, hits[(size_t)k]);
    jobs++;
  }
  return jobs;
}

// ---- fork ---------------------------------------------------------------------------------------------------------
static const char *check_fork(int threads) {
#ifdef WATCH_CHECK_TSAN
  (void)threads;
  return "not run under ThreadSanitizer";
#else
  HashPool &pool = HashPool::get();
  auto job_alone = [&pool](int n) {
    std::vector<int> hits((size_t)n, 0);
    pool.run(n, [&](int k) { hits[(size_t)k]++; });
    for (int k = 0; k < n; k++) if (hits[(size_t)k] != 1) return false;
    return true;
  };
  CHECK(job_alone(128), "the job before fork()");
  const pid_t pid = fork();
  CHECK(pid >= 0, "fork()");
  if (pid == 0) {  // no worker threads here, both locks free: the child does every part itself
    if (pool.has_workers()) _exit(21);
    if (!job_alone(128) || !job_alone(1)) _exit(22);
    Key k;
    const std::vector<unsigned char> b = pattern(70000, 4);
    remember(k, b.data(), b.size());
    uint64_t h[kSlices];
    _exit(k.full == combined_alone(b.data(), b.size(), h) ? 0 : 23);
  }
  CHECK(pool.has_workers() == (threads > 0) && job_alone(128), "the parent after fork()");
  int status = -1;
  CHECK(pid > 0 && waitpid(pid, &status, 0) == pid && WIFEXITED(status) && WEXITSTATUS(status) == 0, "the child's status %d", status);
  CHECK(job_alone(512), "the parent after the child");
  return "ok";
#endif
}

// ---- keys ---------------------------------------------------------------------------------------------------------
static void check_keys() {
  const size_t n = 20000;
  std::vector<double> buf(n), moved;
  for (size_t i = 0; i < n; i++) buf[i] = (double)(i * 7 % 256);
  const size_t off = 1;  // (the fingerprint samples k * (n - 1) / 63: 0, 317, ...)
  for (size_t k = 0; k < 64; k++) CHECK(k * (n - 1) / 63 != off, "index %zu is sampled", off);
  Key k;
  bool hashed = false;
  remember(k, buf.data(), n);
  const Key first = k;
  CHECK(k.valid && k.full_known && k.addr == buf.data() && k.n == n && k.cheap_same(buf.data(), n, fingerprint(buf.data(), n)), "remember");
  CHECK(same_content(k, buf.data(), n, false, false, &hashed) && !hashed, "an unchanged buffer, nothing hashed");
  moved = buf;
  CHECK(moved.data() != buf.data() && same_content(k, moved.data(), n, false, false, &hashed) && hashed && k.addr == moved.data() && k.full == first.full,
        "the same content at a new address");
  hashed = false;
  CHECK(!same_content(k, moved.data(), n - 1, false, false, &hashed) && hashed && k.n == n - 1, "a new length");
  remember(k, buf.data(), n);
  buf[off] += 1.0;  // off the sampled indices: the blind spot the rotation is for
  hashed = false;
  CHECK(same_content(k, buf.data(), n, false, false, &hashed) && !hashed && k.full == first.full, "a change off the samples, not forced");
  CHECK(!same_content(k, buf.data(), n, true, false, &hashed) && hashed && k.full != first.full, "a change off the samples, forced");
  CHECK(same_content(k, buf.data(), n, true, false, &hashed), "the key follows what it has seen");
  buf[0] += 1.0;  // a sampled index
  CHECK(!same_content(k, buf.data(), n, false, false, &hashed), "a change on a sample");
  // a key without hashes
  const Key full_now = k;
  k = Key::cheap_only(buf.data(), n);
  CHECK(k.valid && !k.full_known && k.full == 0 && k.addr == buf.data() && k.n == n && k.quick == full_now.quick, "cheap_only");
  hashed = false;
  CHECK(same_content(k, buf.data(), n, false, false, &hashed) && !hashed && !k.full_known, "a key without hashes, cheap check");
  CHECK(!same_content(k, buf.data(), n, true, false, &hashed) && hashed && k.full_known && k.full == full_now.full, "a key without hashes is changed by default");
  k = Key::cheap_only(buf.data(), n);
  CHECK(same_content(k, buf.data(), n, true, true, &hashed) && k.full_known && k.full == full_now.full &&
            std::memcmp(k.slice, full_now.slice, sizeof(k.slice)) == 0, "a key without hashes, completed");
  k = Key::cheap_only(buf.data(), n);
  CHECK(!same_content(k, moved.data(), n, false, true, &hashed), "a key without hashes at another address is not completed");
  k = Key();
  CHECK(!same_content(k, buf.data(), n, false, true, &hashed) && k.valid, "an empty key");
  // the small arrays: address, length and hash
  std::vector<int> cnt(256, 300), cnt2;
  Key s;
  CHECK(!same_small(s, cnt.data(), cnt.size()) && s.valid && s.full_known && s.quick == 0 && s.full == small_hash(cnt.data(), cnt.size()), "same_small on an empty key");
  CHECK(same_small(s, cnt.data(), cnt.size()), "same_small, unchanged");
  cnt2 = cnt;
  CHECK(!same_small(s, cnt2.data(), cnt2.size()) && same_small(s, cnt2.data(), cnt2.size()), "same_small keys on the address");
  CHECK(!same_small(s, cnt2.data(), cnt2.size() - 1) && s.n == cnt2.size() - 1, "same_small keys on the length");
  remember_small(s, cnt.data(), cnt.size());
  cnt[200] = 299;
  CHECK(!same_small(s, cnt.data(), cnt.size()) && same_small(s, cnt.data(), cnt.size()), "same_small keys on the content");
  remember(k, (const double *)nullptr, 0);
  CHECK(k.valid && k.addr == nullptr && k.full == 1 && k.quick == 1 && k.full_known, "the key of no buffer");
}

// ---- rotation -----------------------------------------------------------------------------------------------------
static int check_rotation() {
  const size_t N = 4800;  // 38 400 bytes and up: 127 slices of 256 bytes or more and a longer last one
  const size_t cnt[4] = {N, 3 * N, N, 4 * N};
  const unsigned part[4] = {1, 1, 2, 4};
  const char *name[4] = {"im0", "points3d", "im1", "bs_ref"};
  std::vector<double> buf[4];
  Key key[4];
  for (int b = 0; b < 4; b++) {
    buf[b].resize(cnt[b]);
    for (size_t i = 0; i < cnt[b]; i++) buf[b][i] = (double)((i * 2654435761u + (unsigned)b) % 1021);
    remember(key[b], buf[b].data(), cnt[b]);
  }
  auto table = [&] {
    WatchTable t;
    for (int b = 0; b < 4; b++) t[(size_t)b] = Watched{&key[b], buf[b].data(), cnt[b], sizeof(double), part[b], name[b]};
    return t;
  };
  Verifier v;
  int calls = 0;
  {
    const Verifier::Stale r = [&] { CHECK(v.begin(table(), 0, 0, kSlices), "nothing fresh: a job"); return v.end(); }();
    CHECK(r.parts == 0 && r.n == 0 && r.count == kSlices, "unchanged buffers: parts %u", r.parts);
  }
  for (int b = 0; b < 4; b++)
    for (int s : {0, 1, 64, 126, 127}) {
      size_t lo, hi;
      slice_range(cnt[b] * sizeof(double), s, &lo, &hi);
      unsigned char *byte = reinterpret_cast<unsigned char *>(buf[b].data()) + lo + (size_t)(b + s) % (hi - lo);
      *byte ^= 0x04;
      for (int count : {1, 3, 6, kSlices})
        for (int cursor : {0, 60, 125, 126, 127}) {
          int reported = 0;
          for (int c = 0; c * count < kSlices + count; c++) {  // one round and a little: some windows wrap
            const int first = (cursor + c * count) % kSlices;
            const bool inside = (s - first + kSlices) % kSlices < count;
            CHECK(v.begin(table(), 0, first, count) && v.running(), "a job for slices %d + %d", first, count);
            const Verifier::Stale r = v.end();
            calls++;
            CHECK(!v.running() && r.count == count, "the job of slices %d + %d ended", first, count);
            if (inside) {
              CHECK(r.parts == part[b] && r.n == 1 && r.at[0].slice == s && std::strcmp(r.at[0].name, name[b]) == 0,
                    "buffer %d slice %d in window %d + %d: parts %u, %d stale, slice %d", b, s, first, count, r.parts, r.n, r.at[0].slice);
              reported++;
            } else {
              CHECK(r.parts == 0 && r.n == 0, "buffer %d slice %d outside window %d + %d: parts %u", b, s, first, count, r.parts);
            }
          }
          CHECK(reported >= 1, "buffer %d slice %d, %d per call from %d: never reported", b, s, count, cursor);
        }
      // left out: a fresh part, another address, a key without hashes
      {
        CHECK(v.begin(table(), part[b], 0, kSlices), "the other parts are on");
        const Verifier::Stale r = v.end();
        CHECK(r.parts == 0, "a fresh part is left out: parts %u", r.parts);
      }
      {
        std::vector<double> copy = buf[b];
        WatchTable t = table();
        t[(size_t)b].addr = copy.data();
        CHECK(v.begin(t, 0, 0, kSlices), "the other buffers are on");
        const Verifier::Stale r = v.end();
        CHECK(r.parts == 0, "a buffer at another address than its key's is left out: parts %u", r.parts);
        t = table();
        t[(size_t)b].n--;
        v.begin(t, 0, 0, kSlices);
        CHECK(v.end().parts == 0, "a buffer of another length than its key's is left out");
      }
      {
        Key unhashed = key[b];
        unhashed.full_known = false;
        WatchTable t = table();
        t[(size_t)b].key = &unhashed;
        v.begin(t, 0, 0, kSlices);
        CHECK(v.end().parts == 0, "a key without hashes is left out");
        Key invalid = key[b];
        invalid.valid = false;
        t[(size_t)b].key = &invalid;
        v.begin(t, 0, 0, kSlices);
        CHECK(v.end().parts == 0, "an invalid key is left out");
      }
      calls += 5;
      *byte ^= 0x04;
    }
  // two stale buffers of two parts in one call: both named, each with its first stale slice of the window
  {
    size_t lo, hi;
    slice_range(cnt[1] * sizeof(double), 9, &lo, &hi);
    reinterpret_cast<unsigned char *>(buf[1].data())[lo] ^= 1;
    reinterpret_cast<unsigned char *>(buf[1].data())[hi] ^= 1;  // slice 10
    slice_range(cnt[3] * sizeof(double), 127, &lo, &hi);
    reinterpret_cast<unsigned char *>(buf[3].data())[hi - 1] ^= 1;
    v.begin(table(), 0, 120, 20);  // slices 120 .. 127, 0 .. 11
    const Verifier::Stale r = v.end();
    CHECK(r.parts == (part[1] | part[3]) && r.n == 2 && r.at[0].slice == 9 && !std::strcmp(r.at[0].name, "points3d") &&
              r.at[1].slice == 127 && !std::strcmp(r.at[1].name, "bs_ref"), "two stale buffers: parts %u, %d stale", r.parts, r.n);
    remember(key[1], buf[1].data(), cnt[1]);
    remember(key[3], buf[3].data(), cnt[3]);
    calls++;
  }
  // no buffer (null at both ends) is left out; with nothing on, no job is started and the pool stays free
  {
    Key none;
    remember(none, (const double *)nullptr, 0);
    WatchTable t = table();
    t[2] = Watched{&none, nullptr, 0, sizeof(double), part[2], name[2]};
    CHECK(v.begin(t, part[0] | part[3], 0, kSlices) == false && !v.running(), "a null buffer alone starts no job");
    CHECK(v.begin(table(), 1 | 2 | 4, 0, 3) == false && !v.running(), "every part fresh: no job");
    const Verifier::Stale r = v.end();
    CHECK(r.parts == 0 && r.n == 0 && r.count == 0, "end() without a job");
    int ran = 0;
    HashPool::get().run(1, [&](int) { ran++; });  // (would wait for ever on a pool that a job still held)
    CHECK(ran == 1, "the pool is free");
  }
  return calls;
}

int main() {
  alarm(240);  // a deadlock ends the program with SIGALRM instead of hanging the test
  const int threads = env_int("NID_LEGACY_HASH_THREADS", 3, 0, 15), spin_us = env_int("NID_LEGACY_HASH_SPIN_US", 150, 0, 100000);
  const int lens = check_slices();
  const long flips = check_hashes();
  const int jobs = check_pool(threads, spin_us);
  const char *forked = check_fork(threads);
  check_keys();
  const int calls = check_rotation();
  std::printf("buffer watch (%d workers, %d us of polling): %d lengths sliced, %ld bits flipped, %d pool jobs, fork %s, %d verifying calls, %ld checks, %ld failures\n",
              threads, spin_us, lens, flips, jobs, forked, calls, g_checks, g_failures);
  return g_failures ? 1 : 0;
}
