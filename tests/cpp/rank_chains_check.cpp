// lm::rank_chains (csrc/nid_lm_step.h: the one rank rule of nid_pyr_multistart_lm's survivors and the tracker's
// candidates) against an independent sort: a selection sort over (chi2 / n_active, index) pairs that knows nothing of
// std::stable_sort.  Fixed cases -- ties, n_active == 0 and below, NaN / +-inf chi2, nothing eligible, an empty batch -- and
// a few thousand LCG batches drawn from a handful of values, so that ties are the rule.  Built with
// -fsanitize=address,undefined by tests/test_multistart_cpu.py.  Exit code 0: all as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "nid_lm_step.h"

namespace {

uint64_t g_state = 20240611ull;
uint32_t draw(uint32_t n) {  // [0, n)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_state >> 33) % n);
}

// the rule, restated: eligible <=> n_active > 0 and chi2 is a finite number; the smallest chi2 / n_active first, the lower
// index first among equals
std::vector<int> restated(const std::vector<nid_ms_result> &res) {
  std::vector<int> pool, out;
  for (int k = 0; k < (int)res.size(); k++)
    if (res[k].n_active >= 1 && !std::isnan(res[k].chi2) && !std::isinf(res[k].chi2)) pool.push_back(k);
  while (!pool.empty()) {
    size_t at = 0;
    for (size_t i = 1; i < pool.size(); i++) {
      const double v = res[pool[i]].chi2 / (double)res[pool[i]].n_active, w = res[pool[at]].chi2 / (double)res[pool[at]].n_active;
      if (v < w || (v == w && pool[i] < pool[at])) at = i;
    }
    out.push_back(pool[at]);
    pool.erase(pool.begin() + (long)at);
  }
  return out;
}

int g_bad = 0, g_cases = 0, g_ties = 0;

nid_ms_result chain(double chi2, int n_active) {
  nid_ms_result r = {};
  r.chi2 = chi2;
  r.n_active = n_active;
  return r;
}

void check(const char *what, const std::vector<nid_ms_result> &res, const std::vector<int> *want = nullptr) {
  std::vector<int> order = {7, 7, 7};  // (stale contents: the helper starts from nothing)
  nid::lm::rank_chains(res.data(), (int)res.size(), order);
  const std::vector<int> ref = restated(res);
  g_cases++;
  for (size_t i = 0; i + 1 < ref.size(); i++)
    g_ties += res[ref[i]].chi2 / (double)res[ref[i]].n_active == res[ref[i + 1]].chi2 / (double)res[ref[i + 1]].n_active;
  if (order != ref || (want && order != *want)) {
    if (g_bad < 20) {
      std::printf("%s: got", what);
      for (int k : order) std::printf(" %d", k);
      std::printf(", want");
      for (int k : (want ? *want : ref)) std::printf(" %d", k);
      std::printf("\n");
    }
    g_bad++;
  }
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  {  // an empty batch; the data pointer of an empty vector may be null
    const std::vector<int> none;
    check("empty", {}, &none);
    std::vector<int> order = {1};
    nid::lm::rank_chains(nullptr, 0, order);
    if (!order.empty()) { std::printf("empty (null): order not cleared\n"); g_bad++; }
  }
  {  // ties: equal chi2 / n_active from different pairs, the lower index first
    const std::vector<int> want = {1, 3, 4, 0, 2};
    check("ties", {chain(6.0, 2), chain(2.0, 2), chain(9.0, 3), chain(1.0, 1), chain(4.0, 4)}, &want);
  }
  {  // n_active == 0 (and a negative count) is out whatever chi2 is; 0 / 0 never reaches the comparison
    const std::vector<int> want = {3, 1};
    check("n_active == 0", {chain(0.0, 0), chain(5.0, 1), chain(1.0, -3), chain(4.0, 1), chain(nan, 0)}, &want);
  }
  {  // NaN and both infinities are out; the largest finite double is in
    const std::vector<int> want = {4, 1, 5};
    check("NaN / inf", {chain(nan, 5), chain(3.0, 1), chain(inf, 2), chain(-inf, 2), chain(-1.0, 1), chain(1.7976931348623157e308, 1)}, &want);
  }
  {  // nothing eligible
    const std::vector<int> none;
    check("nothing eligible", {chain(nan, 1), chain(1.0, 0), chain(inf, 3)}, &none);
  }
  {  // one chain
    const std::vector<int> want = {0};
    check("one chain", {chain(2.5, 7)}, &want);
  }
  // random batches of 0 .. 66 chains (NID_MAX_BATCH + 2 and below) over few values: most neighbours tie
  const double values[8] = {0.0, 1.0, 2.0, 4.0, 8.0, nan, inf, -inf};
  const int counts[6] = {0, 1, 2, 4, 8, -1};
  for (int k = 0; k < 4000; k++) {
    std::vector<nid_ms_result> res(draw(67));
    for (nid_ms_result &r : res) r = chain(values[draw(8)], counts[draw(6)]);
    check("random", res);
  }
  std::printf("rank chains: %d cases, %d ties among ranked neighbours, %d failures\n", g_cases, g_ties, g_bad);
  return g_bad ? 1 : 0;
}
