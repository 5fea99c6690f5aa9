// lm::lm_step (csrc/nid_lm_step.h) driven over the model cases of tests/cpp/lm_eval_stub.cpp, the ones
// tests/golden/lm_flows_trace.json records the shipped LM of host/g2o_min.cpp on: a chain from {0,0,0,1,0,0,0}, 30
// iterations, delta sqrt(0.95); each round the stub's nid_multi_normal_equations(want_jac = 1) at the pose the chain asked
// for, packed into a reduced block.  Behind every step that leaves the chain running the same (H + lambda I, b) goes to
// g2o::LinearSolverDense().solve.  Linked with lm_eval_stub.cpp and host/g2o_min.cpp, built with
// -fsanitize=address,undefined and read, together with the golden file, by tests/test_lm_step_cpu.py.
// Prints one JSON object: per case the trials of every outer iteration, the final status and pose (doubles as %a) and per
// step {outer (the outer iteration the solved trial belongs to), lambda, max_diag, ldlt_ok, dense_ok, rel_dx}.
// fail_start and fail_trial are left out by name: a failing evaluation is not an input lm_step has.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "g2o_min/g2o_min.h"
#include "lm_eval_stub.h"
#include "nid/nid_multi.h"
#include "nid_lm_step.h"

int main() {
  const double pose0[7] = {0, 0, 0, 1, 0, 0, 0};
  const double delta = std::sqrt(0.95);
  const int iterations = 30;
  bool first_case = true;
  std::printf("{");
  for (int c = 0; c < lm_stub_case_count(); c++) {
    const std::string name = lm_stub_select_case(c);
    if (name == "fail_start" || name == "fail_trial") continue;
    nid_ms_state S;
    nid::lm::lm_init(&S, pose0, iterations, 0);
    std::vector<int> trials;
    std::string steps;
    int cur = 0;
    for (int round = 0; round < 1 + nid::lm::kMaxTrials * iterations; round++) {
      double H36[36], b6[6], chi2 = 0, r[32] = {0};
      int32_t na = 0;
      const int rc = nid_multi_normal_equations(lm_stub_pair(), S.rec_q, 1, delta, H36, b6, &chi2, &na);
      if (rc != NID_OK) {
        std::fprintf(stderr, "%s: the evaluation failed in round %d\n", name.c_str(), round);
        return 2;
      }
      r[0] = chi2;
      for (int i = 0; i < 6; i++) r[1 + i] = b6[i];
      for (int i = 0, k = 7; i < 6; i++)
        for (int j = i; j < 6; j++, k++) r[k] = H36[i * 6 + j];
      r[28] = na;
      const bool running = nid::lm::lm_step(&S, r);
      if (S.flags & (NID_MS_F_ACCEPT | NID_MS_F_REJECT)) cur++;
      if (S.flags & NID_MS_F_OUTER_END) { trials.push_back(cur); cur = 0; }
      if (!running) break;
      // the solve this step made, handed to the host stack's solver
      double A[36], xd[6] = {0, 0, 0, 0, 0, 0}, maxd = 0;
      for (int i = 0, k = 0; i < 6; i++)
        for (int j = i; j < 6; j++, k++) A[i * 6 + j] = A[j * 6 + i] = S.H[k];
      for (int i = 0; i < 6; i++) { maxd = std::fmax(maxd, std::fabs(A[i * 6 + i])); A[i * 6 + i] += S.lambda; }
      const bool dense_ok = g2o::LinearSolverDense().solve(A, xd, S.b);
      double dx = 0, xn = 0;
      for (int i = 0; i < 6; i++) { dx = std::fmax(dx, std::fabs(S.x[i] - xd[i])); xn = std::fmax(xn, std::fabs(xd[i])); }
      const double rel = S.solve_ok && dense_ok ? (xn > 0 ? dx / xn : dx) : 0.0;
      char buf[256];
      std::snprintf(buf, sizeof(buf), "%s\n    {\"outer\": %d, \"lambda\": \"%a\", \"max_diag\": \"%a\", \"ldlt_ok\": %s, \"dense_ok\": %s, \"rel_dx\": \"%a\"}",
                    steps.empty() ? "" : ",", S.outer_done, S.lambda, maxd,
                    S.solve_ok ? "true" : "false", dense_ok ? "true" : "false", rel);
      steps += buf;
    }
    std::printf("%s\n \"%s\": {\"trials\": [", first_case ? "" : ",", name.c_str());
    first_case = false;
    for (size_t k = 0; k < trials.size(); k++) std::printf("%s%d", k ? ", " : "", trials[k]);
    std::printf("], \"status\": %d, \"final_pose\": [", S.status);
    for (int i = 0; i < 7; i++) std::printf("%s\"%a\"", i ? ", " : "", S.pose7[i]);
    std::printf("],\n  \"steps\": [%s]}", steps.c_str());
  }
  std::printf("\n}\n");
  return 0;
}
