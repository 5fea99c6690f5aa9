// lm_flows_caller.cpp -- SparseOptimizer::optimize() of host/g2o_min.cpp for every LM flow (fused 0..4 of
// nid_pose_problem), set up the way nid_host_run_lm sets the solver up, over the model cases of
// tests/cpp/lm_eval_stub.cpp, without a GPU.  Linked with host/g2o_min.cpp and the stub and nothing else of the
// product; built and run by tests/test_lm_flows_cpu.py under -fsanitize=address,undefined.
// Prints one JSON object: per case and flow the return value, every outer iteration's record (doubles as %a), the
// final pose and the stub's call log.  tests/golden/lm_flows_trace.json is this output.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <sstream>

#include "g2o_min/g2o_min.h"
#include "lm_eval_stub.h"

// Fresh memory is zero here, so that a member the code under test reads before it has written it holds the same in
// every run: the recorded trace was taken from a g2o_min.cpp whose speculative flows started a chain from the block
// solver's never-written x.
void *operator new(std::size_t n) {
  void *p = std::calloc(1, n ? n : 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void *operator new[](std::size_t n) { return operator new(n); }
void operator delete(void *p) noexcept { std::free(p); }
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete(void *p, std::size_t) noexcept { std::free(p); }
void operator delete[](void *p, std::size_t) noexcept { std::free(p); }

static void print_doubles(const double *v, int n) {
  std::printf("[");
  for (int i = 0; i < n; i++) std::printf("%s\"%a\"", i ? ", " : "", v[i]);
  std::printf("]");
}

static void run(int fused, int iterations) {
  const int cell = lm_stub_cell_num();
  g2o::SparseOptimizer optimizer;
  g2o::BlockSolver_6_X::LinearSolverType *linearSolver = new g2o::LinearSolverDense();
  g2o::BlockSolver_6_X *solver_ptr = new g2o::BlockSolver_6_X(linearSolver);
  g2o::OptimizationAlgorithmLevenberg *solver = new g2o::OptimizationAlgorithmLevenberg(solver_ptr);
  solver->setFusedNormalEquations(fused != 0);
  solver->setSpeculativeTrials(fused == 2 || fused == 3);
  solver->setSpeculativeJacobian(fused >= 3);
  optimizer.setAlgorithm(solver);
  optimizer.setVerbose(true);
  optimizer.setComputeBatchStatistics(true);
  std::ostringstream log;
  optimizer.setLogStream(&log);

  const double pose0[7] = {0, 0, 0, 1, 0, 0, 0};
  g2o::VertexSE3Expmap *vSE3 = new g2o::VertexSE3Expmap();
  vSE3->setEstimate(g2o::SE3Quat::fromPose7(pose0));
  vSE3->setId(0);
  vSE3->setFixed(false);
  optimizer.addVertex(vSE3);

  // the per-edge flow hands these to CudaComputeH, which here reads none of them but Href's cell count
  double dummy[1] = {0}, intrinsics[5] = {1, 1, 0, 0, 1};
  int idummy[1] = {0};
  std::vector<double> Href(cell * cell);
  std::vector<int> bs_counter(cell * cell, 1);
  for (int c = 0; c < cell * cell; c++) Href[c] = lm_stub_href(c);
  optimizer.im0_ = dummy; optimizer.im1_ = dummy; optimizer.points3d_ = dummy;
  optimizer.rows_ = cell; optimizer.cols_ = cell; optimizer.camera_intrincis_ = intrinsics;
  optimizer.bin_num_ = 8; optimizer.bs_degree_ = 3; optimizer.cell_num_ = cell;
  optimizer.bs_counter_ = bs_counter.data(); optimizer.bs_value_ref_ = dummy;
  optimizer.bs_index_ref_ = idummy; optimizer.Href_ = Href.data();
  optimizer.native_pair_ = fused != 0 ? lm_stub_pair() : nullptr;

  const double deltaNID = std::sqrt(0.95);
  for (int c = 0; c < cell * cell; c++) {
    g2o::EdgeSE3ProjectIntensityOnlyPoseNID *e = new g2o::EdgeSE3ProjectIntensityOnlyPoseNID();
    e->setVertex(0, optimizer.vertex(0));
    e->use_CPU_ = false;
    e->set_bspline_relates(3, 8);
    g2o::RobustKernelHuber *rk = new g2o::RobustKernelHuber;
    e->setRobustKernel(rk);
    rk->setDelta(deltaNID);
    e->setInformation(1.0);
    if (std::isnan(Href[c])) e->setLevel(1);
    else e->set_href(Href[c]);
    optimizer.addEdge(e);
  }
  optimizer.initializeOptimization(0);
  const int done = optimizer.optimize(iterations);

  std::printf("{\"ret\": %d, \"iterations\": [", done);
  const std::vector<g2o::IterationRecord> &tr = optimizer.trace();
  const double *prev_pose = pose0;
  for (size_t k = 0; k < tr.size(); k++) {
    // Did the FIRST solve of this outer iteration's trial chain succeed?  It is (H + lambda I) x = b at the pose and
    // the lambda the iteration before ended with; the first iteration's lambda is not recorded anywhere.
    const char *first_solve = "null";
    if (k > 0) {
      double H[36], b[6], x[6];
      lm_stub_system(prev_pose, deltaNID, H, b);
      for (int j = 0; j < 6; j++) H[j * 6 + j] += tr[k - 1].lambda;
      first_solve = g2o::LinearSolverDense().solve(H, x, b) ? "true" : "false";
    }
    std::printf("%s\n    {\"lm_trials\": %d, \"first_solve_ok\": %s, \"chi2\": \"%a\", \"lambda\": \"%a\", \"rho\": \"%a\", \"pose7\": ",
                k ? "," : "", tr[k].levenbergIter, first_solve, tr[k].chi2, tr[k].lambda, tr[k].rho);
    print_doubles(tr[k].pose7, 7);
    std::printf("}");
    prev_pose = tr[k].pose7;
  }
  double final_pose[7];
  vSE3->estimate().toPose7(final_pose);
  std::printf("],\n   \"final_pose\": ");
  print_doubles(final_pose, 7);
  std::printf(",\n   \"calls\": [");
  const std::vector<std::string> &calls = lm_stub_call_log();
  for (size_t k = 0; k < calls.size(); k++) std::printf("%s\"%s\"", k ? ", " : "", calls[k].c_str());
  std::printf("]}");
}

int main() {
  std::printf("{");
  for (int c = 0; c < lm_stub_case_count(); c++) {
    for (int fused = 0; fused <= 4; fused++) {
      const char *name = lm_stub_select_case(c);
      if (fused == 0) std::printf("%s\n \"%s\": {", c ? "," : "", name);
      std::printf("%s\n  \"%d\": ", fused ? "," : "", fused);
      run(fused, 30);
    }
    std::printf("\n }");
  }
  std::printf("\n}\n");
  return 0;
}
