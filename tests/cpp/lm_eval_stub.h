// lm_eval_stub.h -- what tests/cpp/lm_flows_caller.cpp asks of tests/cpp/lm_eval_stub.cpp beyond the entry points
// that host/g2o_min.cpp calls.
#ifndef LM_EVAL_STUB_H
#define LM_EVAL_STUB_H

#include <string>
#include <vector>

struct nid_multi;

int lm_stub_case_count();
const char *lm_stub_select_case(int k);  // makes case k the model, clears the call log; returns its name
int lm_stub_cell_num();                  // cells per image side (cell_num_ of the optimizer)
double lm_stub_href(int cell);           // NaN: an inactive cell (level 1 edge)
nid_multi *lm_stub_pair();               // stands for the frame pair on the device (SparseOptimizer::native_pair_)
const std::vector<std::string> &lm_stub_call_log();
// H and b of the whole image at a pose, as the fused entry points form them; not logged
void lm_stub_system(const double *pose7, double huber_delta, double *H36, double *b6);

#endif
