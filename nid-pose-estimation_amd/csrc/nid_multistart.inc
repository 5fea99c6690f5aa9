// nid_multistart.inc -- many Levenberg-Marquardt chains at once, stepped on the device (include/nid/nid_multistart.h):
// k_lm_step and the round loop.  Part of nid_capi.hip's translation unit (included behind the pipelined loops).
//
// A ROUND is [k_eval2 grid of n poses with the Jacobian -> k_repair -> k_lm_step] on one in-order stream.  The grid's
// per-pose records live in a device array of the call's own for EVERY n (launches of <= kMaxBatch poses normally carry
// them in the kernel arguments, which would not see the poses k_lm_step writes): the EXT instantiations of the 128- /
// 256-thread kernels, whatever n is, so a chain gives the same bits alone and beside 255 others.  Each chain owns its
// per-cell blocks, group sums, tickets (zero between grids, as the kernels leave them), its record -- a PosePool of the
// call's own, like the fused pipeline's -- and its result block; the public slots are neither used nor marked.
// k_lm_step runs lm_step() of nid_lm_step.h for every chain on the block its pose just produced (k_repair is in front
// of it in the stream: a repaired cell's contribution is in), writes the chain's state and the `pose` member of its
// record, one trace record if asked, and adds the chains that are still running to the round's word.  A finished chain
// is frozen, so what the host enqueues past the end changes nothing: it enqueues chunks of rounds and reads the last
// word between chunks.

namespace {

static_assert(sizeof(nid_ms_state) == 72 * 8 + 12 * 4, "nid_ms_state: doubles then 32-bit integers, no padding");
static_assert(sizeof(nid_ms_trace) == 10 * 8 + 2 * 4 && sizeof(nid_ms_result) == 9 * 8 + 4 * 4, "trace / result layout");
static_assert(sizeof(((Pose *)nullptr)->q) == 7 * 8 && sizeof(((Pose *)nullptr)->M) == 12 * 8, "the pose record lm::pose_record fills");

struct MsStepArgs {
  nid_ms_state *state;      // [n]
  SlotArgs *recs;           // [n]: the records the next grid reads
  const double *reduced;    // [n][kReducedLen]: this round's result blocks
  nid_ms_trace *trace;      // this round's [n] trace records, or null
  unsigned *running;        // this round's word: chains still running behind it
  int n;
};

// one thread per chain; plain loads and stores
__global__ void __launch_bounds__(64) k_lm_step(const MsStepArgs A) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= A.n) return;
  nid_ms_state *G = A.state + i;
  if (G->status != NID_MS_RUNNING) {  // frozen: nothing of the chain changes
    if (A.trace) { nid_ms_state S = *G; lm::lm_trace(&S, A.trace + i); }
    return;
  }
  nid_ms_state S = *G;
  double r[kReducedLen];
  for (int k = 0; k < kReducedLen; k++) r[k] = A.reduced[(size_t)i * kReducedLen + k];
  const bool running = lm::lm_step(&S, r);
  *G = S;
  if (running) {
    Pose &P = A.recs[i].pose;
    for (int k = 0; k < 7; k++) P.q[k] = S.rec_q[k];
    for (int k = 0; k < 12; k++) P.M[k] = S.rec_M[k];
    P.mode = S.rec_mode;
    atomicAdd(A.running, 1u);
  }
  if (A.trace) lm::lm_trace(&S, A.trace + i);
}

// buffers for `chains` chains and `rounds` rounds (grow only; the trace only when asked for).  A step that fails leaves
// the count it was growing at zero, and the next call makes that part anew.
int ensure_ms_pool(nid_ctx *ctx, int chains, int rounds, bool trace) {
  nid_ctx::MsPool &Q = ctx->ms;
  if (Q.chains < chains) {
    resident_retire(ctx);  // (a release waits for the whole device)
    rounds = std::max(rounds, Q.rounds);
    Q = nid_ctx::MsPool();
    const size_t n = (size_t)chains;
    int rc;
    if ((rc = pool_ensure(ctx, Q.poses, n, true))) return rc;
    NID_HIP(ctx, Q.reduced.alloc(n * kReducedLen));
    NID_HIP(ctx, Q.state_dev.alloc(n));
    NID_HIP(ctx, Q.state_host.alloc(n));
    Q.chains = chains;
  }
  if (Q.rounds < rounds) {
    resident_retire(ctx);
    Q.rounds = 0;
    NID_HIP(ctx, Q.running_dev.alloc((size_t)rounds));
    NID_HIP(ctx, Q.running_host.alloc((size_t)rounds));
    Q.rounds = rounds;
  }
  if (trace && Q.trace_dev.size() < (size_t)rounds * chains) {
    resident_retire(ctx);
    NID_HIP(ctx, Q.trace_dev.alloc((size_t)rounds * chains));
  }
  return NID_OK;
}

// rounds the host enqueues between two looks at the running word: a look costs a stream synchronisation (~15 us), a round
// too many costs a grid -- few chains: cheap grids, look rarely; many: look after every round.  NID_MS_CHUNK overrides
// (the result does not depend on it).
int ms_chunk(int n) {
  const char *e = getenv("NID_MS_CHUNK");
  if (e && atoi(e) > 0) return atoi(e);
  return std::max(1, std::min(8, 64 / n));
}

}  // namespace

extern "C" {

int nid_lm_step_host(nid_ms_state *state, const double *reduced32) {
  if (!state || !reduced32) return NID_ERR_INVALID_ARG;
  return lm::lm_step(state, reduced32) ? 1 : 0;
}

// k_lm_step alone on what the caller brings: buffers of the call's own (the context's multi-start pool is not touched),
// the records uploaded first so that one the kernel leaves alone comes back as it went in
int nid_lm_step_device(nid_ctx *ctx, nid_ms_state *states, const double *reduced32, int n, double *rec19, int32_t *rec_mode,
                       nid_ms_trace *trace, unsigned *running) {
  if (!ctx || !states || !reduced32 || !rec19 || !rec_mode || !running || n < 1 || n > (1 << 16)) return NID_ERR_INVALID_ARG;
  if (any_pending(ctx)) { ctx->last_error = "a launch is pending: nid_wait() it first"; return NID_ERR_STATE; }
  NID_HIP(ctx, hipSetDevice(ctx->cfg.device));
  resident_retire(ctx);  // (the buffers below are allocated and released here: a release waits for the whole device)
  const size_t m = (size_t)n;
  DevBuf<nid_ms_state> state_dev;
  DevBuf<SlotArgs> recs_dev;
  DevBuf<double> reduced_dev;
  DevBuf<nid_ms_trace> trace_dev;
  DevBuf<unsigned> running_dev;
  NID_HIP(ctx, state_dev.alloc(m));
  NID_HIP(ctx, recs_dev.alloc(m));
  NID_HIP(ctx, reduced_dev.alloc(m * kReducedLen));
  NID_HIP(ctx, running_dev.alloc(1));
  if (trace) NID_HIP(ctx, trace_dev.alloc(m));
  std::vector<SlotArgs> recs(m);  // (value-initialised: only the `pose` member means anything here)
  for (size_t k = 0; k < m; k++) {
    Pose &P = recs[k].pose;
    for (int i = 0; i < 7; i++) P.q[i] = rec19[19 * k + i];
    for (int i = 0; i < 12; i++) P.M[i] = rec19[19 * k + 7 + i];
    P.mode = rec_mode[k];
  }
  hipStream_t st = ctx->stream;
  auto drain = [&]() { (void)hipStreamSynchronize(st); };  // (the buffers go when this call returns: nothing may still use them)
  hipError_t e = hipMemcpyAsync(state_dev, states, m * sizeof(nid_ms_state), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(recs_dev, recs.data(), m * sizeof(SlotArgs), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(reduced_dev, reduced32, m * kReducedLen * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(running_dev, 0, sizeof(unsigned), st);
  if (e == hipSuccess) {
    MsStepArgs A{state_dev, recs_dev, reduced_dev, trace ? trace_dev.get() : nullptr, running_dev, n};
    hipLaunchKernelGGL(k_lm_step, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, A);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(states, state_dev, m * sizeof(nid_ms_state), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(recs.data(), recs_dev, m * sizeof(SlotArgs), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && trace) e = hipMemcpyAsync(trace, trace_dev, m * sizeof(nid_ms_trace), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(running, running_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) {
    drain();
    ctx->last_error = std::string("nid_lm_step_device: ") + hipGetErrorString(e);
    return NID_ERR_HIP;
  }
  NID_HIP(ctx, hipStreamSynchronize(st));
  for (size_t k = 0; k < m; k++) {
    const Pose &P = recs[k].pose;
    for (int i = 0; i < 7; i++) rec19[19 * k + i] = P.q[i];
    for (int i = 0; i < 12; i++) rec19[19 * k + 7 + i] = P.M[i];
    rec_mode[k] = P.mode;
  }
  return NID_OK;
}

int nid_multistart_lm(nid_ctx *ctx, const double *poses7_in, int n, int iterations, double delta, int max_rounds,
                      nid_ms_result *results, int *best, nid_ms_trace *trace, int *rounds_done) {
  if (!ctx || !poses7_in || !results || n < 1 || n > kMaxBatchExt || iterations < 1 || max_rounds < 0) return NID_ERR_INVALID_ARG;
  if (iterations > (1 << 20)) return NID_ERR_INVALID_ARG;
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (any_pending(ctx)) { ctx->last_error = "a launch is pending: nid_wait() it first"; return NID_ERR_STATE; }
  if (ctx->dbg_enabled || ctx->dbg_stamps) { ctx->last_error = "nid_multistart_lm: switch the per-pixel dump / phase stamps off"; return NID_ERR_STATE; }
  NID_HIP(ctx, hipSetDevice(ctx->cfg.device));
  const int rounds_cap = max_rounds > 0 ? max_rounds : 1 + lm::kMaxTrials * iterations;
  if ((rc = ensure_ms_pool(ctx, n, rounds_cap, trace != nullptr))) return rc;
  nid_ctx::MsPool &Q = ctx->ms;
  hipStream_t st = ctx->stream;

  // records and states of the start poses: pinned mirrors, one copy each (the records': with the first grid, below)
  nid_ms_state *state_host = Q.state_host;
  for (int k = 0; k < n; k++) {
    nid_ms_state &S = state_host[k];
    lm::lm_init(&S, poses7_in + 7 * (size_t)k, iterations, ctx->xform);
    SlotArgs &A = Q.poses.rec_host[k];
    pool_record(ctx, Q.poses, (size_t)k, Q.reduced + (size_t)k * kReducedLen, &A);
    for (int i = 0; i < 7; i++) A.pose.q[i] = S.rec_q[i];
    for (int i = 0; i < 12; i++) A.pose.M[i] = S.rec_M[i];
    A.pose.mode = S.rec_mode;
  }
  NID_HIP(ctx, hipMemcpyAsync(Q.state_dev, state_host, (size_t)n * sizeof(nid_ms_state), hipMemcpyHostToDevice, st));
  NID_HIP(ctx, hipMemsetAsync(Q.running_dev, 0, (size_t)rounds_cap * sizeof(unsigned), st));

  EvalParams P{};
  fill_common_params(ctx, delta, &P);
  const int chunk = ms_chunk(n);
  int enqueued = 0, done = -1;  // done: rounds until the last chain finished
  auto drain = [&]() { (void)hipStreamSynchronize(st); };  // (an error must not leave grids of this call behind)
  while (enqueued < rounds_cap && done < 0) {
    const int upto = std::min(rounds_cap, enqueued + chunk);
    for (int r = enqueued; r < upto; r++) {
      // records on the device for every n: see the head of this file (launch_eval2 keeps such a grid at <= 256 threads);
      // ONE upload, with the call's first grid -- k_lm_step keeps the poses there up to date
      if ((rc = launch_records(ctx, P, r == 0 ? Q.poses.rec_host : nullptr, n, Q.poses.rec_dev, true, true, st))) { drain(); return rc; }
      MsStepArgs A{Q.state_dev, Q.poses.rec_dev, Q.reduced, trace ? Q.trace_dev + (size_t)r * n : nullptr, Q.running_dev + r, n};
      hipLaunchKernelGGL(k_lm_step, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, A);
    }
    if (hipGetLastError() != hipSuccess) { drain(); ctx->last_error = "k_lm_step launch failed"; return NID_ERR_HIP;}
    if (hipMemcpyAsync(Q.running_host + enqueued, Q.running_dev + enqueued, (size_t)(upto - enqueued) * sizeof(unsigned),
                       hipMemcpyDeviceToHost, st) != hipSuccess) { drain(); ctx->last_error = "hipMemcpyAsync(running words)"; return NID_ERR_HIP; }
    NID_HIP(ctx, hipStreamSynchronize(st));
    for (int r = enqueued; r < upto && done < 0; r++)
      if (Q.running_host[(size_t)r] == 0u) done = r + 1;
    enqueued = upto;
  }
  const int rounds = done > 0 ? done : enqueued;
  NID_HIP(ctx, hipMemcpy(state_host, Q.state_dev, (size_t)n * sizeof(nid_ms_state), hipMemcpyDeviceToHost));
  if (trace) {
    NID_HIP(ctx, hipMemcpy(trace, Q.trace_dev, (size_t)rounds * n * sizeof(nid_ms_trace), hipMemcpyDeviceToHost));
    std::memset(trace + (size_t)rounds * n, 0, (size_t)(rounds_cap - rounds) * n * sizeof(nid_ms_trace));
  }
  int best_k = -1;
  double best_v = 0;
  for (int k = 0; k < n; k++) {
    const nid_ms_state &S = state_host[k];
    nid_ms_result &R = results[k];
    std::memcpy(R.pose7, S.pose7, sizeof(R.pose7));
    R.chi2 = S.chi2;
    R.lambda = S.lambda;
    R.n_active = S.n_active;
    R.outer_iterations = S.outer_done;
    R.trials = S.trials_total;
    R.status = S.status;
    if (S.started && S.n_active > 0 && lm::finite(S.chi2)) {  // (the front of lm::rank_chains, found in passing)
      const double v = S.chi2 / (double)S.n_active;
      if (best_k < 0 || v < best_v) { best_k = k; best_v = v; }
    }
  }
  if (best) *best = best_k;
  if (rounds_done) *rounds_done = rounds;
  return NID_OK;
}

}  // extern "C"
