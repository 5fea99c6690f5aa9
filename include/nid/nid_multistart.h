/*
 * nid_multistart.h -- many Levenberg-Marquardt chains at once, stepped on the device (libnid_hip.so).
 *
 * NID has a narrow convergence basin, so a tracker starts from several guesses (the previous pose, a motion
 * prediction, perturbations around them) and keeps the best result.  nid_multistart_lm runs all of them together:
 * ONE evaluation grid per round evaluates every chain's trial pose with its Jacobian, and behind it in the same
 * stream a step kernel (k_lm_step, one thread per chain) runs the accept / reject rule, the damped 6x6 solve, the
 * SE(3) update and the lambda schedule for every chain and writes the next pose records straight into the device
 * array the next grid reads.  The host enqueues rounds and looks at one device word between chunks of them.
 *
 * The per-chain rule is ONE function, lm_step() of csrc/nid_lm_step.h, compiled for the device (k_lm_step) and for
 * the host (nid_lm_step_host): IEEE + - * / sqrt and comparisons only, its own sin / cos, built without contraction,
 * so both compilations give the same bits.  It restates the sequential Levenberg-Marquardt of the host stack
 * (OptimizationAlgorithmLevenberg::solveFused, SparseOptimizer::optimize of host/g2o_min.cpp):
 *   first block of a chain (its start pose): adopt H, b, chi2; lambda = 1e-5 max|H_jj|, ni = 2, nBad = 0; solve
 *     (H + lambda I) x = b; trial = exp(x) * current;
 *   every later block is the trial's evaluation: rho = (chi2_cur - chi2_trial) / (sum x_j (lambda x_j + b_j) + 1e-3),
 *     a failed solve counting as chi2_trial = DBL_MAX; ACCEPT if rho > 0 and the trial chi2 is finite (the trial
 *     becomes the current pose together with ITS H, b, chi2; lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)), ni = 2),
 *     else REJECT (lambda *= ni, ni *= 2).  An outer iteration ends with an accepted trial, after 10 trials, or when
 *     rho is not < 0; it ends the chain if it took 10 trials or rho == 0, else by the nBad rule
 *     ((iniChi - chi2) * 1e3 < iniChi three times running), else after `iterations` outer iterations.
 *   A chain that goes on solves and produces the next trial pose.  A FINISHED chain is frozen: its state, pose and
 *   record no longer change, whatever blocks it is handed -- the result does not depend on how many rounds are
 *   enqueued past its end, or on the chunks the host enqueues them in.
 * What "restates" covers: the rule, branch for branch, and the idea of the host stack's 6x6 solver (LinearSolverDense:
 * the largest remaining |diagonal| next, positive or fail) -- not its elimination order.  Where lambda is below the
 * rounding of H (lambda < 2^-40 max|H_jj|; seen only at <= 5.3e-16 of it, on singular H) the damped matrix is singular
 * to rounding and the two solvers can decide differently on success, or on x; everywhere else they agree on success and
 * on x to 1e-9 relative, and the chains give the shipped LM's trials per outer iteration
 * (tests/cpp/lm_step_flows_check.cpp over the recorded trace tests/golden/lm_flows_trace.json).
 *
 * Out of scope: cell shards over several GPUs (nid_multi.h contexts: use one context that owns all cells), more
 * than NID_MAX_BATCH = 256 chains per call, and compacting finished chains out of the grid (a finished chain's
 * pose is still evaluated every round until the last chain ends; its blocks are ignored).  Chains over the levels of
 * an image pyramid, coarse to fine: include/nid/nid_pyr.h.
 */
#ifndef NID_MULTISTART_H
#define NID_MULTISTART_H

#include <stdint.h>

#include "nid/nid_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nid_ms_state.status / nid_ms_result.status */
#define NID_MS_RUNNING 0          /* not finished (in a result: not within max_rounds) */
#define NID_MS_ITERATIONS 1       /* `iterations` outer iterations done */
#define NID_MS_TRIALS_EXHAUSTED 2 /* an outer iteration took its 10 trials */
#define NID_MS_RHO_NOT_NEGATIVE 3 /* a trial was rejected with rho == 0 */
#define NID_MS_NBAD 4             /* three outer iterations in a row gained less than a thousandth */

/* nid_ms_state.flags / nid_ms_trace.flags: what the last step did */
#define NID_MS_F_FIRST 1         /* adopted the start pose's block */
#define NID_MS_F_ACCEPT 2        /* accepted the trial */
#define NID_MS_F_REJECT 4        /* rejected it */
#define NID_MS_F_OUTER_END 8     /* the outer iteration ended with this trial */
#define NID_MS_F_SOLVE_FAILED 16 /* the solve for the NEXT trial failed (a pivot < 0 or NaN): x kept, the trial counts as DBL_MAX */
#define NID_MS_F_FINISHED 32     /* the chain finished with this step */

/* One chain.  To start one: zero the struct, set pose7 (unit quaternion, w >= 0), iterations and xform_mode
 * (NID_XFORM_*); everything else is the step function's.  Doubles first, then 32-bit integers: one layout for the
 * host, the device and ctypes. */
typedef struct {
  double pose7[7];   /* current pose */
  double chi2;       /* its robust chi2 */
  double H[21];      /* its H, upper triangle row-major (a reduced block's [7..27]) */
  double b[6];
  double lambda, ni;
  double ini_chi2;   /* chi2 at the start of the running outer iteration */
  double x[6];       /* the last solve's solution (kept by a failed solve) */
  double trial7[7];  /* the trial pose under evaluation: exp(x) * pose7 */
  double trial_chi2; /* the last block's chi2 as handed over */
  double rho;        /* the last decision's rho */
  double rec_q[7], rec_M[12]; /* the trial's pose record (what the evaluation kernel reads: q = trial7, M = rows of [R|t]) */
  int32_t iterations, xform_mode;
  int32_t started;   /* 0: the next block is the start pose's */
  int32_t n_active;  /* active cells at the current pose */
  int32_t n_bad, trials, outer_done, trials_total;
  int32_t solve_ok;  /* the solve that produced trial7 succeeded */
  int32_t status;    /* NID_MS_* */
  int32_t flags;     /* NID_MS_F_* of the last step */
  int32_t rec_mode;  /* the record's mode word (= xform_mode) */
} nid_ms_state;

typedef struct {
  double pose7[7];
  double chi2, lambda;
  int32_t n_active;
  int32_t outer_iterations; /* outer iterations done */
  int32_t trials;           /* trial poses evaluated (the start pose's evaluation not counted) */
  int32_t status;           /* NID_MS_* */
} nid_ms_result;

/* one per round and chain: the chain's state behind that round's step (a finished chain repeats its last record) */
typedef struct {
  double trial_chi2, lambda, rho;
  double pose7[7];
  int32_t flags, status;
} nid_ms_trace;

/* The host build of lm_step(): one step of one chain with the 32-double reduced block of the pose it asked for
 * (state->rec_q; the start pose's for a fresh chain).  Returns 1 while the chain is running, 0 once it is finished,
 * NID_ERR_INVALID_ARG for a null pointer. */
int nid_lm_step_host(nid_ms_state *state, const double *reduced32);

/* One launch of k_lm_step (the kernel nid_multistart_lm's rounds run) over n caller-given chains: tests, debugging.
 * states[n] in/out; reduced32: n x 32; rec19 (n x 19: q[7], M[12]) and rec_mode[n] in/out -- uploaded into the records
 * first, so a record the kernel does not write comes back as passed in; trace[n] (may be NULL); *running: the word.
 * Buffers are the call's own (the multi-start pool is not touched); no pair need be set.  NID_ERR_INVALID_ARG for a
 * null pointer (but trace) or unless 1 <= n <= 65536; NID_ERR_STATE while a launch is pending. */
int nid_lm_step_device(nid_ctx *ctx, nid_ms_state *states, const double *reduced32, int n, double *rec19,
                       int32_t *rec_mode, nid_ms_trace *trace, unsigned *running);

/* n_chains Levenberg-Marquardt chains from poses7_in (n_chains x 7) on the context's frame pair, at most
 * `iterations` outer iterations each.  A round is one grid of n_chains poses with the Jacobian in the context's
 * cost + Jacobian shape (a context set to 512 / 1024 threads runs these grids with 256, as every launch of more than
 * 16 poses does), its repair kernel and the step kernel; the records come from a device array for EVERY n_chains,
 * so a chain's bits do not depend on how many chains run beside it.  Buffers are the call's own: the public slots
 * are not touched.  max_rounds = 0 means 1 + 10 * iterations (every chain finishes within that).
 * results[n_chains]; *best (may be NULL) = the chain with the smallest chi2 / n_active among chains with finite chi2
 * and n_active > 0, the lowest index winning ties, -1 if there is none; trace (may be NULL) max_rounds x n_chains
 * records, round-major, rows from *rounds_done on zeroed; *rounds_done (may be NULL) = rounds until the last chain
 * finished (max_rounds if one did not).  Blocking.
 * NID_ERR_INVALID_ARG unless 1 <= n_chains <= NID_MAX_BATCH and iterations >= 1; NID_ERR_STATE while a launch is
 * pending, the pair is not set, or the per-pixel dump / phase stamps are on.  FAST and STRICT math both work. */
int nid_multistart_lm(nid_ctx *ctx, const double *poses7_in, int n_chains, int iterations, double huber_delta,
                      int max_rounds, nid_ms_result *results, int *best, nid_ms_trace *trace, int *rounds_done);

#ifdef __cplusplus
}
#endif
#endif
