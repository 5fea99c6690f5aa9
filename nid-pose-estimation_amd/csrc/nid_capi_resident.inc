// nid_capi_resident.inc -- host side of the resident evaluator (k_resident: single poses through a mailbox): probe,
// one-per-device registry, start / retire / quiesce, posting a request, waiting, the fall-back to launches.  (Round 5's
// resident BATCH evaluator -- a persistent grid for short sequences -- was measured slower than launches at every length,
// profiles/r05_short_sequences.txt, and was removed in round 6.)
// Part of nid_capi.hip's translation unit (included inside its anonymous namespace: it works on nid_ctx's internals).

// ---- the RESIDENT evaluator (k_resident) ----------------------------------------------------------------------------
// Host side: the mailbox lives in fine-grained DEVICE memory that the CPU writes through the PCIe BAR (pose record and
// flags, a store fence, the doorbell word, a store fence); results come back by the DIRECT protocol into res.rec_host
// (and slot 0's cellout_host for the per-cell calls).  One request in flight at a time.  The kernel is started on its
// own stream at the first request, retired (exit word + stream synchronisation: microseconds, every workgroup polls the
// word) by every call that changes what it has cached or frees device memory, and by the next request after
// kResidentHostIdle without one; a kernel that is gone nevertheless (its own idle limit) is noticed by the unanswered
// request, which is then re-issued as an ordinary DIRECT launch (resident_fallback).
// One resident kernel per DEVICE in this process: its workgroups hold most of every CU, a second context's kernel would
// not be scheduled beside it (its requests would time out into fallbacks while the first one sits there).  The registry
// names the context that holds a device; another context's nid_set_resident / request is refused (it keeps launching).
constexpr int kResMaxDevices = 64;
static std::atomic<nid_ctx *> g_res_owner[kResMaxDevices];  // (contexts of one device may live on different threads)
static bool res_claim(nid_ctx *ctx) {
  const int d = ctx->cfg.device;
  if (d < 0 || d >= kResMaxDevices) return true;
  nid_ctx *none = nullptr;
  return g_res_owner[d].compare_exchange_strong(none, ctx) || none == ctx;
}
static void res_release(nid_ctx *ctx) {
  const int d = ctx->cfg.device;
  nid_ctx *me = ctx;
  if (d >= 0 && d < kResMaxDevices) g_res_owner[d].compare_exchange_strong(me, nullptr);
}
static bool res_held_by_other(const nid_ctx *ctx) {
  const int d = ctx->cfg.device;
  if (d < 0 || d >= kResMaxDevices) return false;
  const nid_ctx *o = g_res_owner[d].load();
  return o && o != ctx;
}

int resident_probe(nid_ctx *ctx) {
  nid_ctx::Resident &R = ctx->res;
  if (R.probed) return R.probed > 0 ? NID_OK : NID_ERR_UNSUPPORTED;
  R.probed = -1;
  // Can the CPU store to device memory?  Asked, not tried: the device's large-BAR attribute (a store to memory the CPU
  // cannot reach faults, and a fault probe would have to swap the process's SIGSEGV / SIGBUS handlers under the feet
  // of every other thread).
  int large_bar = 0;
  if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, ctx->cfg.device) != hipSuccess || !large_bar) {
    (void)hipGetLastError();
    R.why = "the device's memory is not CPU-addressable here (no large BAR): resident requests need a mailbox the host can write";
    return NID_ERR_UNSUPPORTED;
  }
  void *p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, 4096, hipDeviceMallocFinegrained);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    R.why = std::string("hipExtMallocWithFlags(hipDeviceMallocFinegrained): ") + hipGetErrorString(e);
    return NID_ERR_UNSUPPORTED;
  }
  auto fail = [&](const char *what, int rc) {  // every failure path gives back what was created
    (void)hipGetLastError();
    (void)hipFree(p);  // (the mailbox: the one raw allocation of the unit)
    R.ctl = nullptr;
    R.stream.reset();
    R.rec_host.reset();
    R.why = what;
    return rc;
  };
  e = hipMemset(p, 0, 4096);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) return fail("clearing the mailbox failed", NID_ERR_UNSUPPORTED);
  R.ctl = static_cast<ResidentCtl *>(p);
  if (R.stream.create() != hipSuccess) return fail("no stream for the resident kernel", NID_ERR_HIP);
  const size_t n = (size_t)2 * ctx->g.nloc * kDirectRec;
  if (R.rec_host.alloc(n, hipHostMallocMapped) != hipSuccess) return fail("no pinned memory for the records", NID_ERR_NOMEM);
  fill_sentinel(R.rec_host, n);
  R.probed = 1;
  return NID_OK;
}

inline void store_fence() { __builtin_ia32_sfence(); }

void resident_retire(nid_ctx *ctx) {
  nid_ctx::Resident &R = ctx->res;
  if (!R.running) return;
  (void)hipSetDevice(ctx->cfg.device);
  volatile unsigned long long *w = R.ctl->w;
  w[7] = kResExitWord;
  store_fence();
  (void)hipStreamSynchronize(R.stream);  // every workgroup polls the word: microseconds
  w[7] = R.seq << 8;                     // (a word no request carries: the next kernel starts from it)
  store_fence();
  R.running = false;
  res_release(ctx);
}

int resident_launch(nid_ctx *ctx, const EvalParams &P, int nt, size_t lds, unsigned grid) {
  nid_ctx::Resident &R = ctx->res;
  // every workgroup must be ON the device for a request to be answered.  A 512-thread workgroup of this kernel is two
  // waves per SIMD with up to 256 registers each and > 100 KB of LDS: exactly one fits a CU, so the grid must not
  // exceed the CU count.  (Not hipOccupancyMaxActiveBlocksPerMultiprocessor: the ROCm 7.0 runtime a torch process
  // carries answers 0 for any kernel with more than 64 KB of dynamic LDS, which the device runs all the same.)
  // The 256-thread form (k_resident<256, NB, 0>: the loop form, one wave per SIMD and workgroup, at most 128 registers,
  // ~15-25 KB of LDS) fits FOUR workgroups per CU: contexts of up to 4 x CUs cells (BASELINE configs[1]: 1024 cells on 256
  // CUs) -- as long as the device is otherwise empty; a workgroup that is not on the device shows as a request that
  // times out (resident_fallback backs off).
  int cus = 0;
  NID_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->cfg.device));
  const long per_cu = nt == 512 ? 1 : std::min<long>(4, (long)((160 * 1024) / std::max<size_t>(lds, 1)));
  if ((long)cus * per_cu < (long)grid) {
    ctx->last_error = "resident evaluator: " + std::to_string(grid) + " workgroups of " + std::to_string(nt) + " threads and " +
                      std::to_string(lds) + " B of LDS on " + std::to_string(cus) + " CUs";
    return NID_ERR_UNSUPPORTED;
  }
  long long idle_ticks = kResidentIdleTicks;
  if (const char *e = getenv("NID_RESIDENT_IDLE_US")) idle_ticks = std::max(1L, atol(e)) * 100;  // tests: a kernel that leaves early
  // the mailbox word the kernel starts from (whatever is there now is not a request)
  volatile unsigned long long *w = R.ctl->w;
  w[7] = R.seq << 8;
  store_fence();
  launch_resident(P, nt, lds, grid, R.stream, (const ResidentCtl *)R.ctl, R.seq << 8, idle_ticks, ctx->xform);
  NID_HIP(ctx, hipGetLastError());
  return NID_OK;
}

int resident_start(nid_ctx *ctx, int nt) {
  nid_ctx::Resident &R = ctx->res;
  int rc = resident_probe(ctx);
  if (rc) { ctx->last_error = "resident evaluator: mailbox probe failed"; return rc; }
  EvalParams P{};
  fill_common_params(ctx, 1.0, &P);  // (the Huber weights of a DIRECT launch are the host's business)
  P.batch = 1;
  set_hist_params(P);
  SlotArgs &A = P.slot[0];
  Slot &S0 = ctx->slots[0];
  A.cellout = S0.cellout_host.dev();
  A.quad = R.rec_host.dev();
  A.gpart = nullptr; A.ticket = nullptr; A.out_reduced = nullptr; A.host_seq = nullptr;
  A.launch_seq = 0; A.cellout_host = 0; A.host_quad = 1;
  // eval_cell's LDS + the cell's tile entries (k_eval2's LAT branch, RES): rounds x threads x (7 doubles + 1 int)
  if (nt != 512 && nt != 256) { ctx->last_error = "resident evaluator: shape " + std::to_string(nt); return NID_ERR_UNSUPPORTED; }
  const size_t lds = eval_lds_bytes(P.g, nt, true) + 16 + (size_t)lat_rounds(nt) * nt * (7 * 8 + 4);  // (256 threads: the loop form, no tile entries in LDS)
  if (lds > 160 * 1024) { ctx->last_error = "resident evaluator: LDS request " + std::to_string(lds); return NID_ERR_UNSUPPORTED; }
  const unsigned grid = (unsigned)(((P.g.nloc + 7) / 8) * 8);
  const int nb = P.g.nb;
  if (!res_claim(ctx)) { ctx->last_error = "resident evaluator: another context's resident kernel holds this device"; return NID_ERR_STATE; }
  rc = resident_launch(ctx, P, nt, lds, grid);
  if (rc) { res_release(ctx); return rc; }
  R.running = true;
  R.nt = nt;
  R.starts++;
  R.last_post = std::chrono::steady_clock::now();
  return NID_OK;
}

// may THIS single-pose launch go to the resident kernel?  (FAST math at the 512-thread latency shape -- two waves per
// SIMD: the resident workgroup may use 256 registers per lane; at 1024 threads it would spill --, its rounds covering a
// cell, and the shape cost + Jacobian launches of this context use anyway: the Jacobian's last bits depend on it)
bool resident_usable(const nid_ctx *ctx) {
  const nid_ctx::Resident &R = ctx->res;
  if (!R.enabled || R.probed < 0 || R.pending_slot >= 0 || !direct_ok(ctx)) return false;
  // another context's resident kernel holds this device: launch (see g_res_owner)
  if (res_held_by_other(ctx)) return false;
  if (ctx->math_mode != NID_MATH_FAST || ctx->loop_form) return false;
  const int nt = ctx->jac_threads;
  if ((nt != 512 && nt != 256) || nt == R.unfit_nt) return false;
  if (ctx->cost_threads != 0 && ctx->cost_threads != nt) return false;  // (cost-only results are the same bits in every shape)
  return nt == 256 ? ctx->g.pstride <= 32 * nt : ctx->g.pstride <= lat_rounds(nt) * nt;  // (256: the loop form's lane masks cover 32 rounds)
}

// hand one request to the resident kernel (starting it if need be); NID_ERR_UNSUPPORTED: use an ordinary launch
int resident_post(nid_ctx *ctx, int slot, const Pose &pose, bool jac, bool want_cellout) {
  nid_ctx::Resident &R = ctx->res;
  // the mailbox carries a pose7 and the kernel forms the matrix from it -- if the pose's matrix IS that matrix;
  // a pose that exists only as a matrix (nid_evaluate_matrix) goes as the matrix, in two lines
  bool as_matrix = false;
  {
    Pose chk;
    pose_from_pose7(pose.q, pose.mode, &chk);
    if (std::memcmp(chk.M, pose.M, sizeof(chk.M)) != 0) {
      if (pose.mode != NID_XFORM_MATRIX) return NID_ERR_STATE;
      as_matrix = true;
    }
  }
  const auto now = std::chrono::steady_clock::now();
  if (R.running && (R.nt != ctx->jac_threads || now - R.last_post > kResidentHostIdle)) resident_retire(ctx);
  if (!R.running) {
    int rc = resident_start(ctx, ctx->jac_threads);
    if (rc) {
      if (getenv("NID_RESIDENT_DEBUG")) fprintf(stderr, "[nid resident] start failed: %d %s\n", rc, ctx->last_error.c_str());
      if (rc == NID_ERR_UNSUPPORTED) { R.unfit_nt = ctx->jac_threads; R.why = ctx->last_error; }  // (this geometry never fits this shape: later nid_set_resident(1) calls say so)
      return rc;
    }
  }
  R.pose = pose; R.jac = jac; R.want_cellout = want_cellout;
  // the mailbox line(s): the payload, a store fence, (number << 8 | flags), a store fence (ResidentCtl)
  volatile unsigned long long *dst = R.ctl->w;
  unsigned long long words[12];
  const unsigned flags = (jac ? kResJac : 0u) | (want_cellout ? kResCellout : kResRecord) | (as_matrix ? kResMatrix : 0u);
  if (as_matrix) {
    std::memcpy(words, pose.M, sizeof(words));
    for (int i = 0; i < 7; i++) dst[i] = words[i];
    for (int i = 0; i < 5; i++) dst[8 + i] = words[7 + i];
  } else {
    std::memcpy(words, pose.q, 7 * sizeof(words[0]));
    for (int i = 0; i < 7; i++) dst[i] = words[i];
  }
  store_fence();
  const unsigned long long word = (++R.seq << 8) | flags;
  if (as_matrix) dst[15] = word;
  dst[7] = word;
  store_fence();  // out of the write-combining buffers now
  R.last_post = std::chrono::steady_clock::now();
  R.pending_slot = slot;
  return NID_OK;
}

// An ordinary evaluation launch is about to be enqueued.  The resident workgroups hold two waves per SIMD with ~200
// registers each on every CU they sit on: a launch whose workgroups do not fit beside them would wait until the
// resident kernel leaves by itself.  So it leaves now -- after the request it may be working on has been collected
// (its slot keeps the result for nid_wait).
int resident_quiesce(nid_ctx *ctx) {
  nid_ctx::Resident &R = ctx->res;
  if (!R.running) return NID_OK;
  if (R.pending_slot >= 0) {
    Slot &S = ctx->slots[R.pending_slot];
    int rc = wait_direct(ctx, S);  // (the per-cell calls are blocking: never pending here)
    if (rc) return rc;
    S.delivery = Delivery::Collected;
  }
  resident_retire(ctx);
  return NID_OK;
}

// the resident kernel did not answer: take it down and put the request through an ordinary DIRECT launch (into the
// slot's own record buffer; the per-cell outputs have one buffer either way)
int resident_fallback(nid_ctx *ctx, Slot &S) {
  nid_ctx::Resident &R = ctx->res;
  resident_retire(ctx);  // (if it was still there: no late writes after this)
  R.fallbacks++;
  // A request that times out costs 2 ms of spinning plus a launch.  One such event after an idle spell is the kernel's
  // own idle limit at work; a run of them -- the workgroups are not co-resident: a shared GPU, another process's kernels
  // -- means the mode does not work here: it is switched off, with the reason on record (nid_last_error,
  // nid_resident_stats), instead of making every evaluation 100x slower than a launch.
  R.fallback_run++;
  if (R.fallback_run >= 3 || (R.fallbacks > 8 && R.fallbacks > R.served)) {
    R.enabled = false;
    R.why = "resident evaluator switched off: " + std::to_string(R.fallbacks) + " requests timed out (" + std::to_string(R.served) +
            " served) -- its workgroups are not staying on the device (a shared GPU?); requests are launched from now on";
    ctx->last_error = R.why;
  }
  fill_sentinel(R.rec_host, (size_t)2 * ctx->g.nloc * kDirectRec);
  if (R.want_cellout) fill_sentinel(ctx->slots[0].cellout_host, (size_t)ctx->g.nloc * kCellOut);
  int rc = ensure_quad_host(ctx, S);
  if (rc) return rc;
  EvalParams P{};
  fill_common_params(ctx, 1.0, &P);
  SlotArgs &A = P.slot[0];
  fill_slot_args(ctx, R.pose, S, nullptr, nullptr, &A);
  A.quad = S.quad_host.dev();
  A.host_quad = R.want_cellout ? 2 : 1;
  S.quad_dirty = !R.want_cellout;
  if (R.want_cellout) { A.cellout = ctx->slots[0].cellout_host.dev(); A.cellout_host = 1; }
  NID_HIP(ctx, hipSetDevice(ctx->cfg.device));
  S.delivery = R.want_cellout ? Delivery::Cellout : Delivery::Direct;  // from here on the wait is an ordinary one
  R.pending_slot = -1;
  return launch_eval2(ctx, P, R.jac, ctx->stream);
}
