// The context behind the C ABI of libbot7hip.so (include/bot7hip.h): errors, device and pinned buffers, phase timing, creation and
// destruction.  There is no CPU fallback: without a working HIP device b7_create fails and nothing else runs.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "b7_internal.h"

static thread_local std::string g_create_err;

int b7_fail(b7_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c)
    c->err = buf;
  else
    g_create_err = buf;
  return code;
}

int b7_ensure(b7_ctx *c, DevBuf &b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.cap >= bytes) return B7_OK;
  if (b.p) {
    // keep stream order: nothing in flight may still use the old block
    B7_HIP(c, hipStreamSynchronize(c->stream));
    B7_HIP(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    return b7_fail(c, B7_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
  }
  b.cap = bytes;
  return B7_OK;
}

void b7_release(DevBuf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

int b7_pin_ensure(b7_ctx *c, PinBuf &b, size_t bytes, bool mapped) {
  if (b.bytes >= bytes) return B7_OK;
  B7_HIP(c, hipStreamSynchronize(c->stream));  // nothing in flight reads or writes the block about to go
  if (b.host) (void)hipHostFree(b.host);
  b = PinBuf();
  B7_HIP(c, hipHostMalloc(&b.host, 2 * bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault));
  if (mapped) B7_HIP(c, hipHostGetDevicePointer(&b.dev, b.host, 0));
  b.bytes = 2 * bytes;
  return B7_OK;
}

static hipEvent_t phase_event(b7_ctx *c) {
  if (!c->free_events.empty()) {
    hipEvent_t e = c->free_events.back();
    c->free_events.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// Turn the recorded event pairs into phase times (one stream synchronisation) and recycle the events.
static void resolve_phases(b7_ctx *c) {
  if (c->pending.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  for (const b7_ctx::PendingPhase &p : c->pending) {
    float ms = 0.f;
    if (p.e0 && p.e1 && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
      PhaseStat &s = c->phases[p.name];
      s.ms += ms;
      s.launches += 1;
    }
    if (p.e0) c->free_events.push_back(p.e0);
    if (p.e1) c->free_events.push_back(p.e1);
  }
  c->pending.clear();
}

// Phases do not nest.  Recording costs two hipEventRecord calls and no synchronisation: a profiled step keeps the
// host running ahead of the GPU exactly like an unprofiled one.
PhaseScope::PhaseScope(b7_ctx *c_, const char *name_) : c(c_), name(name_) {
  if (!c->profile) return;
  c->phase_e0 = phase_event(c);
  if (c->phase_e0) (void)hipEventRecord(c->phase_e0, c->stream);
}
PhaseScope::~PhaseScope() {
  if (!c->profile || !c->phase_e0) return;
  hipEvent_t e1 = phase_event(c);
  if (e1) (void)hipEventRecord(e1, c->stream);
  c->pending.push_back({name, c->phase_e0, e1});
  c->phase_e0 = nullptr;
  if (c->pending.size() >= 4096) resolve_phases(c);  // bound the pool in long profiled loops
}

int npad_of(const b7_ctx *c, int64_t n) { return (c->npad_small && n <= 64) ? 64 : (int)round_up(n, B7_NPAD); }

// The streams of the contexts o[0 .. n - 1] of one call, n <= 1 + B7_TS_FEAS_CMAX, ordered by events both ways around the work that
// o[0]'s stream does on the others' buffers.  before: o[0]'s stream waits for what every other stream has been given (event m - 1 for
// o[m]: a nomination may return before its stream is formally idle); after: whatever the other contexts enqueue next waits for that
// work (the last event).  A context that appears twice is waited on once.  The events are o[0]'s, made when first needed.
int streams_order(b7_ctx *const *o, int n, bool before) {
  b7_ctx *c = o[0];
  bool recorded = false;
  for (int m = 1; m < n; ++m) {
    bool seen = false;
    for (int i = 0; i < m; ++i) seen = seen || o[m] == o[i];
    if (seen) continue;
    hipEvent_t &e = c->ev_order[before ? m - 1 : B7_TS_FEAS_CMAX];
    if (!e) B7_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (before || !recorded) B7_HIP(c, hipEventRecord(e, before ? o[m]->stream : c->stream));
    recorded = true;
    B7_HIP(c, hipStreamWaitEvent(before ? c->stream : o[m]->stream, e, 0));
  }
  return B7_OK;
}

static int timers_init(b7_ctx *c) {
  if (c->tev_init) return B7_OK;
  for (int i = 0; i < B7_MAX_TIMERS; ++i) {
    B7_HIP(c, hipEventCreate(&c->tev[i][0]));
    B7_HIP(c, hipEventCreate(&c->tev[i][1]));
  }
  c->tev_init = true;
  return B7_OK;
}

extern "C" {

int b7_abi_version(void) { return B7_ABI_VERSION; }

int b7_create(b7_ctx **out, int device_id) {
  if (!out) return b7_fail(nullptr, B7_ERR_INVALID, "b7_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return b7_fail(nullptr, B7_ERR_HIP, "no HIP device available (%s); libbot7hip has no CPU path",
                   e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev)
    return b7_fail(nullptr, B7_ERR_INVALID, "device_id %d out of range [0,%d)", device_id, ndev);
  e = hipSetDevice(device_id);
  if (e != hipSuccess) return b7_fail(nullptr, B7_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device_id);
  if (e != hipSuccess) return b7_fail(nullptr, B7_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return b7_fail(nullptr, B7_ERR_UNSUPPORTED, "device %d is %s; libbot7hip is built for gfx950 only", device_id,
                   prop.gcnArchName);
  b7_ctx *c = new b7_ctx();
  c->device = device_id;
  c->cus = prop.multiProcessorCount;
  b7_gp_default_opts(&c->opts);
  // the one tunable of the shipped library, read once here, never in the launch paths
  if (const char *pv = getenv("B7_SPIN_US")) c->spin_us = atoi(pv);  // 0: never spin on a completion word, always wait for the stream
#ifdef B7_DIAG
  // DIAGNOSTIC build only (tools/_build/libbot7hip_diag.so, python -m bot7_amd.build --diag; tests load it beside the shipped
  // library): the A/B arms that tests/test_gpu_parity.py holds against the default paths, stamp collection, the persistent
  // schedule's fault injector.  None of these names exists in libbot7hip.so.
  if (const char *pv = getenv("B7_DIAG_VARIANT")) c->diag_variant = atoi(pv);  // 0 rsqrt chain, 1 DPP-fused (default), 2 its mov+fma reference
  if (const char *pv = getenv("B7_NPAD_SMALL")) c->npad_small = atoi(pv) != 0;  // 0: pad N <= 64 (and <= 64 basis features) to 128 as N > 64
  if (const char *pv = getenv("B7_POTRF_SMALL")) c->potrf_small = atoi(pv) != 0;
  if (getenv("B7_POTRF_SCHED") || getenv("B7_DIAG_VARIANT") || getenv("B7_INVERSE_INLINE")) c->potrf_small = c->fit_small = false;  // an explicit schedule is an A/B arm of the general path
  if (const char *pv = getenv("B7_BLR_SMALL")) c->blr_small = atoi(pv) != 0;  // 0: the head of b7_blr_eval_nominate through the general launches
  if (const char *pv = getenv("B7_INVERSE_INLINE")) c->inverse_inline = atoi(pv);  // 0 never, 1 up to N = 8192, 2 always
  if (const char *pv = getenv("B7_POTRF_SCHED")) c->potrf_sched = atoi(pv);  // 0 pairs, 1 one panel at a time up to N = 4096, 2 always
  c->persist_stamps = getenv("B7_PERSIST_STAMPS") != nullptr;
  if (const char *pv = getenv("B7_PERSIST_HELPERS")) c->persist_helpers = atoi(pv);
  if (const char *pv = getenv("B7_PERSIST_FAULT")) c->persist_fault = atoi(pv);
  if (const char *pv = getenv("B7_NLL_SMALL")) c->nll_small = atoi(pv);  // 0: likelihoods of small sets through the general path too; 2: round 3's kernel
  if (const char *pv = getenv("B7_FIT_SMALL")) c->fit_small = atoi(pv) != 0;  // 0: small fits through the general schedule too
  if (const char *pv = getenv("B7_KPOST_SMALL")) c->kpost_small = atoi(pv) != 0;  // 0: small posteriors through ksx_kernel + post_kernel too
  if (const char *pv = getenv("B7_SYRK_SMALL")) c->syrk_small = atoi(pv) ? 1 : 0;
  if (const char *pv = getenv("B7_POTRF_DEFER")) c->potrf_defer = atoi(pv) ? 1 : 0;
  if (const char *pv = getenv("B7_POTRF_GROUP")) {
    const int g = atoi(pv);
    if (g >= 1 && g <= 8) c->potrf_group = g;
  }
  if (const char *pv = getenv("B7_TS_HVI_LAYOUT")) c->ts_hvi_layout = atoi(pv) ? 1 : 0;  // 0: a pick reads column j of [M][q] at stride q; 1: the [q][M] copy (default)
  if (const char *pv = getenv("B7_TS_FEAS_ONEPASS")) c->ts_feas_onepass = atoi(pv) ? 1 : 0;  // 0: the constrained Thompson pick path by path, q chained passes (default); 1: one pass for all q paths, taken rows resolved on the host
#endif
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fit, hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc((void **)&c->pinned, B7_PINNED_BYTES, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&c->pinned_dev, c->pinned, 0);
  if (e != hipSuccess) {
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return b7_fail(nullptr, B7_ERR_HIP, "stream / pinned result block creation: %s", hipGetErrorString(e));
  }
  if (b7_ensure(c, c->scratch, B7_SCRATCH_BYTES) != B7_OK) {  // the fixed ScratchBlock, never regrown
    g_create_err = c->err;
    b7_destroy(c);
    return B7_ERR_NOMEM;
  }
  *out = c;
  return B7_OK;
}

void b7_destroy(b7_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)b7_comm_destroy(c);
  DevBuf *all[] = {&c->grid[0], &c->grid[1], &c->xobs, &c->w,     &c->zsc,  &c->zss,     &c->K,      &c->L,
                   &c->Linv,    &c->W,       &c->dinv, &c->alpha, &c->resid, &c->info,   &c->ybuf,   &c->mu,
                   &c->var,     &c->acc,     &c->ks,   &c->part,  &c->scratch, &c->tmpgrid, &c->tmpmu, &c->tmpvar, &c->fant, &c->feat, &c->netbuf, &c->atmp, &c->slots, &c->pstamps,
                   &c->bhyp, &c->bw, &c->bzsc, &c->bzss, &c->bK, &c->bL, &c->bdinv, &c->bflags, &c->binfo, &c->bresid, &c->bterms,
                   &c->bLinv, &c->balpha, &c->bmu, &c->bvar, &c->ticket, &c->bel, &c->belvec, &c->ystar, &c->mes_ticket, &c->mes_user,
                   &c->ts_paths, &c->ts_draw, &c->ts_work, &c->ts_user, &c->ts_ref_ws, &c->ts_ref_trace, &c->ts_ref_user, &c->slice_trace, &c->slice_state, &c->refine_ws, &c->refine_trace, &c->refine_user,
                   &c->feas, &c->feas_stage, &c->kg, &c->kgvec, &c->kg_slopes, &c->kg_user,
                   &c->ts_hvi, &c->ts_hvi_t, &c->ts_hvi_user, &c->ts_feas, &c->ts_feas_user, &c->post, &c->ehvi_front, &c->ehvi_user, &c->ehvi3_front, &c->ehvi3_table, &c->ehvi3_user, &c->clf, &c->clf_mode, &c->clf_user};
  for (auto &kv : c->pjobs_cache) b7_release(kv.second.buf);
  for (DevBuf *b : all) b7_release(*b);
  if (c->tev_init)
    for (int i = 0; i < B7_MAX_TIMERS; ++i) {
      (void)hipEventDestroy(c->tev[i][0]);
      (void)hipEventDestroy(c->tev[i][1]);
    }
  resolve_phases(c);
  if (c->pinned) (void)hipHostFree(c->pinned);
  for (PinBuf *b : {&c->pin_eval, &c->pin_blr, &c->pin_nll, &c->pin_bel, &c->pin_slice, &c->pin_kg})
    if (b->host) (void)hipHostFree(b->host);
  if (c->tab_host) (void)hipHostFree(c->tab_host);
  for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
  if (c->phase_e0) (void)hipEventDestroy(c->phase_e0);
  if (c->ev_fit) (void)hipEventDestroy(c->ev_fit);
  for (hipEvent_t e : c->ev_order)
    if (e) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

const char *b7_last_error(const b7_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int b7_device_info(b7_ctx *c, char *name_out, int *compute_units, int64_t *hbm_bytes) {
  if (!c) return B7_ERR_INVALID;
  hipDeviceProp_t prop;
  B7_HIP(c, hipGetDeviceProperties(&prop, c->device));
  if (name_out) snprintf(name_out, 64, "%s (%s)", prop.name, prop.gcnArchName);
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  return B7_OK;
}

int b7_sync(b7_ctx *c) {
  if (!c) return B7_ERR_INVALID;
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_set_workspace(b7_ctx *c, int64_t bytes) {
  if (!c || bytes < (int64_t)(8 * 128 * 128)) return c ? b7_fail(c, B7_ERR_INVALID, "workspace too small") : B7_ERR_INVALID;
  c->ks_bytes = (size_t)bytes;
  return B7_OK;
}

// ---- measurement ---------------------------------------------------------------------------------------
int b7_timer_start(b7_ctx *c, int slot) {
  if (!c || slot < 0 || slot >= B7_MAX_TIMERS) return B7_ERR_INVALID;
  B7_TRY(timers_init(c));
  B7_HIP(c, hipEventRecord(c->tev[slot][0], c->stream));
  return B7_OK;
}

int b7_timer_stop(b7_ctx *c, int slot) {
  if (!c || slot < 0 || slot >= B7_MAX_TIMERS) return B7_ERR_INVALID;
  B7_TRY(timers_init(c));
  B7_HIP(c, hipEventRecord(c->tev[slot][1], c->stream));
  return B7_OK;
}

int b7_timer_ms(b7_ctx *c, int slot, float *ms_out) {
  if (!c || slot < 0 || slot >= B7_MAX_TIMERS || !ms_out) return B7_ERR_INVALID;
  B7_TRY(timers_init(c));
  B7_HIP(c, hipEventSynchronize(c->tev[slot][1]));
  B7_HIP(c, hipEventElapsedTime(ms_out, c->tev[slot][0], c->tev[slot][1]));
  return B7_OK;
}

int b7_profile_enable(b7_ctx *c, int on) {
  if (!c) return B7_ERR_INVALID;
  c->profile = on != 0;
  return B7_OK;
}

int b7_profile_reset(b7_ctx *c) {
  if (!c) return B7_ERR_INVALID;
  resolve_phases(c);
  c->phases.clear();
  return B7_OK;
}

int b7_profile_get(b7_ctx *c, const char *phase, double *ms_total, int64_t *launches) {
  if (!c || !phase) return B7_ERR_INVALID;
  resolve_phases(c);
  auto it = c->phases.find(phase);
  if (ms_total) *ms_total = it == c->phases.end() ? 0.0 : it->second.ms;
  if (launches) *launches = it == c->phases.end() ? 0 : it->second.launches;
  return B7_OK;
}

}  // extern "C"
