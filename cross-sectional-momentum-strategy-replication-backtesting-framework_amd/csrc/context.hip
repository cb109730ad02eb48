// context.hip -- the C ABI's context and knob plumbing; no kernel.
//
//   csm_create / csm_destroy   the context (csm_common.h csm_ctx): its device, its stream and the
//                              buffers it owns from the start (the decile row flags, the fused
//                              long-short's ticket); the workspaces the stages grow lazily are
//                              freed here.
//   csm_tune / csm_tune_ptr    dispatch only.  Every stage keeps its knobs static in its own source,
//                              behind its own table and csm_tune_<stage>; these try each in turn.
#include <stdlib.h>

#include "csm_common.h"

extern "C" {

int csm_abi_version(void) { return CSM_ABI_VERSION; }

// Process-wide knobs (csm_tune).  Every one selects between PRODUCT paths that give identical
// results (the fallbacks odd widths / unaligned buffers / narrow panels take), so tests can
// drive each path on inputs that would not reach it by default.  The measured variants that
// lost their A/B (profiles/r0*/experiments) are not in the library.
int csm_tune(const char* key, int value) {
  for (auto stage : {csm_tune_scans, csm_tune_signal, csm_tune_signal_tc, csm_tune_deciles,
                     csm_tune_shards, csm_tune_signals, csm_tune_market, csm_tune_groups,
                     csm_tune_dailymkt, csm_tune_liq, csm_tune_range, csm_tune_asym})
    if (stage(key, value) == CSM_OK) return CSM_OK;
  return csm_tune_portfolio(key, value);
}

int csm_tune_ptr(const char* key, void* p) {
  if (csm_tune_ptr_deciles(key, p) == CSM_OK) return CSM_OK;
  return csm_tune_ptr_portfolio(key, p);
}

int csm_create(int device, csm_ctx** out) {
  if (!out) return CSM_E_INVAL;
  *out = nullptr;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return CSM_E_HIP;
  if (hipSetDevice(device) != hipSuccess) return CSM_E_HIP;
  csm_ctx* c = (csm_ctx*)calloc(1, sizeof(csm_ctx));
  if (!c) return CSM_E_INVAL;
  c->device = device;
  c->stream = nullptr;
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
    c->n_cu = 256;
  c->dec_flg_bytes = ((size_t)1 << 16) * sizeof(int32_t);
  if (hipMalloc(&c->dec_flg, c->dec_flg_bytes) != hipSuccess) {
    free(c);
    return CSM_E_HIP;
  }
  // the fused long-short's arrival counter: allocated and zeroed here, so a captured pipeline
  // never allocates; each decile launch's last workgroup leaves it zero again
  if (hipMalloc(&c->ticket, 256) != hipSuccess) {
    (void)hipFree(c->dec_flg);
    free(c);
    return CSM_E_HIP;
  }
  if (hipMemset(c->ticket, 0, 256) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(c->ticket);
    (void)hipFree(c->dec_flg);
    free(c);
    return CSM_E_HIP;
  }
  *out = c;
  return CSM_OK;
}

int csm_destroy(csm_ctx* ctx) {
  if (ctx) (void)csm_allgather_free(ctx);
  if (ctx && (ctx->scratch || ctx->dec_flg || ctx->ticket || ctx->dsplit || ctx->mkt_ws ||
              ctx->xs_ws || ctx->grp_ws)) {
    (void)hipSetDevice(ctx->device);
    if (ctx->grp_ws) (void)hipFree(ctx->grp_ws);
    if (ctx->xs_ws) (void)hipFree(ctx->xs_ws);
    if (ctx->mkt_ws) (void)hipFree(ctx->mkt_ws);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->dec_flg) (void)hipFree(ctx->dec_flg);
    if (ctx->ticket) (void)hipFree(ctx->ticket);
    if (ctx->dsplit) (void)hipFree(ctx->dsplit);
  }
  free(ctx);
  return CSM_OK;
}

const char* csm_last_error(const csm_ctx* ctx) { return ctx ? ctx->err : "null context"; }

int csm_set_stream(csm_ctx* ctx, void* stream) {
  if (!ctx) return CSM_E_INVAL;
  ctx->stream = (hipStream_t)stream;
  return CSM_OK;
}

int csm_sync(csm_ctx* ctx) {
  int r = prep(ctx);
  if (r) return r;
  HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CSM_OK;
}

}  // extern "C"
