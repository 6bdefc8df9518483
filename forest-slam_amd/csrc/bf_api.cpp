// extern "C" entry points of the k-nearest-neighbour matcher and the ratio test (include/fvo.h):
// argument checks, host-only; the launches are bf_knn_run's and bf_ratio_run's (bf.hip).  Kept out
// of capi.cpp so that file's host-only sanitizer build (tools/sanitize.sh) links unchanged.
#include <cmath>
#include <cstdint>

#include "fvo_internal.h"

// The checks the two entry points share; 1 = nothing to do (batch == 0), < 0 = refused.
static int bf_check(fvo_ctx* c, const void* query, const void* n_query, const void* train, const void* n_train,
                    int32_t batch, int32_t cap) {
  if (!c) return -1;
  if (!(c->cfg.stages & FVO_STAGE_BF)) return fvo_fail(c, "stage not enabled in this context (fvo_config.stages)");
  if (batch < 0 || batch > c->cfg.max_batch) return fvo_fail(c, "batch exceeds max_batch");
  if (batch == 0) return 1;
  if (!query || !n_query || !train || !n_train) return fvo_fail(c, "null pointer argument");
  if (cap < 1 || cap > c->kp_cap) return fvo_fail(c, "cap must be in [1, fvo_kp_capacity()]");
  if ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(train)) & 15)
    return fvo_fail(c, "descriptor buffers must be 16-byte aligned");
  return 0;
}

extern "C" {

int fvo_bf_knn_match(fvo_ctx* c, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                     const int32_t* n_train, int32_t batch, int32_t cap, int32_t k, int32_t* knn, fvo_stream stream) {
  const int rc = bf_check(c, query, n_query, train, n_train, batch, cap);
  if (rc) return rc < 0 ? rc : 0;
  if (k < 1 || k > FVO_BF_MAX_K) return fvo_fail(c, "bf_knn_match: k must be in [1, 8]");
  if (!knn) return fvo_fail(c, "null pointer argument");
  return bf_knn_run(c, query, n_query, train, n_train, batch, cap, k, knn, (hipStream_t)stream);
}

int fvo_bf_ratio_match(fvo_ctx* c, const uint8_t* query, const int32_t* n_query, const uint8_t* train,
                       const int32_t* n_train, int32_t batch, int32_t cap, double ratio, int32_t mutual,
                       int32_t* matches, int32_t* n_matches, fvo_stream stream) {
  const int rc = bf_check(c, query, n_query, train, n_train, batch, cap);
  if (rc) return rc < 0 ? rc : 0;
  if (!matches || !n_matches) return fvo_fail(c, "null pointer argument");
  if (!std::isfinite(ratio) || ratio <= 0.0) return fvo_fail(c, "bf_ratio_match: ratio must be finite and > 0");
  return bf_ratio_run(c, query, n_query, train, n_train, batch, cap, ratio, mutual != 0, matches, n_matches,
                      (hipStream_t)stream);
}

}  // extern "C"
