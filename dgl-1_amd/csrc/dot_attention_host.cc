// Scaled dot-product graph attention on the host: the semantics of
// dot_attention.hip, one sequential pass per row on the thread pool (the rows
// split over the workers), the forward and both halves of the backward. Any
// head width. The last bits differ from the device's: another expf, one
// maximum per row instead of one per batch, another order of the dot
// products.
#include "../../include/dgl_hip.h"
#include "attention_host.h"

#include <cmath>

namespace dglhip {

namespace {

inline float clamp_score(float s, float lo, float hi) { return s < lo ? lo : (s > hi ? hi : s); }

struct Score {
  float scale, lo, hi;
  // the clamped score's exponential against lse, and its gradient's factor:
  // 0 strictly outside [lo, hi], as torch.clamp's backward
  float grad(float raw, float lse, float dp, float delta, float& e) const {
    e = std::exp(clamp_score(raw, lo, hi) - lse);
    return (raw < lo || raw > hi) ? 0.0f : e * (dp - delta) * scale;
  }
};

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_dot_attention_host(int64_t num_rows, int64_t num_cols, int64_t nnz, int64_t num_heads,
                              int64_t head_dim, const int64_t* indptr, const int32_t* indices,
                              const float* q, const float* k, const float* v, float scale,
                              float lo, float hi, float* out, float* lse, int num_threads) {
  API_BEGIN();
  const int64_t H = num_heads, D = head_dim, F = H * D;
  DGLHIP_CHECK(num_rows >= 0 && num_cols >= 0 && nnz >= 0 && H >= 0 && D >= 0, "negative size");
  check_csr(num_rows, num_cols, nnz, indptr, indices);
  if (num_rows == 0 || F == 0) return 0;
  DGLHIP_CHECK(q && out && lse && (nnz == 0 || (k && v)), "null pointer argument");
  parallel_for(num_rows, threads_of(num_threads), [&](int64_t r0, int64_t r1, int) {
    softmax_aggregate_rows(r0, r1, H, D, indptr, indices, v, out, lse,
                           [&](int64_t r, int64_t h, int64_t j) {
      return clamp_score(dot(q + r * F + h * D, k + indices[j] * F + h * D, D) * scale, lo, hi);
    });
  }, nnz * F > 32768 ? 2 : num_rows + 1);
  API_END();
}

int dglhip_dot_attention_bwd_host(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                  int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                  const int32_t* indices, const int64_t* t_indptr,
                                  const int32_t* t_indices, const float* q, const float* k,
                                  const float* v, const float* out, const float* lse,
                                  const float* dout, float scale, float lo, float hi,
                                  float* delta, float* dq, float* dk, float* dv,
                                  int num_threads) {
  API_BEGIN();
  const int64_t H = num_heads, D = head_dim, F = H * D;
  DGLHIP_CHECK(num_rows >= 0 && num_cols >= 0 && nnz >= 0 && H >= 0 && D >= 0, "negative size");
  check_csr(num_rows, num_cols, nnz, indptr, indices);
  check_csr(num_cols, num_rows, nnz, t_indptr, t_indices);
  if (F == 0 || (num_rows == 0 && num_cols == 0)) return 0;
  DGLHIP_CHECK(q && k && v && out && lse && dout && delta && dq && dk && dv,
               "null pointer argument");
  const Score sc = {scale, lo, hi};
  const int nt = threads_of(num_threads);
  const int64_t min_n = nnz * F > 32768 ? 2 : num_rows + num_cols + 1;
  // delta and dq: the forward CSR, a destination per pass
  parallel_for(num_rows, nt, [&](int64_t r0, int64_t r1, int) {
    for (int64_t r = r0; r < r1; ++r) {
      for (int64_t h = 0; h < H; ++h) {
        const int64_t at = r * F + h * D;
        const float de = dot(dout + at, out + at, D);
        delta[r * H + h] = de;
        float* g = dq + at;
        for (int64_t d = 0; d < D; ++d) g[d] = 0.0f;
        for (int64_t j = indptr[r]; j < indptr[r + 1]; ++j) {
          const float* ku = k + indices[j] * F + h * D;
          float e;
          const float t = sc.grad(dot(q + at, ku, D) * scale, lse[r * H + h],
                                  dot(dout + at, v + indices[j] * F + h * D, D), de, e);
          for (int64_t d = 0; d < D; ++d) g[d] += t * ku[d];
        }
      }
    }
  }, min_n);
  // dk and dv: the transposed CSR, a source per pass (delta is complete: the
  // pool has joined)
  parallel_for(num_cols, nt, [&](int64_t u0, int64_t u1, int) {
    for (int64_t u = u0; u < u1; ++u) {
      for (int64_t h = 0; h < H; ++h) {
        const int64_t at = u * F + h * D;
        float* gk = dk + at;
        float* gv = dv + at;
        for (int64_t d = 0; d < D; ++d) gk[d] = gv[d] = 0.0f;
        for (int64_t j = t_indptr[u]; j < t_indptr[u + 1]; ++j) {
          const int64_t r = t_indices[j], ar = r * F + h * D;
          float e;
          const float t = sc.grad(dot(q + ar, k + at, D) * scale, lse[r * H + h],
                                  dot(dout + ar, v + at, D), delta[r * H + h], e);
          for (int64_t d = 0; d < D; ++d) {
            gv[d] += e * dout[ar + d];
            gk[d] += t * q[ar + d];
          }
        }
      }
    }
  }, min_n);
  API_END();
}

}  // extern "C"
