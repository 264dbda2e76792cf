// GATv2 attention on the host: the semantics of gatv2_attention.hip, one
// sequential pass per row in slot order on the thread pool (the rows split
// over the workers), the forward and both walks of the backward. Any head
// width. The last bits differ from the device's: another expf, one maximum
// per row instead of one per batch, another order of the score's sum.
#include "../../include/dgl_hip.h"
#include "attention_host.h"

#include <cmath>

namespace dglhip {

namespace {

constexpr int64_t kRange = 256;  // rows whose dattn partials one pass adds up

inline float lrelu(float z, float slope) { return z > 0.0f ? z : slope * z; }

// s = sum_d attn[d] lrelu(fs[d] + fd[d]) of one head
inline float score(const float* fs, const float* fd, const float* attn, float slope, int64_t D) {
  float t = 0.0f;
  for (int64_t d = 0; d < D; ++d) t += attn[d] * lrelu(fs[d] + fd[d], slope);
  return t;
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_gatv2_attention_host(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                const int32_t* indices, const float* fs, const float* fd,
                                const float* attn, float negative_slope, float* out, float* lse,
                                int num_threads) {
  API_BEGIN();
  const int64_t H = num_heads, D = head_dim, F = H * D;
  const float slope = negative_slope;
  DGLHIP_CHECK(num_rows >= 0 && num_cols >= 0 && nnz >= 0 && H >= 0 && D >= 0, "negative size");
  check_csr(num_rows, num_cols, nnz, indptr, indices);
  if (num_rows == 0 || F == 0) return 0;
  DGLHIP_CHECK(fd && attn && out && lse && (nnz == 0 || fs), "null pointer argument");
  parallel_for(num_rows, threads_of(num_threads), [&](int64_t r0, int64_t r1, int) {
    softmax_aggregate_rows(r0, r1, H, D, indptr, indices, fs, out, lse,
                           [&](int64_t r, int64_t h, int64_t j) {
      return score(fs + indices[j] * F + h * D, fd + r * F + h * D, attn + h * D, slope, D);
    });
  }, nnz * F > 32768 ? 2 : num_rows + 1);
  API_END();
}

int dglhip_gatv2_attention_bwd_host(int64_t num_rows, int64_t num_cols, int64_t nnz,
                                    int64_t num_heads, int64_t head_dim, const int64_t* indptr,
                                    const int32_t* indices, const int64_t* t_indptr,
                                    const int32_t* t_indices, const float* fs, const float* fd,
                                    const float* attn, const float* out, const float* lse,
                                    const float* dout, float negative_slope, float* delta,
                                    float* dfs, float* dfd, float* dattn, int num_threads) {
  API_BEGIN();
  const int64_t H = num_heads, D = head_dim, F = H * D;
  const float slope = negative_slope;
  DGLHIP_CHECK(num_rows >= 0 && num_cols >= 0 && nnz >= 0 && H >= 0 && D >= 0, "negative size");
  check_csr(num_rows, num_cols, nnz, indptr, indices);
  check_csr(num_cols, num_rows, nnz, t_indptr, t_indices);
  if (F == 0) return 0;
  DGLHIP_CHECK(attn && dattn && (num_rows == 0 || (fd && out && lse && dout && delta && dfd)) &&
                   (num_cols == 0 || (fs && dfs)),
               "null pointer argument");
  const int nt = threads_of(num_threads);
  const int64_t big = nnz * F > 32768;
  // delta, dfd and dattn: the forward CSR, a destination per pass; dattn per
  // range of kRange rows (the ranges do not depend on the thread count)
  const int64_t ranges = (num_rows + kRange - 1) / kRange;
  std::vector<float> part(static_cast<size_t>(ranges * F), 0.0f);
  parallel_for(ranges, nt, [&](int64_t g0, int64_t g1, int) {
    std::vector<float> gs(D);
    for (int64_t r = g0 * kRange; r < std::min(num_rows, g1 * kRange); ++r) {
      float* da = part.data() + (r / kRange) * F;
      for (int64_t h = 0; h < H; ++h) {
        const int64_t at = r * F + h * D;
        const float* av = attn + h * D;
        const float de = dot(dout + at, out + at, D);
        delta[r * H + h] = de;
        for (int64_t d = 0; d < D; ++d) gs[d] = 0.0f;
        for (int64_t j = indptr[r]; j < indptr[r + 1]; ++j) {
          const float* fu = fs + indices[j] * F + h * D;
          const float e = std::exp(score(fu, fd + at, av, slope, D) - lse[r * H + h]);
          const float ds = e * (dot(dout + at, fu, D) - de);
          for (int64_t d = 0; d < D; ++d) {
            const float z = fu[d] + fd[at + d];
            gs[d] += ds * (z > 0.0f ? 1.0f : slope);
            da[h * D + d] += ds * lrelu(z, slope);
          }
        }
        for (int64_t d = 0; d < D; ++d) dfd[at + d] = av[d] * gs[d];
      }
    }
  }, big ? 2 : ranges + 1);
  for (int64_t f = 0; f < F; ++f) {
    float t = 0.0f;
    for (int64_t g = 0; g < ranges; ++g) t += part[g * F + f];
    dattn[f] = t;
  }
  // dfs: the transposed CSR, a source per pass (delta is complete: the pool
  // has joined)
  parallel_for(num_cols, nt, [&](int64_t u0, int64_t u1, int) {
    std::vector<float> sc(D);
    for (int64_t u = u0; u < u1; ++u) {
      for (int64_t h = 0; h < H; ++h) {
        const int64_t at = u * F + h * D;
        const float* av = attn + h * D;
        float* g = dfs + at;
        for (int64_t d = 0; d < D; ++d) g[d] = sc[d] = 0.0f;
        for (int64_t j = t_indptr[u]; j < t_indptr[u + 1]; ++j) {
          const int64_t r = t_indices[j], ar = r * F + h * D;
          const float e = std::exp(score(fs + at, fd + ar, av, slope, D) - lse[r * H + h]);
          const float ds = e * (dot(dout + ar, fs + at, D) - delta[r * H + h]);
          for (int64_t d = 0; d < D; ++d) {
            g[d] += e * dout[ar + d];
            sc[d] += ds * (fs[at + d] + fd[ar + d] > 0.0f ? 1.0f : slope);
          }
        }
        for (int64_t d = 0; d < D; ++d) g[d] += av[d] * sc[d];
      }
    }
  }, big ? 2 : num_cols + 1);
  API_END();
}

}  // extern "C"
