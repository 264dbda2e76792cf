// Segment top-k on the host: the packed words and the comparator of
// segment_topk.hip (key << 32 | row within the segment, smaller first), a
// partial sort per (segment, column) item on the thread pool. The order is
// strict, so the bits are the device's whatever it does with chunks.
#include "../../include/dgl_hip.h"
#include "common.h"

#include <cstring>

namespace dglhip {

namespace {

inline uint64_t pack_key(float v, uint32_t pos, bool desc) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  uint32_t key = 0xffffffffu;
  if (v == v) {
    if (b == 0x80000000u) b = 0u;
    key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  if (desc) key = ~key;
  return (uint64_t(key) << 32) | pos;
}

void check_args(int64_t B, int64_t N, int64_t F, int64_t k, int64_t sortby,
                const int64_t* offsets) {
  DGLHIP_CHECK(B >= 0 && N >= 0 && F >= 0, "negative size");
  DGLHIP_CHECK(k >= 1 && k <= DGLHIP_TOPK_CHUNK,
               "k = " << k << " outside [1, DGLHIP_TOPK_CHUNK = " << DGLHIP_TOPK_CHUNK << "]");
  DGLHIP_CHECK(sortby >= -1 && (sortby < F || F == 0), "sortby " << sortby << " is no column");
  DGLHIP_CHECK(N < (int64_t(1) << 32) - 1, "rows within a segment are kept in 32 bits");
  DGLHIP_CHECK(offsets != nullptr, "offsets is null");
  DGLHIP_CHECK(offsets[0] == 0, "offsets must start at 0, got " << offsets[0]);
  for (int64_t s = 0; s < B; ++s)
    DGLHIP_CHECK(offsets[s + 1] >= offsets[s], "offsets decrease at segment " << s);
  DGLHIP_CHECK(offsets[B] == N, "offsets end at " << offsets[B] << ", expected the " << N
                                                  << " rows");
}

// the first min(k, n) words of column c of rows [beg, beg + n), in order
void rank_column(const float* x, int64_t ldx, int64_t beg, int64_t n, int64_t c, int64_t k,
                 bool desc, std::vector<uint64_t>& w) {
  w.resize(n);
  for (int64_t r = 0; r < n; ++r)
    w[r] = pack_key(x[(beg + r) * ldx + c], static_cast<uint32_t>(r), desc);
  const int64_t m = std::min(k, n);
  std::partial_sort(w.begin(), w.begin() + m, w.end());
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_segment_topk_host(int64_t num_segments, int64_t num_rows, int64_t feat_len,
                             int64_t k, int descending, int64_t sortby, const int64_t* offsets,
                             const float* x, int64_t ldx, float* values, int64_t* indices,
                             int num_threads) {
  API_BEGIN();
  check_args(num_segments, num_rows, feat_len, k, sortby, offsets);
  if (num_segments == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(values && indices && (num_rows == 0 || x), "null pointer argument");
  DGLHIP_CHECK(ldx >= feat_len, "row stride below the row width");
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  const int64_t F = feat_len;
  const bool desc = descending != 0, rows = sortby >= 0;
  const int64_t Fe = rows ? 1 : F;
  parallel_for(num_segments * Fe, nt, [&](int64_t i0, int64_t i1, int) {
    std::vector<uint64_t> w;
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t s = i / Fe, f = i - s * Fe;
      const int64_t beg = offsets[s], n = offsets[s + 1] - beg;
      rank_column(x, ldx, beg, n, rows ? sortby : f, k, desc, w);
      for (int64_t j = 0; j < k; ++j) {
        const int64_t idx = j < n ? static_cast<int64_t>(static_cast<uint32_t>(w[j])) : -1;
        if (rows) {
          float* o = values + (s * k + j) * F;
          for (int64_t c = 0; c < F; ++c) o[c] = idx < 0 ? 0.0f : x[(beg + idx) * ldx + c];
          indices[s * k + j] = idx;
        } else {
          values[(s * k + j) * F + f] = idx < 0 ? 0.0f : x[(beg + idx) * ldx + f];
          indices[(s * k + j) * F + f] = idx;
        }
      }
    }
  }, num_rows * feat_len > 32768 ? 2 : num_segments * Fe + 1);
  API_END();
}

int dglhip_segment_topk_bwd_host(int64_t num_segments, int64_t num_rows, int64_t feat_len,
                                 int64_t k, int descending, int64_t sortby,
                                 const int64_t* offsets, const float* dy,
                                 const int64_t* indices, float* dx, int num_threads) {
  API_BEGIN();
  (void)descending;
  check_args(num_segments, num_rows, feat_len, k, sortby, offsets);
  if (num_rows == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(dy && indices && dx, "null pointer argument");
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  const int64_t F = feat_len;
  const bool rows = sortby >= 0;
  parallel_for(num_segments, nt, [&](int64_t b0, int64_t b1, int) {
    for (int64_t s = b0; s < b1; ++s) {
      const int64_t beg = offsets[s], n = offsets[s + 1] - beg;
      if (n == 0) continue;
      std::memset(dx + beg * F, 0, sizeof(float) * n * F);
      for (int64_t j = 0; j < std::min(k, n); ++j) {
        const float* g = dy + (s * k + j) * F;
        if (rows) {
          const int64_t idx = indices[s * k + j];
          if (idx >= 0 && idx < n) std::memcpy(dx + (beg + idx) * F, g, sizeof(float) * F);
        } else {
          for (int64_t f = 0; f < F; ++f) {
            const int64_t idx = indices[(s * k + j) * F + f];
            if (idx >= 0 && idx < n) dx[(beg + idx) * F + f] = g[f];
          }
        }
      }
    }
  }, num_rows * feat_len > 32768 ? 2 : num_segments + 1);
  API_END();
}

}  // extern "C"
