// Edge softmax on the host: the semantics of edge_softmax.hip, one sequential
// pass per row on the thread pool (the rows split over the workers). The last
// bits differ from the device's: another expf, another order of the row sum.
#include "../../include/dgl_hip.h"
#include "common.h"

#include <cmath>
#include <limits>

namespace dglhip {

namespace {

void check_indptr(int64_t R, int64_t nnz, const int64_t* indptr) {
  DGLHIP_CHECK(indptr != nullptr, "indptr is null");
  DGLHIP_CHECK(indptr[0] == 0, "indptr must start at 0, got " << indptr[0]);
  for (int64_t r = 0; r < R; ++r)
    DGLHIP_CHECK(indptr[r + 1] >= indptr[r], "indptr decreases at row " << r);
  DGLHIP_CHECK(indptr[R] == nnz, "indptr ends at " << indptr[R] << ", expected the " << nnz
                                                   << " slots");
}

void check_eid(int64_t nnz, const int64_t* eid) {
  if (!eid) return;
  for (int64_t k = 0; k < nnz; ++k)
    DGLHIP_CHECK(eid[k] >= 0 && eid[k] < nnz, "edge id " << eid[k] << " of slot " << k
                                                         << " out of range");
}

// torch's max: a NaN on either side wins
inline float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_edge_softmax_host(int64_t num_rows, int64_t nnz, int64_t feat_len,
                             const int64_t* indptr, const int64_t* eid, const float* x,
                             float* y, int num_threads) {
  API_BEGIN();
  DGLHIP_CHECK(num_rows >= 0 && nnz >= 0 && feat_len >= 0, "negative size");
  check_indptr(num_rows, nnz, indptr);
  if (num_rows == 0 || nnz == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(x && y, "null pointer argument");
  check_eid(nnz, eid);
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  const int64_t H = feat_len;
  parallel_for(num_rows, nt, [&](int64_t r0, int64_t r1, int) {
    std::vector<float> m(H), s(H);
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t beg = indptr[r], end = indptr[r + 1];
      if (beg == end) continue;
      for (int64_t h = 0; h < H; ++h) {
        m[h] = -std::numeric_limits<float>::infinity();
        s[h] = 0.0f;
      }
      for (int64_t k = beg; k < end; ++k) {
        const float* row = x + (eid ? eid[k] : k) * H;
        for (int64_t h = 0; h < H; ++h) m[h] = nanmax(m[h], row[h]);
      }
      for (int64_t k = beg; k < end; ++k) {
        const int64_t off = (eid ? eid[k] : k) * H;
        for (int64_t h = 0; h < H; ++h) {
          const float e = std::exp(x[off + h] - m[h]);
          y[off + h] = e;
          s[h] = s[h] + e;
        }
      }
      for (int64_t k = beg; k < end; ++k) {
        float* row = y + (eid ? eid[k] : k) * H;
        for (int64_t h = 0; h < H; ++h) row[h] = row[h] / s[h];
      }
    }
  }, nnz * feat_len > 32768 ? 2 : num_rows + 1);
  API_END();
}

int dglhip_edge_softmax_bwd_host(int64_t num_rows, int64_t nnz, int64_t feat_len,
                                 const int64_t* indptr, const int64_t* eid, const float* y,
                                 const float* dy, float* dx, int num_threads) {
  API_BEGIN();
  DGLHIP_CHECK(num_rows >= 0 && nnz >= 0 && feat_len >= 0, "negative size");
  check_indptr(num_rows, nnz, indptr);
  if (num_rows == 0 || nnz == 0 || feat_len == 0) return 0;
  DGLHIP_CHECK(y && dy && dx, "null pointer argument");
  check_eid(nnz, eid);
  const int nt = num_threads > 0 ? num_threads : default_num_threads();
  const int64_t H = feat_len;
  parallel_for(num_rows, nt, [&](int64_t r0, int64_t r1, int) {
    std::vector<float> t(H);
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t beg = indptr[r], end = indptr[r + 1];
      if (beg == end) continue;
      for (int64_t h = 0; h < H; ++h) t[h] = 0.0f;
      for (int64_t k = beg; k < end; ++k) {
        const int64_t off = (eid ? eid[k] : k) * H;
        for (int64_t h = 0; h < H; ++h) t[h] = t[h] + y[off + h] * dy[off + h];
      }
      for (int64_t k = beg; k < end; ++k) {
        const int64_t off = (eid ? eid[k] : k) * H;
        for (int64_t h = 0; h < H; ++h) dx[off + h] = y[off + h] * (dy[off + h] - t[h]);
      }
    }
  }, nnz * feat_len > 32768 ? 2 : num_rows + 1);
  API_END();
}

}  // extern "C"
