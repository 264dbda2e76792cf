/* The weighted host sampler (csrc/neighbor_sample_host.cc, csrc/sample_key.h)
 * under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program,
 * linked with the sanitized host library (make -C dgl-1_amd/csrc asan), that
 * drives dglhip_neighbor_sample_host_weighted and
 * dglhip_neighbor_sample_host_fetch on random multigraphs (rows shorter and
 * longer than the fan-out, a long row, self loops, neighbour ids outside the
 * graph, weights of every kind), the two key exports, and the error paths
 * (null weights, negative sizes, a seed outside the graph, a fetch of the wrong
 * size). Built and run by tests/test_weighted_sampler_sanitize.py; any invalid
 * access, leak or UB aborts with a report. The results are checked for the
 * properties every answer has: vertices ascending and distinct, seeds at
 * layer 0, as many edges as the expanded rows' min(degree, fan-out) sum to,
 * every edge one of its row's slots, a weightless slot taken only when its row
 * has fewer weighted slots than the fan-out. Host only: no GPU needed. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dgl_hip.h"

#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);        \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      exit(1);                                                   \
    }                                                            \
  } while (0)
#define OK(call) CHECK((call) == 0, "%s -> %s", #call, DGLGetLastError())
#define REFUSED(call) \
  CHECK((call) != 0 && strlen(DGLGetLastError()) > 0, "%s was not refused", #call)

static uint64_t g_state = 88172645463325252ull;
static uint64_t rnd(void) {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return g_state;
}

static void* xmalloc(size_t n) {
  void* p = malloc(n ? n : 1);
  CHECK(p != NULL, "out of memory");
  return p;
}

static int has_weight(float w) { return isfinite(w) && w >= 1.17549435e-38f; }

static float some_weight(void) {
  switch (rnd() % 12) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return 1e-40f; /* a denormal */
    case 3: return -1.0f;
    case 4: return INFINITY;
    case 5: return NAN;
    case 6: return 1.17549435e-38f;
    case 7: return 3.40282347e+38f;
    default: return (float)(1 + rnd() % 1000) / 37.0f;
  }
}

static void run_case(int64_t n, int64_t long_row, int64_t fanout, int num_hops, int in_dir,
                     int64_t num_seeds) {
  int64_t* indptr = xmalloc(sizeof(int64_t) * (size_t)(n + 1));
  indptr[0] = 0;
  for (int64_t v = 0; v < n; ++v) {
    int64_t d = (int64_t)(rnd() % 12); /* around the fan-outs used */
    if (v == 1) d = long_row;
    if (v % 9 == 0) d = 0;
    indptr[v + 1] = indptr[v] + d;
  }
  const int64_t nnz = indptr[n];
  int32_t* indices = xmalloc(sizeof(int32_t) * (size_t)nnz);
  int64_t* eid = xmalloc(sizeof(int64_t) * (size_t)nnz);
  float* weight = xmalloc(sizeof(float) * (size_t)n);
  for (int64_t v = 0; v < n; ++v) weight[v] = some_weight();
  for (int64_t v = 0; v < n; ++v)
    for (int64_t j = indptr[v]; j < indptr[v + 1]; ++j) {
      indices[j] = (int32_t)(rnd() % (uint64_t)n);
      if (j % 13 == 0) indices[j] = (int32_t)v;                  /* self loops */
      if (j % 17 == 0 && j > indptr[v]) indices[j] = indices[j - 1]; /* parallel edges */
      if (j % 41 == 0) indices[j] = (j % 2) ? -1 : (int32_t)n;    /* outside the graph */
      eid[j] = nnz - 1 - j;
    }
  int64_t* seeds = xmalloc(sizeof(int64_t) * (size_t)num_seeds);
  for (int64_t i = 0; i < num_seeds; ++i) seeds[i] = (int64_t)(rnd() % (uint64_t)n);
  if (num_seeds > 1) seeds[0] = 1;                          /* the long row */
  if (num_seeds > 2) seeds[num_seeds - 1] = seeds[1];       /* a repeated seed */

  int64_t sizes[2] = {-1, -1};
  OK(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, nnz ? indices : NULL,
                                          nnz ? eid : NULL, weight, in_dir,
                                          num_seeds ? seeds : NULL, num_seeds, num_hops, fanout,
                                          7 + (uint64_t)fanout, sizes));
  const int64_t nv = sizes[0], m = sizes[1];
  CHECK(nv >= 0 && nv <= n && m >= 0 && m <= nnz, "sizes %lld %lld", (long long)nv, (long long)m);
  /* a fetch of another size is refused and drops the sample: sample again */
  int64_t dummy[4];
  REFUSED(dglhip_neighbor_sample_host_fetch(nv + 1, m, dummy, dummy, dummy, dummy, dummy));
  OK(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, nnz ? indices : NULL,
                                          nnz ? eid : NULL, weight, in_dir,
                                          num_seeds ? seeds : NULL, num_seeds, num_hops, fanout,
                                          7 + (uint64_t)fanout, sizes));
  CHECK(sizes[0] == nv && sizes[1] == m, "the same call gave another sample");
  int64_t* vertices = xmalloc(sizeof(int64_t) * (size_t)nv);
  int64_t* layers = xmalloc(sizeof(int64_t) * (size_t)nv);
  int64_t* src = xmalloc(sizeof(int64_t) * (size_t)m);
  int64_t* dst = xmalloc(sizeof(int64_t) * (size_t)m);
  int64_t* pe = xmalloc(sizeof(int64_t) * (size_t)m);
  OK(dglhip_neighbor_sample_host_fetch(nv, m, vertices, layers, src, dst, pe));

  int64_t want_edges = 0, zero_layer = 0;
  for (int64_t i = 0; i < nv; ++i) {
    CHECK(vertices[i] >= 0 && vertices[i] < n, "vertex %lld", (long long)vertices[i]);
    CHECK(i == 0 || vertices[i - 1] < vertices[i], "vertices are not ascending");
    CHECK(layers[i] >= 0 && layers[i] <= num_hops, "layer %lld", (long long)layers[i]);
    zero_layer += layers[i] == 0;
    if (layers[i] < num_hops) {
      const int64_t d = indptr[vertices[i] + 1] - indptr[vertices[i]];
      want_edges += d < fanout ? d : fanout;
    }
  }
  for (int64_t i = 0; i < num_seeds; ++i) {
    int found = 0;
    for (int64_t j = 0; j < nv; ++j) found |= vertices[j] == seeds[i] && layers[j] == 0;
    CHECK(found, "seed %lld is not at layer 0", (long long)seeds[i]);
  }
  CHECK(zero_layer <= num_seeds, "more layer-0 vertices than seeds");
  CHECK(m == want_edges, "%lld edges, the rows give %lld", (long long)m, (long long)want_edges);
  for (int64_t j = 0; j < m; ++j) {
    const int64_t slot = nnz - 1 - pe[j];
    CHECK(slot >= 0 && slot < nnz, "edge id %lld", (long long)pe[j]);
    const int64_t row = in_dir ? dst[j] : src[j], other = in_dir ? src[j] : dst[j];
    CHECK(row >= 0 && row < nv && other >= -1 && other < nv, "endpoints");
    const int64_t v = vertices[row];
    CHECK(slot >= indptr[v] && slot < indptr[v + 1], "edge %lld is not a slot of its row",
          (long long)j);
    const int32_t nbr = indices[slot];
    if (nbr < 0 || nbr >= n) CHECK(other == -1, "a neighbour outside the graph was followed");
    else CHECK(other >= 0 && vertices[other] == nbr, "edge %lld ends elsewhere", (long long)j);
    CHECK(j == 0 || (in_dir ? dst : src)[j - 1] < row ||
              ((in_dir ? dst : src)[j - 1] == row && pe[j - 1] > pe[j]),
          "edges are not in row order, ascending position");
    /* a weightless slot only when the row has fewer weighted ones than the fan-out */
    const int weighted_slot = nbr >= 0 && nbr < n && has_weight(weight[nbr]);
    const int64_t d = indptr[v + 1] - indptr[v];
    if (!weighted_slot && d > fanout) {
      int64_t weighted = 0;
      for (int64_t s = indptr[v]; s < indptr[v + 1]; ++s)
        weighted += indices[s] >= 0 && indices[s] < n && has_weight(weight[indices[s]]);
      CHECK(weighted < fanout, "a weightless slot of a row with %lld weighted ones",
            (long long)weighted);
    }
  }
  /* nothing is left to fetch */
  if (nv > 0) REFUSED(dglhip_neighbor_sample_host_fetch(nv, m, vertices, layers, src, dst, pe));

  /* the error paths: nothing is read through a refused argument */
  REFUSED(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, indices, eid, NULL, in_dir, seeds,
                                               num_seeds, num_hops, fanout, 1, sizes));
  REFUSED(dglhip_neighbor_sample_host_weighted(-1, nnz, indptr, indices, eid, weight, in_dir,
                                               seeds, num_seeds, num_hops, fanout, 1, sizes));
  REFUSED(dglhip_neighbor_sample_host_weighted(n, -1, indptr, indices, eid, weight, in_dir, seeds,
                                               num_seeds, num_hops, fanout, 1, sizes));
  REFUSED(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, indices, eid, weight, in_dir, seeds,
                                               -1, num_hops, fanout, 1, sizes));
  REFUSED(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, indices, eid, weight, in_dir, seeds,
                                               num_seeds, -1, fanout, 1, sizes));
  REFUSED(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, indices, eid, weight, in_dir, seeds,
                                               num_seeds, num_hops, -1, 1, sizes));
  REFUSED(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, indices, eid, weight, in_dir, seeds,
                                               num_seeds, num_hops, fanout, 1, NULL));
  const int64_t bad_ids[3] = {n, -1, (int64_t)1 << 40};
  for (int b = 0; b < 3; ++b) {
    const int64_t two[2] = {0, bad_ids[b]};
    REFUSED(dglhip_neighbor_sample_host_weighted(n, nnz, indptr, indices, eid, weight, in_dir,
                                                 two, 2, num_hops, fanout, 1, sizes));
    CHECK(strstr(DGLGetLastError(), "Invalid vertex") != NULL, "message: %s", DGLGetLastError());
  }
  free(indptr); free(indices); free(eid); free(weight); free(seeds);
  free(vertices); free(layers); free(src); free(dst); free(pe);
}

static uint64_t bits_of(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof(b));
  return b;
}

static void check_keys(void) {
  const uint64_t weightless = 0x7FF0000000000000ull;
  CHECK(dglhip_sample_neglog((uint64_t)1 << 53) == 0.0, "neglog(2^53)");
  CHECK(fabs(dglhip_sample_neglog(1) - 53 * log(2.0)) < 1e-12, "neglog(1)");
  double last = dglhip_sample_neglog(1);
  for (uint64_t m = 2; m <= ((uint64_t)1 << 53); m += 1 + m / 3) {
    const double e = dglhip_sample_neglog(m);
    CHECK(e >= 0 && e <= last, "neglog is not monotone at %llu", (unsigned long long)m);
    CHECK(fabs(e + log((double)m) - 53 * log(2.0)) <= 1e-12 * (e > 1 ? e : 1), "neglog(%llu)",
          (unsigned long long)m);
    last = e;
  }
  (void)dglhip_sample_neglog(0); /* outside the rule's range: defined, no UB */
  (void)dglhip_sample_neglog(~(uint64_t)0);
  const float none[7] = {0.0f, -0.0f, 1e-40f, -1.0f, INFINITY, -INFINITY, NAN};
  for (uint64_t seed = 0; seed < 50; ++seed)
    for (int64_t p = 0; p < 20; ++p) {
      const int64_t v = (int64_t)(rnd() % 100000);
      for (int i = 0; i < 7; ++i)
        CHECK(dglhip_sample_weighted_key(seed, v, p, none[i]) == weightless, "weightless %d", i);
      const double e = dglhip_sample_neglog((dglhip_sample_key(seed, v, p) >> 11) + 1);
      CHECK(dglhip_sample_weighted_key(seed, v, p, 1.0f) == bits_of(e), "weight 1");
      CHECK(dglhip_sample_weighted_key(seed, v, p, 3.5f) == bits_of(e / 3.5), "weight 3.5");
      CHECK(dglhip_sample_weighted_key(seed, v, p, 1.17549435e-38f) < weightless, "tiny");
      CHECK(dglhip_sample_weighted_key(seed, v, p, 3.40282347e+38f) < weightless, "huge");
    }
}

int main(void) {
  check_keys();
  for (int in_dir = 0; in_dir < 2; ++in_dir) {
    run_case(1, 0, 3, 1, in_dir, 1);         /* one node, no edge */
    run_case(6, 0, 3, 2, in_dir, 0);         /* no seeds */
    run_case(50, 5, 0, 2, in_dir, 4);        /* fan-out 0 */
    run_case(50, 5, 4, 0, in_dir, 4);        /* no hops */
    run_case(300, 700, 1, 2, in_dir, 5);     /* fan-out 1, a long row */
    run_case(300, 700, 5, 3, in_dir, 9);
    run_case(300, 257, 64, 2, in_dir, 30);
    run_case(300, 256, 1000, 2, in_dir, 30); /* every row kept whole */
  }
  printf("weighted_sample_sanitize ok\n");
  return 0;
}
