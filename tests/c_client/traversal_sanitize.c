/* The host traversals (csrc/graph_traversal.cc) under AddressSanitizer +
 * UndefinedBehaviorSanitizer: a stand-alone program, linked with the sanitized
 * host library (make -C dgl-1_amd/csrc asan), that drives the five
 * traversal._CAPI_* functions through the PackedFunc convention on random
 * multigraphs (self loops, duplicate edges, isolated nodes, cycles), on the
 * mutable and the immutable index, forward and reversed, and on the error
 * paths (a source outside the graph, a loop under the topological order).
 * Built and run by tests/test_traversal_sanitize.py; any invalid access, leak
 * in our code or UB aborts with a report. The results are checked for the
 * properties every answer has: sections sum to the id count and hold no zero,
 * BFS lists a non-source node at most once and an edge frontier is as long as
 * the node frontier it discovered, the topological order respects every edge,
 * labels are 0, 1 or 2. Host only: no GPU needed. */
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

static DGLHipFunctionHandle get(const char* name) {
  DGLHipFunctionHandle f = NULL;
  OK(DGLFuncGetGlobal(name, &f));
  CHECK(f != NULL, "missing %s", name);
  return f;
}

static DGLHipArrayHandle ids(const int64_t* v, int64_t n) {
  DGLHipArrayHandle a = NULL;
  OK(DGLArrayAlloc(&n, 1, 0, 64, 1, 1, 0, &a));
  if (n) OK(DGLArrayCopyFromBytes(a, (void*)v, (size_t)n * sizeof(int64_t)));
  return a;
}

typedef struct {
  int64_t* v;
  int64_t n;
} Vec;

/* element `which` of an indexable list of int64 arrays, copied out */
static Vec item(DGLHipFunctionHandle list, int which) {
  DGLHipValue w, ret;
  int wc = DGLHIP_TC_INT, rcode;
  w.v_int64 = which;
  OK(DGLFuncCall(list, &w, &wc, 1, &ret, &rcode));
  CHECK(rcode == DGLHIP_TC_NDARRAY_CONTAINER, "element %d is not an array", which);
  DGLHipArrayHandle arr = (DGLHipArrayHandle)ret.v_handle;
  const DGLHipTensor* t = (const DGLHipTensor*)arr;
  Vec out;
  out.n = t->ndim == 1 ? t->shape[0] : -1;
  CHECK(out.n >= 0, "element %d is not 1-D", which);
  out.v = xmalloc(sizeof(int64_t) * (size_t)out.n);
  if (out.n) OK(DGLArrayCopyToBytes(arr, out.v, (size_t)out.n * sizeof(int64_t)));
  OK(DGLArrayFree(arr));
  return out;
}

/* calls `name`(g, [source,] flags...) and returns the list; *failed is set
 * instead when the call reports an error */
static DGLHipFunctionHandle call(const char* name, void* g, DGLHipArrayHandle source,
                                 const int64_t* flags, int nflags, int* failed) {
  DGLHipValue args[8], ret;
  int codes[8], rcode, n = 0;
  args[n].v_handle = g;
  codes[n++] = DGLHIP_TC_HANDLE;
  if (source) {
    args[n].v_handle = source;
    codes[n++] = DGLHIP_TC_NDARRAY_CONTAINER;
  }
  for (int i = 0; i < nflags; ++i) {
    args[n].v_int64 = flags[i];
    codes[n++] = DGLHIP_TC_INT;
  }
  const int rc = DGLFuncCall(get(name), args, codes, n, &ret, &rcode);
  if (failed) {
    *failed = rc != 0;
    if (rc != 0) {
      CHECK(strlen(DGLGetLastError()) > 0, "%s failed without a message", name);
      return NULL;
    }
  } else {
    CHECK(rc == 0, "%s -> %s", name, DGLGetLastError());
  }
  CHECK(rcode == DGLHIP_TC_FUNC_HANDLE, "%s returned type %d", name, rcode);
  return ret.v_handle;
}

static void check_sections(Vec all, Vec sections) {
  int64_t total = 0;
  for (int64_t i = 0; i < sections.n; ++i) {
    CHECK(sections.v[i] > 0, "empty frontier %lld", (long long)i);
    total += sections.v[i];
  }
  CHECK(total == all.n, "sections hold %lld of %lld ids", (long long)total, (long long)all.n);
}

static void* make_graph(int64_t n, int64_t m, const int64_t* src, const int64_t* dst,
                        int readonly) {
  DGLHipValue args[6], ret;
  int codes[6], rcode;
  DGLHipArrayHandle s = ids(src, m), d = ids(dst, m);
  void* g;
  if (readonly) {
    int64_t* e = xmalloc(sizeof(int64_t) * (size_t)m);
    for (int64_t i = 0; i < m; ++i) e[i] = i;
    DGLHipArrayHandle ea = ids(e, m);
    args[0].v_handle = s; codes[0] = DGLHIP_TC_NDARRAY_CONTAINER;
    args[1].v_handle = d; codes[1] = DGLHIP_TC_NDARRAY_CONTAINER;
    args[2].v_handle = ea; codes[2] = DGLHIP_TC_NDARRAY_CONTAINER;
    args[3].v_int64 = 1; codes[3] = DGLHIP_TC_INT;
    args[4].v_int64 = n; codes[4] = DGLHIP_TC_INT;
    args[5].v_int64 = 1; codes[5] = DGLHIP_TC_INT;
    OK(DGLFuncCall(get("graph_index._CAPI_DGLGraphCreate"), args, codes, 6, &ret, &rcode));
    g = ret.v_handle;
    OK(DGLArrayFree(ea));
    free(e);
  } else {
    args[0].v_int64 = 1; codes[0] = DGLHIP_TC_INT;
    OK(DGLFuncCall(get("graph_index._CAPI_DGLGraphCreateMutable"), args, codes, 1, &ret,
                   &rcode));
    g = ret.v_handle;
    args[0].v_handle = g; codes[0] = DGLHIP_TC_HANDLE;
    args[1].v_int64 = n; codes[1] = DGLHIP_TC_INT;
    OK(DGLFuncCall(get("graph_index._CAPI_DGLGraphAddVertices"), args, codes, 2, &ret, &rcode));
    if (m) {
      args[1].v_handle = s; codes[1] = DGLHIP_TC_NDARRAY_CONTAINER;
      args[2].v_handle = d; codes[2] = DGLHIP_TC_NDARRAY_CONTAINER;
      OK(DGLFuncCall(get("graph_index._CAPI_DGLGraphAddEdges"), args, codes, 3, &ret, &rcode));
    }
  }
  CHECK(g != NULL, "no graph handle");
  OK(DGLArrayFree(s));
  OK(DGLArrayFree(d));
  return g;
}

static void free_graph(void* g) {
  DGLHipValue a, ret;
  int c = DGLHIP_TC_HANDLE, rcode;
  a.v_handle = g;
  OK(DGLFuncCall(get("graph_index._CAPI_DGLGraphFree"), &a, &c, 1, &ret, &rcode));
}

/* n nodes, m random edges; `dag` keeps src < dst so the topological order exists */
static void run_case(int64_t n, int64_t m, int dag, int readonly, int64_t num_sources) {
  int64_t* src = xmalloc(sizeof(int64_t) * (size_t)m);
  int64_t* dst = xmalloc(sizeof(int64_t) * (size_t)m);
  const int64_t span = n > 4 ? n - 3 : n; /* the last nodes stay isolated */
  for (int64_t e = 0; e < m; ++e) {
    int64_t u = (int64_t)(rnd() % (uint64_t)span), v = (int64_t)(rnd() % (uint64_t)span);
    if (dag) {
      if (u == v) v = (u + 1) % span;
      if (u > v) { int64_t t = u; u = v; v = t; }
    } else if (e % 11 == 0) {
      v = u; /* self loops */
    }
    src[e] = u;
    dst[e] = v;
    if (e % 7 == 0 && e > 0) { src[e] = src[e - 1]; dst[e] = dst[e - 1]; } /* duplicates */
  }
  void* g = make_graph(n, m, src, dst, readonly);
  int64_t* sv = xmalloc(sizeof(int64_t) * (size_t)num_sources);
  for (int64_t i = 0; i < num_sources; ++i) sv[i] = (int64_t)(rnd() % (uint64_t)n);
  if (num_sources > 2) sv[num_sources - 1] = sv[0]; /* a repeated source */
  DGLHipArrayHandle source = ids(sv, num_sources);
  int* seen = xmalloc(sizeof(int) * (size_t)(n ? n : 1));

  for (int64_t reversed = 0; reversed < 2; ++reversed) {
    DGLHipFunctionHandle f = call("traversal._CAPI_DGLBFSNodes", g, source, &reversed, 1, NULL);
    Vec nodes = item(f, 0), nsec = item(f, 1);
    OK(DGLFuncFree(f));
    check_sections(nodes, nsec);
    CHECK(nodes.n >= num_sources && (num_sources == 0 || nsec.v[0] == num_sources),
          "the first frontier is not the source");
    memset(seen, 0, sizeof(int) * (size_t)(n ? n : 1));
    for (int64_t i = 0; i < nodes.n; ++i) {
      CHECK(nodes.v[i] >= 0 && nodes.v[i] < n, "node %lld", (long long)nodes.v[i]);
      if (i < num_sources) CHECK(nodes.v[i] == sv[i], "source %lld moved", (long long)i);
      else CHECK(!seen[nodes.v[i]], "node %lld listed twice", (long long)nodes.v[i]);
      seen[nodes.v[i]] = 1;
    }
    f = call("traversal._CAPI_DGLBFSEdges", g, source, &reversed, 1, NULL);
    Vec edges = item(f, 0), esec = item(f, 1);
    OK(DGLFuncFree(f));
    check_sections(edges, esec);
    CHECK(esec.n == (nsec.n ? nsec.n - 1 : 0), "edge frontiers: %lld for %lld node frontiers",
          (long long)esec.n, (long long)nsec.n);
    for (int64_t i = 0; i < esec.n; ++i) CHECK(esec.v[i] == nsec.v[i + 1], "frontier %lld", (long long)i);
    int64_t pos = num_sources;
    for (int64_t i = 0; i < edges.n; ++i, ++pos) {
      CHECK(edges.v[i] >= 0 && edges.v[i] < m, "edge %lld", (long long)edges.v[i]);
      CHECK((reversed ? src : dst)[edges.v[i]] == nodes.v[pos], "edge %lld does not end at its node",
            (long long)i);
    }
    free(nodes.v); free(nsec.v); free(edges.v); free(esec.v);

    int failed = 0;
    f = call("traversal._CAPI_DGLTopologicalNodes", g, NULL, &reversed, 1, &failed);
    if (dag) CHECK(!failed, "a DAG was refused: %s", DGLGetLastError());
    if (!failed) {
      Vec order = item(f, 0), osec = item(f, 1);
      OK(DGLFuncFree(f));
      check_sections(order, osec);
      CHECK(order.n == n, "%lld of %lld nodes", (long long)order.n, (long long)n);
      int64_t* level = xmalloc(sizeof(int64_t) * (size_t)(n ? n : 1));
      int64_t p = 0;
      for (int64_t l = 0; l < osec.n; ++l)
        for (int64_t k = 0; k < osec.v[l]; ++k) level[order.v[p++]] = l;
      for (int64_t e = 0; e < m; ++e)
        CHECK(reversed ? level[dst[e]] < level[src[e]] : level[src[e]] < level[dst[e]],
              "edge %lld is not respected", (long long)e);
      free(level); free(order.v); free(osec.v);
    }

    f = call("traversal._CAPI_DGLDFSEdges", g, source, &reversed, 1, NULL);
    Vec dfs = item(f, 0), dsec = item(f, 1);
    OK(DGLFuncFree(f));
    check_sections(dfs, dsec);
    for (int combo = 0; combo < 8; ++combo) {
      const int64_t flags[4] = {reversed, combo & 1, (combo >> 1) & 1, (combo >> 2) & 1};
      f = call("traversal._CAPI_DGLDFSLabeledEdges", g, source, flags, 4, NULL);
      Vec le = item(f, 0), ll, ls;
      if (flags[3]) {
        ll = item(f, 1);
        ls = item(f, 2);
        CHECK(ll.n == le.n, "labels: %lld for %lld edges", (long long)ll.n, (long long)le.n);
        for (int64_t i = 0; i < ll.n; ++i) CHECK(ll.v[i] >= 0 && ll.v[i] <= 2, "label");
        free(ll.v);
      } else {
        ls = item(f, 1);
      }
      OK(DGLFuncFree(f));
      check_sections(le, ls);
      if (combo == 0) CHECK(le.n == dfs.n && memcmp(le.v, dfs.v, sizeof(int64_t) * (size_t)le.n) == 0,
                            "DFSLabeledEdges without flags differs from DFSEdges");
      for (int64_t i = 0; i < le.n; ++i) CHECK(le.v[i] >= 0 && le.v[i] < m, "edge id");
      free(le.v); free(ls.v);
    }
    free(dfs.v); free(dsec.v);
  }

  /* a source outside the graph is refused by every function that takes one */
  const int64_t bad_ids[3] = {n, -1, (int64_t)1 << 40};
  for (int b = 0; b < 3; ++b) {
    int64_t two[2] = {0, bad_ids[b]};
    DGLHipArrayHandle bad = ids(n > 0 ? two : two + 1, n > 0 ? 2 : 1);
    const int64_t flags[4] = {0, 1, 1, 1};
    const char* names[4] = {"traversal._CAPI_DGLBFSNodes", "traversal._CAPI_DGLBFSEdges",
                            "traversal._CAPI_DGLDFSEdges", "traversal._CAPI_DGLDFSLabeledEdges"};
    for (int k = 0; k < 4; ++k) {
      int failed = 0;
      DGLHipFunctionHandle f = call(names[k], g, bad, flags, k == 3 ? 4 : 1, &failed);
      CHECK(failed && f == NULL, "%s accepted the id %lld", names[k], (long long)bad_ids[b]);
    }
    OK(DGLArrayFree(bad));
  }
  OK(DGLArrayFree(source));
  free_graph(g);
  free(src); free(dst); free(sv); free(seen);
}

int main(void) {
  for (int readonly = 0; readonly < 2; ++readonly) {
    run_case(1, 0, 1, readonly, 1);        /* one node, no edge */
    run_case(6, 0, 1, readonly, 0);        /* no edges, no sources */
    run_case(40, 30, 1, readonly, 3);      /* sparse DAG: many components */
    run_case(300, 2500, 1, readonly, 5);   /* DAG with multi-edges */
    run_case(300, 2500, 0, readonly, 5);   /* cycles, self loops: the loop error */
    run_case(2000, 3000, 0, readonly, 64); /* deep and narrow */
  }
  {
    /* a 3-cycle must raise, not spin */
    const int64_t s[4] = {0, 1, 2, 3}, d[4] = {1, 2, 3, 1};
    void* g = make_graph(5, 4, s, d, 0);
    const int64_t reversed = 0;
    int failed = 0;
    call("traversal._CAPI_DGLTopologicalNodes", g, NULL, &reversed, 1, &failed);
    CHECK(failed && strstr(DGLGetLastError(), "loop") != NULL, "a loop was not reported");
    free_graph(g);
  }
  printf("traversal_sanitize ok\n");
  return 0;
}
