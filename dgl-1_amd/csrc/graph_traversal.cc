// Host graph traversals over the native index, under the reference's registry
// names (traversal._CAPI_DGL*; semantics of src/graph/traversal.h and
// traversal.cc there, restated over the flat CSRs of graph_index.h):
//   BFSNodes / BFSEdges       level-synchronous breadth-first frontiers,
//   TopologicalNodes          Kahn's algorithm, one frontier per level,
//   DFSEdges / DFSLabeledEdges  per-source depth-first edge traces, merged
//                             position-wise.
// Every function walks Graph::out_csr() (in_csr() with `reversed`), so both the
// mutable and the immutable index work; a row's slot order is the order of the
// reference's SuccVec / PredVec / OutEdgeVec / InEdgeVec. Each call returns an
// indexable list of int64 host arrays: (ids, sections), or (ids, labels,
// sections) for the labelled DFS. The frontiers are consecutive runs of `ids`
// whose lengths are `sections`; a zero-length frontier is never listed.
//
// csrc/traversal.hip computes the first three on the device with the same
// answer, element for element.
#include "graph_index.h"

#include <algorithm>

namespace dglhip {
namespace gi {

using rt::Args;
using rt::NDArray;
using rt::RetValue;

namespace {

struct Frontiers {
  id_vec ids, labels, sections;
};

// The reference does not check the sources (traversal.h:57-63 indexes
// `visited` with them); here an id outside [0, N) raises.
void check_sources(const Graph& g, Ids source) {
  for (int64_t i = 0; i < source.n; ++i)
    DGLHIP_CHECK(g.has_vertex(source[i]), "Invalid source vertex: " << source[i]
                                              << " is not in a graph of " << g.num_vertices()
                                              << " vertices");
}

// One queue for the whole walk: `queue[head, tail)` is the frontier being
// expanded and everything pushed meanwhile is the next one. The first frontier
// is `source` as given (a repeated id stays repeated; its second expansion
// finds every neighbour visited). With `edges` the output is the id of the edge
// that discovered each node, and the source frontier is not listed.
Frontiers bfs(const Graph& g, Ids source, bool reversed, bool edges) {
  check_sources(g, source);
  const CSRPtr c = reversed ? g.in_csr() : g.out_csr();
  std::vector<bool> visited(static_cast<size_t>(g.num_vertices()), false);
  Frontiers out;
  id_vec nodes;
  id_vec& queue = edges ? nodes : out.ids;
  for (int64_t i = 0; i < source.n; ++i) {
    visited[source[i]] = true;
    queue.push_back(source[i]);
  }
  if (!edges && source.n > 0) out.sections.push_back(source.n);
  size_t head = 0;
  while (head < queue.size()) {
    const size_t tail = queue.size();
    for (; head < tail; ++head) {
      const int64_t u = queue[head];
      for (int64_t k = c->indptr[u]; k < c->indptr[u + 1]; ++k) {
        const int64_t v = c->indices[k];
        if (visited[v]) continue;
        visited[v] = true;
        queue.push_back(v);
        if (edges) out.ids.push_back(c->eid[k]);
      }
    }
    if (queue.size() > tail) out.sections.push_back(static_cast<int64_t>(queue.size() - tail));
  }
  return out;
}

// Kahn's algorithm with one queue. The first frontier is the nodes without
// in-edges (out-edges with `reversed`) in ascending id; a node joins the queue
// at the decrement that brings its counter to zero, and a multi-edge
// decrements once per edge.
Frontiers topological(const Graph& g, bool reversed) {
  const CSRPtr walk = reversed ? g.in_csr() : g.out_csr();
  const CSRPtr opposite = reversed ? g.out_csr() : g.in_csr();
  const int64_t n = g.num_vertices();
  id_vec remain(static_cast<size_t>(n));
  Frontiers out;
  id_vec& queue = out.ids;
  for (int64_t v = 0; v < n; ++v) {
    remain[v] = opposite->degree(v);
    if (remain[v] == 0) queue.push_back(v);
  }
  if (!queue.empty()) out.sections.push_back(static_cast<int64_t>(queue.size()));
  size_t head = 0;
  while (head < queue.size()) {
    const size_t tail = queue.size();
    for (; head < tail; ++head) {
      const int64_t u = queue[head];
      for (int64_t k = walk->indptr[u]; k < walk->indptr[u + 1]; ++k)
        if (--remain[walk->indices[k]] == 0) queue.push_back(walk->indices[k]);
    }
    if (queue.size() > tail) out.sections.push_back(static_cast<int64_t>(queue.size() - tail));
  }
  DGLHIP_CHECK(static_cast<int64_t>(queue.size()) == n,
               "Error in topological traversal: loop detected in the given graph.");
  return out;
}

// The labels of dfs_labeled_edges_generator: FORWARD, REVERSE, NONTREE.
enum DFSLabel : int64_t { kTreeDown = 0, kTreeUp = 1, kOffTree = 2 };

// Depth-first edge trace from one source (traversal.h:239-288). The stack holds
// (node, slot, the slot's edge was taken as a tree edge). The top's edge u -> v
// is looked at: an unvisited v makes it a FORWARD edge, marks the entry as
// on the tree and descends into v when v has out-edges; a visited v closes the
// slot (REVERSE when the entry is on the tree, i.e. on the way back up, NONTREE
// otherwise) and moves the entry to u's next slot.
template <typename Visit>
void dfs_from(const CSR& c, int64_t num_vertices, int64_t source, bool has_reverse_edge,
              bool has_nontree_edge, Visit&& visit) {
  if (c.degree(source) == 0) return;
  struct Entry {
    int64_t u, slot;
    bool on_tree;
  };
  std::vector<Entry> stack;
  std::vector<bool> visited(static_cast<size_t>(num_vertices), false);
  visited[source] = true;
  stack.push_back({source, c.indptr[source], false});
  while (!stack.empty()) {
    Entry& top = stack.back();
    const int64_t u = top.u, k = top.slot;
    const int64_t v = c.indices[k];
    if (visited[v]) {
      if (!top.on_tree && has_nontree_edge) visit(c.eid[k], kOffTree);
      else if (top.on_tree && has_reverse_edge) visit(c.eid[k], kTreeUp);
      stack.pop_back();
      if (k + 1 < c.indptr[u + 1]) stack.push_back({u, k + 1, false});
    } else {
      visited[v] = true;
      top.on_tree = true;
      visit(c.eid[k], kTreeDown);
      if (c.degree(v) > 0) stack.push_back({v, c.indptr[v], false});  // `top` dangles from here
    }
  }
}

// One trace per source, each with its own visited set, merged position-wise:
// frontier i holds the i-th edge of every trace that is that long, in source
// order (MergeMultipleTraversals / ComputeMergedSections, traversal.cc:49-97).
Frontiers dfs(const Graph& g, Ids source, bool reversed, bool has_reverse_edge,
              bool has_nontree_edge, bool labels) {
  check_sources(g, source);
  const CSRPtr c = reversed ? g.in_csr() : g.out_csr();
  std::vector<id_vec> edges(static_cast<size_t>(source.n)), tags(static_cast<size_t>(source.n));
  size_t longest = 0;
  for (int64_t i = 0; i < source.n; ++i) {
    dfs_from(*c, g.num_vertices(), source[i], has_reverse_edge, has_nontree_edge,
             [&](int64_t e, int64_t tag) {
               edges[i].push_back(e);
               if (labels) tags[i].push_back(tag);
             });
    longest = std::max(longest, edges[i].size());
  }
  Frontiers out;
  for (size_t p = 0; p < longest; ++p) {
    int64_t len = 0;
    for (size_t i = 0; i < edges.size(); ++i) {
      if (p >= edges[i].size()) continue;
      out.ids.push_back(edges[i][p]);
      if (labels) out.labels.push_back(tags[i][p]);
      ++len;
    }
    out.sections.push_back(len);
  }
  return out;
}

void ret_frontiers(const Frontiers& f, bool labels, RetValue* rv) {
  std::vector<NDArray> arrays{NDArray::FromVector(f.ids)};
  if (labels) arrays.push_back(NDArray::FromVector(f.labels));
  arrays.push_back(NDArray::FromVector(f.sections));
  rv->set_func(rt::ndarray_vector_func(std::move(arrays)));
}

}  // namespace
}  // namespace gi

void register_traversal_functions() {
  using namespace gi;
  using rt::register_global;
  const std::string ns = "traversal._CAPI_";

  // (handle, source, reversed) -> [node ids, sections]
  register_global(ns + "DGLBFSNodes", [](const Args& a, RetValue* rv) {
    ret_frontiers(bfs(*graph_arg(a, 0), id_arg(a, 1), a.b(2), false), false, rv);
  });
  // (handle, source, reversed) -> [edge ids, sections]
  register_global(ns + "DGLBFSEdges", [](const Args& a, RetValue* rv) {
    ret_frontiers(bfs(*graph_arg(a, 0), id_arg(a, 1), a.b(2), true), false, rv);
  });
  // (handle, reversed) -> [node ids, sections]
  register_global(ns + "DGLTopologicalNodes", [](const Args& a, RetValue* rv) {
    ret_frontiers(topological(*graph_arg(a, 0), a.b(1)), false, rv);
  });
  // (handle, source, reversed) -> [edge ids, sections]: FORWARD edges only
  register_global(ns + "DGLDFSEdges", [](const Args& a, RetValue* rv) {
    ret_frontiers(dfs(*graph_arg(a, 0), id_arg(a, 1), a.b(2), false, false, false), false, rv);
  });
  // (handle, source, reversed, has_reverse_edge, has_nontree_edge, return_labels)
  // -> [edge ids, labels, sections], or [edge ids, sections] without labels
  register_global(ns + "DGLDFSLabeledEdges", [](const Args& a, RetValue* rv) {
    const bool labels = a.b(5);
    ret_frontiers(dfs(*graph_arg(a, 0), id_arg(a, 1), a.b(2), a.b(3), a.b(4), labels), labels,
                  rv);
  });
}

}  // namespace dglhip
