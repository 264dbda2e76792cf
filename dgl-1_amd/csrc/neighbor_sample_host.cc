// Host twin of csrc/neighbor_sample.hip: the same sample from the same arrays
// by the rules of sample_key.h (uniform, or weighted by a node weight), with
// std::nth_element on (key, position) where the device runs a radix select.
// It is the CPU route of a seeded NeighborSampler and what the device route is
// compared against, bit for bit.
#include "../../include/dgl_hip.h"
#include "common.h"
#include "sample_key.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace dglhip {

namespace {

struct HostSample {
  std::vector<int64_t> vertices, layers, src, dst, eid;
};

// The result of the last dglhip_neighbor_sample_host call of this thread,
// until dglhip_neighbor_sample_host_fetch copies it out.
thread_local HostSample t_sample;

// The selected positions of a row of d slots, ascending; key_of(p) is the key
// of slot p.
template <typename KeyOf>
void select_positions(const KeyOf& key_of, int64_t d, int64_t k, std::vector<int64_t>* pos) {
  pos->clear();
  if (k <= 0 || d <= 0) return;
  if (d <= k) {
    for (int64_t p = 0; p < d; ++p) pos->push_back(p);
    return;
  }
  std::vector<std::pair<uint64_t, int64_t>> keys(static_cast<size_t>(d));
  for (int64_t p = 0; p < d; ++p) keys[p] = {key_of(p), p};
  std::nth_element(keys.begin(), keys.begin() + k, keys.end());
  for (int64_t i = 0; i < k; ++i) pos->push_back(keys[i].second);
  std::sort(pos->begin(), pos->end());
}

// The sample of dglhip_neighbor_sample_host[_weighted], left in t_sample.
void sample_on_host(int64_t num_nodes, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                    const int64_t* eid, const float* node_weight, bool weighted, int in_direction,
                    const int64_t* seeds, int64_t num_seeds, int num_hops, int64_t fanout,
                    uint64_t seed, int64_t* sizes) {
  const int64_t N = num_nodes;
  DGLHIP_CHECK(N >= 0 && nnz >= 0 && num_seeds >= 0, "negative size");
  DGLHIP_CHECK(N < (int64_t(1) << 31), "node ids are 32-bit in the CSR");
  DGLHIP_CHECK(num_hops >= 0 && fanout >= 0, "invalid sampling parameters");
  DGLHIP_CHECK(indptr && sizes && (nnz == 0 || (indices && eid)) && (num_seeds == 0 || seeds) &&
                   (!weighted || node_weight),
               "null pointer argument");
  HostSample out;
  std::vector<int32_t> layer(static_cast<size_t>(N), -1);
  std::vector<int64_t> front, next;
  int64_t invalid = 0;
  for (int64_t i = 0; i < num_seeds; ++i) {
    const int64_t v = seeds[i];
    if (v < 0 || v >= N) {
      ++invalid;
    } else if (layer[v] < 0) {
      layer[v] = 0;
      front.push_back(v);
    }
  }
  DGLHIP_CHECK(invalid == 0, "Invalid vertex: " << invalid << " of the " << num_seeds
                                                << " seeds are not in a graph of " << N
                                                << " nodes");
  auto row = [&](int64_t v, int64_t* beg, int64_t* end) {
    int64_t b = indptr[v], e = indptr[v + 1];
    b = b < 0 ? 0 : (b > nnz ? nnz : b);
    e = e < b ? b : (e > nnz ? nnz : e);
    *beg = b;
    *end = e;
  };
  // the selection of the row of v, whose slots are [beg, end)
  std::vector<int64_t> pos;
  auto select = [&](int64_t v, int64_t beg, int64_t end) {
    const uint64_t rb = sample_row_base(seed, v);
    if (!weighted) {
      select_positions([&](int64_t p) { return sample_slot_key(rb, p); }, end - beg, fanout, &pos);
      return;
    }
    select_positions(
        [&](int64_t p) {
          const int64_t nbr = indices[beg + p];
          uint32_t wbits = 0;  // a neighbour outside [0, N) is weightless
          if (nbr >= 0 && nbr < N) std::memcpy(&wbits, node_weight + nbr, sizeof(wbits));
          return sample_weighted_slot_key(sample_slot_key(rb, p), wbits);
        },
        end - beg, fanout, &pos);
  };
  for (int h = 0; h < num_hops && fanout > 0 && !front.empty(); ++h) {
    next.clear();
    for (int64_t v : front) {
      int64_t beg, end;
      row(v, &beg, &end);
      select(v, beg, end);
      for (int64_t p : pos) {
        const int64_t nbr = indices[beg + p];
        if (nbr < 0 || nbr >= N || layer[nbr] >= 0) continue;
        layer[nbr] = h + 1;
        next.push_back(nbr);
      }
    }
    front.swap(next);
  }
  std::vector<int64_t> newid(static_cast<size_t>(N), -1);
  for (int64_t v = 0; v < N; ++v) {
    if (layer[v] < 0) continue;
    newid[v] = static_cast<int64_t>(out.vertices.size());
    out.vertices.push_back(v);
    out.layers.push_back(layer[v]);
  }
  for (size_t i = 0; i < out.vertices.size(); ++i) {
    const int64_t v = out.vertices[i];
    if (out.layers[i] >= num_hops) continue;
    int64_t beg, end;
    row(v, &beg, &end);
    select(v, beg, end);
    for (int64_t p : pos) {
      const int64_t nbr = indices[beg + p];
      const int64_t nid = nbr >= 0 && nbr < N ? newid[nbr] : -1;
      out.src.push_back(in_direction ? nid : static_cast<int64_t>(i));
      out.dst.push_back(in_direction ? static_cast<int64_t>(i) : nid);
      out.eid.push_back(eid[beg + p]);
    }
  }
  sizes[0] = static_cast<int64_t>(out.vertices.size());
  sizes[1] = static_cast<int64_t>(out.eid.size());
  t_sample = std::move(out);
}

}  // namespace

}  // namespace dglhip

using namespace dglhip;

extern "C" {

uint64_t dglhip_sample_mix(uint64_t z) { return sample_mix(z); }

uint64_t dglhip_sample_key(uint64_t seed, int64_t vertex, int64_t position) {
  return sample_key(seed, vertex, position);
}

double dglhip_sample_neglog(uint64_t m) { return sample_neglog(m); }

uint64_t dglhip_sample_weighted_key(uint64_t seed, int64_t vertex, int64_t position,
                                    float weight) {
  return sample_weighted_key(seed, vertex, position, weight);
}

int dglhip_neighbor_sample_host(int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                                const int32_t* indices, const int64_t* eid, int in_direction,
                                const int64_t* seeds, int64_t num_seeds, int num_hops,
                                int64_t fanout, uint64_t seed, int64_t* sizes) {
  API_BEGIN();
  sample_on_host(num_nodes, nnz, indptr, indices, eid, nullptr, false, in_direction, seeds,
                 num_seeds, num_hops, fanout, seed, sizes);
  API_END();
}

int dglhip_neighbor_sample_host_weighted(int64_t num_nodes, int64_t nnz, const int64_t* indptr,
                                         const int32_t* indices, const int64_t* eid,
                                         const float* node_weight, int in_direction,
                                         const int64_t* seeds, int64_t num_seeds, int num_hops,
                                         int64_t fanout, uint64_t seed, int64_t* sizes) {
  API_BEGIN();
  sample_on_host(num_nodes, nnz, indptr, indices, eid, node_weight, true, in_direction, seeds,
                 num_seeds, num_hops, fanout, seed, sizes);
  API_END();
}

int dglhip_neighbor_sample_host_fetch(int64_t num_vertices, int64_t num_edges, int64_t* vertices,
                                      int64_t* layers, int64_t* sub_src, int64_t* sub_dst,
                                      int64_t* parent_eid) {
  API_BEGIN();
  HostSample s = std::move(t_sample);
  t_sample = HostSample();
  DGLHIP_CHECK(num_vertices == static_cast<int64_t>(s.vertices.size()) &&
                   num_edges == static_cast<int64_t>(s.eid.size()),
               "no sample of " << num_vertices << " vertices and " << num_edges
                               << " edges is waiting on this thread");
  DGLHIP_CHECK((num_vertices == 0 || (vertices && layers)) &&
                   (num_edges == 0 || (sub_src && sub_dst && parent_eid)),
               "null pointer argument");
  if (num_vertices) {
    std::memcpy(vertices, s.vertices.data(), size_t(num_vertices) * 8);
    std::memcpy(layers, s.layers.data(), size_t(num_vertices) * 8);
  }
  if (num_edges) {
    std::memcpy(sub_src, s.src.data(), size_t(num_edges) * 8);
    std::memcpy(sub_dst, s.dst.data(), size_t(num_edges) * 8);
    std::memcpy(parent_eid, s.eid.data(), size_t(num_edges) * 8);
  }
  API_END();
}

}  // extern "C"
