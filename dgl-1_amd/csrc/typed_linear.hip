// Typed-edge dense g-SpMM for R-GCN's basis layer on the f32 MFMA
// (v_mfma_f32_16x16x4_f32): every relation has a full Fi x Fo weight,
//   out[v] = row_scale[v] * sum_{e=(u->v)} norm_e * (h[u] @ W[etype_e]).
//
// Replaces the reference's per-edge bmm (examples/pytorch/rgcn/layers.py:
// 94-98: gather W[type] into an E x Fi x Fo tensor, bmm, sum by destination).
// Grouped by relation the product is a grouped GEMM: the positions of one
// relation share one weight, so a 64-position item of the relation-major
// grouping (typed_items.h; built by dglhip_relation_groups_device) is a
// 64 x Fi by Fi x Fo product. Three pieces:
//   messages (here): one workgroup per item computes its 64 x Fo message rows
//     and stores each at its forward slot, msg[slot * Fo + j];
//   sum (typed_block.hip, dglhip_typed_msg_sum_device): each destination's
//     slot-order sum over its message rows, unchanged;
//   weight gradient (here): dW[r] = sum_p norm_p * x[src_p]^T (x) g[dst_p] as
//     a TN product per item, partials of relations with several items
//     combined in item order (launch_typed_combine). No atomics.
// The input gradient is the message kernel over the gradient rows with the
// weight read transposed, then the sum over the transposed CSR.
//
// Message kernel. Four waves, wave w owning positions 16w .. 16w + 15 of the
// item. The K dimension (Fi) runs in tiles of kKT = 32: the item's source
// rows are gathered through pos_row as whole coalesced row segments (32
// consecutive lanes read 128 B of one row) into xs[64][kKT + 2], and the
// relation's weight tile into ws[kKT][SW], once for the four waves; the next
// tile's values are loaded into registers before the current tile's MFMAs.
// Operand maps (node_linear.hip): lane l supplies A[row l&15][k l>>4] and
// B[k l>>4][col l&15]; D[row 4(l>>4)+i][col l&15] is accumulator register i.
//   A = xs[(16w + (l&15)) * 34 + 4s + (l>>4)]: the 32 lanes of a half-wave
//     (l>>4 in {0, 1} or {2, 3}) land on banks 2 (l&15) + (l>>4): all distinct;
//   B = ws[(4s + (l>>4)) * SW + 16t + (l&15)], SW = 16 NT (+ 16 when NT is
//     even) so that SW = 16 mod 32: the two k rows of a half-wave land 16
//     banks apart.
// Each wave keeps NT = ceil(Fo / 16) accumulator tiles (4 NT VGPRs) across
// the K loop. Ragged Fi (no multiple of 4) is zero-filled in both stages,
// ragged Fo and short items are masked at the store: nothing is written
// outside the item's own message rows.
//
// Gate (dglhip_typed_linear_ok): 1 <= Fi, Fo <= 256. At Fo = 256 a wave
// holds 64 accumulator VGPRs and 40 of prefetched operands (152 VGPRs as
// compiled, no scratch), and the weight tile takes 32 x 272 floats = 34 KiB
// of LDS, 43.5 KiB with the rows; twice that width would need 128
// accumulators a lane and a 68 KiB tile, past a workgroup's static 64 KiB.
//
// Each output element is the MFMA's f32 fma chain over k (f32 products, no
// wider accumulation): an ordinary GEMM's association. Nothing promises the
// scalar kernels' bits (typed_block.hip): the order inside one instruction's
// 4 k values is the hardware's, and dW folds the norm into the gradient row
// where the scalar kernel folds it into the source value.
#include <hip/hip_runtime.h>

#include "../../include/dgl_hip.h"
#include "common.h"
#include "launch.h"
#include "timing.h"
#include "typed_items.h"

namespace dglhip {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kKT = 32;        // k values per staged tile
constexpr int kSA = kKT + 2;   // row stride of the staged source rows
constexpr int kMaxWidth = 256; // the gate

template <int NT>
__global__ __launch_bounds__(256) void typed_linear_msg_kernel(
    int64_t num_items, int64_t num_rels, int Fi, int Fo, const int64_t* __restrict__ rel_ptr,
    const int64_t* __restrict__ item_ptr, const int32_t* __restrict__ item_rel,
    const int32_t* __restrict__ pos_row, const int64_t* __restrict__ pos_slot,
    const float* __restrict__ ufeat, const float* __restrict__ operand_scale,
    const float* __restrict__ weight, int wtrans, float* __restrict__ msg) {
  constexpr int NP = 16 * NT;
  constexpr int SW = NP + ((NT & 1) ? 0 : 16);
  constexpr int AQ = 64 * kKT / 256;
  constexpr int BQ = kKT * NP / 256;
  __shared__ float xs[64 * kSA];
  __shared__ float ws[kKT * SW];
  __shared__ int64_t slot_s[64];
  __shared__ int rid[64];
  __shared__ float rsc[64];
  const int64_t it = block_linear();
  if (it >= num_items) return;  // the whole workgroup
  int64_t rel, beg, end;
  bool single;
  if (!item_range(it, num_rels, rel_ptr, item_ptr, item_rel, &rel, &beg, &end, &single)) return;
  const int cnt = static_cast<int>(end - beg);  // <= 64, uniform
  if (cnt == 0) return;
  const int t = threadIdx.x;
  if (t < 64) {
    const bool on = t < cnt;
    const int row = on ? pos_row[beg + t] : -1;
    rid[t] = row;
    slot_s[t] = on ? pos_slot[beg + t] : 0;
    rsc[t] = (on && operand_scale) ? operand_scale[row] : 1.0f;
  }
  __syncthreads();
  const float* wr = weight + rel * int64_t(Fi) * int64_t(Fo);
  float av[AQ], bv[BQ];
  // thread t stages column t & 31 of rows (t >> 5) + 8 q of the tile
  auto load_tile = [&](int k0) {
    const int k = k0 + (t & 31);
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const int p = (t >> 5) + 8 * q;
      const int row = rid[p];
      float x = 0.0f;
      if (row >= 0 && k < Fi) {
        x = ufeat[int64_t(row) * Fi + k];
        // a scaled operand row (the backward's dout * norm[dst]) as torch's
        // product rounds it
        if (operand_scale) x = x * rsc[p];
      }
      av[q] = x;
    }
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
      const int idx = t + 256 * q;
      float v = 0.0f;
      if (wtrans) {  // weight[rel] is (Fo, Fi): k runs along its rows
        const int kk = k0 + idx % kKT, n = idx / kKT;
        if (kk < Fi && n < Fo) v = wr[int64_t(n) * Fi + kk];
      } else {
        const int n = idx % NP, kk = k0 + idx / NP;
        if (kk < Fi && n < Fo) v = wr[int64_t(kk) * Fo + n];
      }
      bv[q] = v;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int q = 0; q < AQ; ++q) xs[((t >> 5) + 8 * q) * kSA + (t & 31)] = av[q];
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
      const int idx = t + 256 * q;
      if (wtrans) ws[(idx % kKT) * SW + idx / kKT] = bv[q];
      else ws[(idx / NP) * SW + idx % NP] = bv[q];
    }
  };
  const int w = t >> 6, lane = t & 63, r = lane & 15, h = lane >> 4;
  const bool busy = 16 * w < cnt;  // wave-uniform: the strip holds a position
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  load_tile(0);
  for (int k0 = 0; k0 < Fi; k0 += kKT) {
    store_tile();
    __syncthreads();
    if (k0 + kKT < Fi) load_tile(k0 + kKT);
    if (busy) {
      const int left = Fi - k0;
      const int nsteps = ((left < kKT ? left : kKT) + 3) >> 2;
      const float* ap = xs + (16 * w + r) * kSA + h;
      const float* bp = ws + h * SW + r;
      for (int s = 0; s < nsteps; ++s) {
        const float a = ap[4 * s];
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[4 * s * SW + 16 * j], acc[j], 0, 0,
                                                        0);
      }
    }
    __syncthreads();
  }
  if (!busy) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = 16 * w + 4 * h + i;
    if (p >= cnt) continue;
    float* mrow = msg + slot_s[p] * Fo;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = 16 * j + r;
      if (col < Fo) mrow[col] = acc[j][i];
    }
  }
}

// dW of item `it` (at most 64 positions of relation r), a 64 x 64 block of
// it per workgroup: block (ig, jg) holds rows 64 ig .. and columns 64 jg ..;
// wave w owns row tile w of the block and its four column tiles (16
// accumulator VGPRs). The positions' source columns and gradient columns of
// the block are staged once, xs[p][64] and gs[p][64] at a stride of kWS = 80
// floats (= 16 mod 32: the two positions a half-wave reads land 16 banks
// apart), the gradient scaled by row_scale[dst] and the position's norm in
// the stage. D = xs^T gs: lane l supplies A[row i = l&15][k = position 4s +
// (l>>4)] and B[k][col j = l&15].
constexpr int kWS = 80;

__global__ __launch_bounds__(256) void typed_linear_wgrad_kernel(
    int64_t num_items, int64_t num_rels, int Fi, int Fo, int gi, int gj,
    const int64_t* __restrict__ rel_ptr, const int64_t* __restrict__ item_ptr,
    const int32_t* __restrict__ item_rel, const int32_t* __restrict__ rel_src,
    const int32_t* __restrict__ rel_dst, const float* __restrict__ rel_norm,
    const float* __restrict__ ufeat, const float* __restrict__ dout,
    const float* __restrict__ dout_scale, float* __restrict__ dw,
    float* __restrict__ partial) {
  __shared__ float xs[64 * kWS];
  __shared__ float gs[64 * kWS];
  __shared__ int sid[64], did[64];
  __shared__ float fsc[64], fnr[64];
  const int64_t blk = block_linear();
  const int64_t it = blk / (gi * gj);
  if (it >= num_items) return;  // the whole workgroup
  const int g = static_cast<int>(blk - it * (gi * gj));
  const int i0 = 64 * (g / gj), j0 = 64 * (g % gj);
  int64_t rel, beg, end;
  bool single;
  if (!item_range(it, num_rels, rel_ptr, item_ptr, item_rel, &rel, &beg, &end, &single)) return;
  const int cnt = static_cast<int>(end - beg);  // <= 64, uniform; 0: zeros
  const int cnt4 = (cnt + 3) & ~3;
  const int t = threadIdx.x;
  if (t < 64) {
    const bool on = t < cnt;
    const int d = on ? rel_dst[beg + t] : 0;
    sid[t] = on ? rel_src[beg + t] : -1;
    did[t] = d;
    fsc[t] = (on && dout_scale) ? dout_scale[d] : 1.0f;
    fnr[t] = (on && rel_norm) ? rel_norm[beg + t] : 1.0f;
  }
  __syncthreads();
  // thread t stages column t & 63 of positions (t >> 6) + 4 q
  const int c = t & 63;
  float xv[16], gv[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int p = (t >> 6) + 4 * q;
    const int s = p < cnt4 ? sid[p] : -1;
    float x = 0.0f, gg = 0.0f;
    if (s >= 0) {
      if (i0 + c < Fi) x = ufeat[int64_t(s) * Fi + i0 + c];
      if (j0 + c < Fo) {
        gg = dout[int64_t(did[p]) * Fo + j0 + c];
        if (dout_scale) gg = gg * fsc[p];  // dout * row_scale as torch rounds it
        if (rel_norm) gg = fnr[p] * gg;
      }
    }
    xv[q] = x;
    gv[q] = gg;
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int p = (t >> 6) + 4 * q;
    if (p < cnt4) {
      xs[p * kWS + c] = xv[q];
      gs[p * kWS + c] = gv[q];
    }
  }
  __syncthreads();
  const int w = t >> 6, lane = t & 63, r = lane & 15, h = lane >> 4;
  if (i0 + 16 * w >= Fi) return;  // wave-uniform: no row of the tile exists
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* ap = xs + h * kWS + 16 * w + r;
  const float* bp = gs + h * kWS + r;
  for (int s = 0; s < (cnt4 >> 2); ++s) {
    const float a = ap[4 * s * kWS];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[4 * s * kWS + 16 * j], acc[j], 0, 0, 0);
  }
  const int64_t wr = int64_t(Fi) * Fo;
  float* dst = single ? dw + rel * wr : partial + it * wr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i0 + 16 * w + 4 * h + i;
    if (row >= Fi) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = j0 + 16 * j + r;
      if (col < Fo) dst[int64_t(row) * Fo + col] = acc[j][i];
    }
  }
}

}  // namespace
}  // namespace dglhip

using namespace dglhip;

extern "C" {

int dglhip_typed_linear_ok(int64_t in_feat, int64_t out_feat) {
  return in_feat >= 1 && out_feat >= 1 && in_feat <= kMaxWidth && out_feat <= kMaxWidth ? 1 : 0;
}

int dglhip_typed_linear_msg_device(int64_t num_rels, int64_t num_items, int64_t in_feat,
                                   int64_t out_feat, const int64_t* rel_ptr,
                                   const int64_t* item_ptr, const int32_t* item_rel,
                                   const int32_t* pos_row, const int64_t* pos_slot,
                                   const float* ufeat, const float* operand_scale,
                                   const float* weight, int weight_transposed, float* msg,
                                   void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DGLHIP_CHECK(num_rels >= 0 && num_items >= 0, "bad sizes");
  DGLHIP_CHECK(dglhip_typed_linear_ok(in_feat, out_feat) == 1,
               "dense typed messages of " << in_feat << " -> " << out_feat
                                          << " features: 1 to " << kMaxWidth << " each way");
  if (num_rels == 0 || num_items == 0) return 0;
  DGLHIP_CHECK(rel_ptr && item_ptr && item_rel, "null pointer argument");
  // a null per-position array (or operand): no positions, no message to store
  if (!pos_row || !pos_slot || !ufeat || !weight || !msg) return 0;
  DGLHIP_CHECK(num_items <= 0x7fffffff, "grid too large");
  const int Fi = static_cast<int>(in_feat), Fo = static_cast<int>(out_feat);
  const int tiles = (Fo + 15) / 16;
#define DGLHIP_TL(NN)                                                                          \
  hipLaunchKernelGGL((typed_linear_msg_kernel<NN>), grid_1d(num_items), dim3(256), 0, stream,  \
                     num_items, num_rels, Fi, Fo, rel_ptr, item_ptr, item_rel, pos_row,        \
                     pos_slot, ufeat, operand_scale, weight, weight_transposed, msg)
  timed_launch(stream, [&] {
    if (tiles <= 1) DGLHIP_TL(1);
    else if (tiles <= 2) DGLHIP_TL(2);
    else if (tiles <= 4) DGLHIP_TL(4);
    else if (tiles <= 8) DGLHIP_TL(8);
    else DGLHIP_TL(16);
  });
#undef DGLHIP_TL
  API_END();
}

int dglhip_typed_linear_wgrad_device(int64_t num_rels, int64_t num_items, int64_t in_feat,
                                     int64_t out_feat, const int64_t* rel_ptr,
                                     const int64_t* item_ptr, const int32_t* item_rel,
                                     int64_t num_heavy, const int32_t* heavy_rel,
                                     const int32_t* rel_src, const int32_t* rel_dst,
                                     const float* rel_norm, const float* ufeat,
                                     const float* dout, const float* dout_scale,
                                     float* dweight, float* partial, void* stream_) {
  API_BEGIN();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DGLHIP_CHECK(num_rels >= 0 && num_items >= 0 && num_heavy >= 0, "bad sizes");
  DGLHIP_CHECK(dglhip_typed_linear_ok(in_feat, out_feat) == 1,
               "dense typed weight gradient of " << in_feat << " x " << out_feat << ": 1 to "
                                                 << kMaxWidth << " each way");
  if (num_rels == 0) return 0;
  DGLHIP_CHECK(rel_ptr && item_ptr && item_rel && dweight, "null pointer argument");
  const int64_t wr = in_feat * out_feat;
  // a null per-position array (or operand): no positions, every relation's
  // gradient is zero
  if (!rel_src || !rel_dst || !ufeat || !dout) {
    HIP_CALL(hipMemsetAsync(dweight, 0, size_t(num_rels) * size_t(wr) * sizeof(float), stream));
    return 0;
  }
  DGLHIP_CHECK(num_heavy == 0 || partial, "chunked relations need their partials");
  const int Fi = static_cast<int>(in_feat), Fo = static_cast<int>(out_feat);
  const int gi = (Fi + 63) / 64, gj = (Fo + 63) / 64;
  const int64_t blocks = num_items * gi * gj;
  DGLHIP_CHECK(blocks <= 0x7fffffff, "grid too large");
  if (blocks > 0) {
    timed_launch(stream, [&] {
      hipLaunchKernelGGL(typed_linear_wgrad_kernel, grid_1d(blocks), dim3(256), 0, stream,
                         num_items, num_rels, Fi, Fo, gi, gj, rel_ptr, item_ptr, item_rel,
                         rel_src, rel_dst, rel_norm, ufeat, dout, dout_scale, dweight, partial);
    });
  }
  if (num_heavy > 0) {
    launch_typed_combine(num_heavy, wr, heavy_rel, item_ptr, partial, dweight, nullptr, stream);
  }
  API_END();
}

}  // extern "C"
