"""Graph convolution modules on the engine's fused kernels.

The reference ships only GraphConvolutionLayer (python/dgl/nn/pytorch/gcn.py);
its GCN / GAT / R-GCN layers live in examples/pytorch/{gcn,gat,rgcn}. The
north star names ``nn.GraphConv`` / ``GATConv`` as the operator surface that
must drop in, so these modules package the example layers' computation (with
the later-DGL module names and arguments) on top of:

* GraphConv    : update_all(copy_src, sum) -> one g-SpMM (gcn_spmv.py:45-62)
* GATConv      : attention, dropout, per-head weighted sum and copy_edge
                 normaliser in one kernel (gat/train.py:61-96, kernel.gat_aggregate)
* GATv2Conv    : GATv2 attention over the in-edges in one kernel, one gathered
                 row per edge (later DGL's GATv2Conv, kernel.gatv2_attention)
* DotGatConv   : scaled dot-product attention over the in-edges in one kernel
                 (transformer/modules/models.py:79-86, kernel.dot_attention)
* SAGEConv     : update_all(copy_src, mean) -> g-SpMM mean
* EdgeConv     : two node products and update_all(copy_src, max) -> the max
                 g-SpMM (DGCNN's layer over a dgl.knn_graph)
* RelGraphConv : typed-edge block-diagonal g-SpMM (rgcn/layers.py:121-132), or
                 with regularizer="basis" the dense per-relation weights of
                 the basis layer on the f32 MFMA (rgcn/layers.py:52-100)
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import function as fn
from ... import kernel
from ...base import DGLError
from .linear import NodeLinear, sage_dense, bias_add

__all__ = ["GraphConv", "GATConv", "GATv2Conv", "DotGatConv", "SAGEConv", "EdgeConv",
           "RelGraphConv"]


class GraphConv(nn.Module):
    """h' = act(D_dst^-1/2 A D_src^-1/2 h W + b) (norm='both'), 'right' = mean-style
    D_dst^-1, 'none' = plain sum. Weight is applied before aggregation when
    in_feats > out_feats (fewer bytes through the g-SpMM), after otherwise."""

    def __init__(self, in_feats, out_feats, norm="both", bias=True, activation=None):
        super(GraphConv, self).__init__()
        if norm not in ("both", "right", "none"):
            raise DGLError("Invalid norm %s" % norm)
        self.in_feats, self.out_feats, self.norm = in_feats, out_feats, norm
        self.weight = nn.Parameter(torch.Tensor(in_feats, out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats)) if bias else None
        self.activation = activation
        nn.init.xavier_uniform_(self.weight)

    def forward(self, g, feat):
        dev = feat.device
        if self.norm == "both":
            src_norm = g.out_degrees().float().clamp(min=1).pow(-0.5).to(dev).unsqueeze(1)
            feat = feat * src_norm
        if self.in_feats > self.out_feats:
            feat = feat @ self.weight
        g.ndata["_gc_h"] = feat
        g.update_all(fn.copy_src("_gc_h", "_gc_m"), fn.sum("_gc_m", "_gc_h"))
        rst = g.ndata.pop("_gc_h")
        if self.in_feats <= self.out_feats:
            rst = rst @ self.weight
        if self.norm != "none":
            deg = g.in_degrees().float().clamp(min=1).to(dev).unsqueeze(1)
            rst = rst * (deg.pow(-0.5) if self.norm == "both" else 1.0 / deg)
        if self.bias is not None:
            rst = bias_add(rst, self.bias)
        return self.activation(rst) if self.activation else rst


class GATConv(nn.Module):
    """Multi-head graph attention; returns (N, num_heads, out_feats)."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0.,
                 negative_slope=0.2, residual=False, activation=None):
        super(GATConv, self).__init__()
        self.num_heads, self.out_feats = num_heads, out_feats
        self.fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
        self.attn_l = nn.Parameter(torch.Tensor(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.Tensor(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop) if feat_drop else None
        self.attn_drop = nn.Dropout(attn_drop) if attn_drop else None
        self.negative_slope = negative_slope
        self.res_fc = None
        if residual:
            self.res_fc = nn.Identity() if in_feats == num_heads * out_feats else \
                nn.Linear(in_feats, num_heads * out_feats, bias=False)
        self.activation = activation
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, g, feat):
        h = self.feat_drop(feat) if self.feat_drop is not None else feat
        ft = self.fc(h).view(-1, self.num_heads, self.out_feats)
        # (ft * attn).sum(-1) in the library's association (kernel.gat_logits):
        # with the same ft, gat_aggregate's blocked forward then recomputes
        # each source's logit from its gathered row instead of reading el
        el, er = kernel.gat_logits(ft, self.attn_l, self.attn_r)  # N x H x 1
        adj = g.sparse_adjacency(feat.device)
        # attention, its dropout, the weighted sum and the normaliser in one
        # kernel (kernel.gat_aggregate); the attention is kept, in CSR slot
        # order, only for the backward. Same per-element arithmetic as the
        # attention g-SDDMM + u_mul_e + copy_e g-SpMMs (bit for bit without
        # dropout); the dropout mask is the kernel's counter hash
        ft_sum, z = kernel.gat_aggregate(
            adj, ft, el, er, self.negative_slope, clamp=(-float("inf"), float("inf")),
            attn_drop=self.attn_drop.p if self.attn_drop is not None else 0.0,
            training=self.training)
        rst = ft_sum / z.clamp(min=1e-20)
        if self.res_fc is not None:
            rst = rst + self.res_fc(h).view(-1, self.num_heads, self.out_feats)
        return self.activation(rst) if self.activation else rst


class GATv2Conv(nn.Module):
    """Multi-head GATv2 attention (Brody et al.): e = <attn, leaky_relu(W_src
    h_u + W_dst h_v)>, softmax over v's in-edges, the sum of W_src h_u
    weighted by it; returns (N, num_heads, out_feats). ``share_weights``: one
    projection for both sides. The attention, its softmax and the sum run in
    one kernel (kernel.gatv2_attention) unless dropout on the attention is
    active (``attn_drop`` > 0 in training), which runs the composition."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0.,
                 negative_slope=0.2, residual=False, activation=None, bias=True,
                 share_weights=False):
        super(GATv2Conv, self).__init__()
        self.num_heads, self.out_feats = num_heads, out_feats
        self.fc_src = nn.Linear(in_feats, num_heads * out_feats, bias=bias)
        self.fc_dst = self.fc_src if share_weights else \
            nn.Linear(in_feats, num_heads * out_feats, bias=bias)
        self.attn = nn.Parameter(torch.Tensor(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop) if feat_drop else None
        self.attn_drop = float(attn_drop)
        self.negative_slope = negative_slope
        self.res_fc = None
        if residual:
            self.res_fc = nn.Identity() if in_feats == num_heads * out_feats else \
                nn.Linear(in_feats, num_heads * out_feats, bias=bias)
        self.activation = activation
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc_src.weight, gain=gain)
        nn.init.xavier_normal_(self.fc_dst.weight, gain=gain)
        nn.init.xavier_normal_(self.attn, gain=gain)
        for fc in (self.fc_src, self.fc_dst):
            if fc.bias is not None:
                nn.init.zeros_(fc.bias)

    def forward(self, g, feat):
        h = self.feat_drop(feat) if self.feat_drop is not None else feat
        fs = self.fc_src(h).view(-1, self.num_heads, self.out_feats)
        fd = fs if self.fc_dst is self.fc_src else \
            self.fc_dst(h).view(-1, self.num_heads, self.out_feats)
        rst = kernel.gatv2_attention(g.sparse_adjacency(feat.device), fs, fd, self.attn,
                                     self.negative_slope,
                                     attn_drop=self.attn_drop if self.training else 0.0)
        if self.res_fc is not None:
            rst = rst + self.res_fc(h).view(-1, self.num_heads, self.out_feats)
        return self.activation(rst) if self.activation else rst


class DotGatConv(nn.Module):
    """Multi-head dot-product graph attention: one projection to num_heads *
    out_feats, each node's projected row its query, key and value over its
    in-edges, scores scaled by out_feats ** -0.5; returns (N, num_heads,
    out_feats)."""

    def __init__(self, in_feats, out_feats, num_heads):
        super(DotGatConv, self).__init__()
        self.num_heads, self.out_feats = num_heads, out_feats
        self.fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
        nn.init.xavier_normal_(self.fc.weight, gain=nn.init.calculate_gain("relu"))

    def forward(self, g, feat):
        ft = self.fc(feat).view(-1, self.num_heads, self.out_feats)
        return kernel.dot_attention(g.sparse_adjacency(feat.device), ft, ft, ft,
                                    scale=self.out_feats ** -0.5)


class SAGEConv(nn.Module):
    """GraphSAGE with the mean aggregator: act(W_self h + W_neigh mean_{u->v} h_u)."""

    def __init__(self, in_feats, out_feats, bias=True, activation=None):
        super(SAGEConv, self).__init__()
        # NodeLinear: nn.Linear whose backward reductions over the node
        # dimension are chunked (split-K weight gradient, chunked bias sum)
        self.fc_self = NodeLinear(in_feats, out_feats, bias=bias)
        self.fc_neigh = NodeLinear(in_feats, out_feats, bias=False)
        self.activation = activation

    def forward(self, g, feat):
        def aggregate(x):
            g.ndata["_sage_h"] = x
            g.update_all(fn.copy_src("_sage_h", "_sage_m"), fn.mean("_sage_m", "_sage_n"))
            g.ndata.pop("_sage_h")
            return g.ndata.pop("_sage_n")
        # fc_neigh (no bias) commutes with the mean: the narrower side is
        # aggregated; both products and their sum fused (linear.sage_dense)
        return sage_dense(feat, aggregate, self.fc_self, self.fc_neigh, self.activation)


class EdgeConv(nn.Module):
    """The EdgeConv layer of DGCNN (Wang et al., "Dynamic Graph CNN for
    Learning on Point Clouds"): h_v = max_{u->v} Theta (x_u - x_v) + Phi x_v,
    per output channel; a node without in-edges gets Phi x_v - Theta x_v + 0.
    x_v leaves the max, h_v = max_u (Theta x_u) + (Phi - Theta) x_v: two node
    products and one copy_u + max g-SpMM, no per-edge product."""

    def __init__(self, in_feats, out_feats, bias=True):
        super(EdgeConv, self).__init__()
        self.theta = NodeLinear(in_feats, out_feats, bias=False)
        self.phi = NodeLinear(in_feats, out_feats, bias=bias)

    def forward(self, g, feat):
        t = self.theta(feat)
        g.ndata["_ec_t"] = t
        g.update_all(fn.copy_src("_ec_t", "_ec_m"), fn.max("_ec_m", "_ec_h"))
        g.ndata.pop("_ec_t")
        return g.ndata.pop("_ec_h") + (self.phi(feat) - t)


class RelGraphConv(nn.Module):
    """R-GCN layer, h' = act(norm * sum_{e=(u->v)} enorm_e W[etype_e] h_u + h W_loop + b).

    regularizer="bdd" (the default): block-diagonal relation weights of
    num_bases blocks, ``weight`` (num_rels, num_bases, in/num_bases,
    out/num_bases), through kernel.typed_block_spmm.

    regularizer="basis" (the reference's RGCNBasisLayer, rgcn/layers.py:
    52-100): every relation a dense in_feat x out_feat weight composed from
    ``weight`` (num_bases, in_feat, out_feat) by ``w_comp`` (num_rels,
    num_bases; present only when num_bases < num_rels, and a num_bases <= 0 or
    > num_rels means num_rels), through kernel.typed_linear_spmm. With
    ``feat`` an int64 tensor of node ids (the featureless input layer) the
    message is the row W[etype_e, feat[u], :]: one g-SpMM over the table
    W.view(num_rels * in_feat, out_feat), no per-edge product."""

    def __init__(self, in_feat, out_feat, num_rels, num_bases, bias=True, activation=None,
                 self_loop=True, dropout=0.0, regularizer="bdd"):
        super(RelGraphConv, self).__init__()
        if regularizer not in ("bdd", "basis"):
            raise DGLError("regularizer must be 'bdd' or 'basis', got %r" % (regularizer,))
        self.regularizer = regularizer
        self.in_feat, self.out_feat, self.num_rels = in_feat, out_feat, num_rels
        gain = nn.init.calculate_gain("relu")
        if regularizer == "basis":
            if num_bases <= 0 or num_bases > num_rels:
                num_bases = num_rels
            self.weight = nn.Parameter(torch.Tensor(num_bases, in_feat, out_feat))
            nn.init.xavier_uniform_(self.weight, gain=gain)
            if num_bases < num_rels:
                self.w_comp = nn.Parameter(torch.Tensor(num_rels, num_bases))
                nn.init.xavier_uniform_(self.w_comp, gain=gain)
            else:
                self.w_comp = None
        else:
            if in_feat % num_bases or out_feat % num_bases:
                raise DGLError("in/out features must be divisible by num_bases")
            self.weight = nn.Parameter(torch.Tensor(num_rels, num_bases, in_feat // num_bases,
                                                    out_feat // num_bases))
            nn.init.xavier_uniform_(self.weight, gain=gain)
        self.num_bases = num_bases
        self.loop_weight = nn.Parameter(torch.Tensor(in_feat, out_feat)) if self_loop else None
        if self_loop:
            nn.init.xavier_uniform_(self.loop_weight, gain=gain)
        self.bias = nn.Parameter(torch.zeros(out_feat)) if bias else None
        self.activation = activation
        self.dropout = nn.Dropout(dropout) if dropout else None

    def relation_weights(self):
        """(num_rels, in_feat, out_feat): the basis layer's dense weights,
        composed by torch so that autograd carries dW to weight and w_comp."""
        if self.w_comp is None:
            return self.weight
        return (self.w_comp @ self.weight.view(self.num_bases, -1)).view(
            self.num_rels, self.in_feat, self.out_feat)

    def _table_adj(self, adj, ids, etype):
        """The featureless layer's adjacency, rows = destinations and column
        of edge e = etype[e] * in_feat + ids[src_e] (a row of the table
        W.view(num_rels * in_feat, out_feat)); cached on ``adj`` for these
        etype and ids tensors at their versions, as the relation grouping is."""
        key = (etype.data_ptr(), etype.numel(), etype._version, ids.data_ptr(), ids.numel(),
               ids._version, self.in_feat)
        hit = getattr(adj, "_rel_table", None)
        if hit is None or hit[0] != key:
            dst, src = kernel.coo_of(adj.fwd)
            col = etype * self.in_feat + ids.index_select(0, src)
            table = kernel.from_coo(adj.fwd.num_rows, self.num_rels * self.in_feat, dst, col,
                                    kernel.ORDER_EID, ids.device)
            # (the keyed tensors are held: their memory is not reused meanwhile)
            hit = adj._rel_table = (key, table, etype, ids)
        return hit[1]

    def forward(self, g, feat, etype, norm=None, enorm=None):
        adj = g.sparse_adjacency(feat.device)
        featureless = feat.dtype == torch.int64
        if self.regularizer == "bdd":
            rst = kernel.typed_block_spmm(adj, feat, self.weight, etype, enorm)
            if norm is not None:
                rst = rst * norm.reshape(-1, 1)
        elif featureless:
            et = torch.as_tensor(etype).to(device=feat.device, dtype=torch.int64).reshape(-1)
            # (ids out of the table's range are refused where the adjacency over
            # them is built, once per etype and ids: from_coo checks its columns)
            table =self.relation_weights().reshape(self.num_rels * self.in_feat, self.out_feat)
            tadj = self._table_adj(adj.to(feat.device), feat.reshape(-1), et)
            if enorm is None:
                rst = kernel.gspmm(tadj, kernel.MSG_COPY_U, kernel.RED_SUM, table)
            else:
                rst = kernel.gspmm(tadj, kernel.MSG_U_MUL_E, kernel.RED_SUM, table,
                                   enorm.detach().reshape(-1, 1))
            if norm is not None:
                rst = rst * norm.reshape(-1, 1)
        else:
            rst = kernel.typed_linear_spmm(adj, feat, self.relation_weights(), etype, enorm,
                                           row_scale=None if norm is None else norm.reshape(-1))
        if self.loop_weight is not None:
            loop = self.loop_weight.index_select(0, feat.reshape(-1)) if featureless \
                else feat @ self.loop_weight
            rst = rst + (self.dropout(loop) if self.dropout is not None else loop)
        if self.bias is not None:
            rst = rst + self.bias
        return self.activation(rst) if self.activation else rst
