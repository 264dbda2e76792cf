"""R-GCN entity classification (counterpart of the reference's
examples/pytorch/rgcn/entity_classify.py on RGCNBasisLayer).

Model as the reference: a featureless input layer (nodes carry only an id, so
a message is the embedding row W[type, id_u, :]), hidden 16, then an output
layer of dense per-relation weights h[u] @ W[type], each relation's weight a
combination of ``--n-bases`` bases; inverse relations and a self-loop relation
in the graph, norm = 1 / in-degree, full-graph training on the labelled nodes.

Both layers are ``nn.RelGraphConv(regularizer="basis")``: the input layer is
one g-SpMM over the weight table, the output layer
``kernel.typed_linear_spmm`` (relation-major grouped GEMMs on the f32 matrix
instruction). No per-edge bmm and no E x in x out weight gather. ``--udf``
runs the reference's formulation (gather W[type], bmm, sum by destination) in
float64 on the same parameters, for comparison.

AIFB cannot be downloaded here: the graph is synthetic with its shape (8,285
entities, 29,043 edges of 45 relations -> 66,371 edges of 91 relations with
inverses and self-loops, 4 classes, 140 training and 36 test entities).

  python examples/rgcn/entity_classify.py --gpu 0
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..",
                                "dgl-1_amd"))
from dgl import DGLGraph  # noqa: E402
from dgl.nn.pytorch import RelGraphConv  # noqa: E402


def synthetic_entities(num_nodes=8285, num_edges=29043, num_rels=45, num_classes=4,
                       num_train=140, num_test=36, seed=0):
    """(src, dst, etype, norm, labels, train_idx, test_idx, total relations):
    power-law entity and relation frequencies; every edge with its inverse
    (relation + num_rels) and a self-loop of relation 2 * num_rels per node.
    An entity's class biases the relations of its in-edges, so the labels can
    be learnt from the structure."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, num_nodes + 1) ** 0.8
    perm = rng.permutation(num_nodes)
    s = perm[rng.choice(num_nodes, num_edges, p=p / p.sum())]
    o = perm[rng.choice(num_nodes, num_edges, p=p / p.sum())]
    cls = rng.integers(0, num_classes, num_nodes)
    q = 1.0 / np.arange(1, num_rels + 1)
    r = rng.choice(num_rels, num_edges, p=q / q.sum())
    biased = rng.random(num_edges) < 0.5
    r[biased] = (r[biased] // num_classes * num_classes + cls[o[biased]]) % num_rels
    loop = np.arange(num_nodes)
    src = np.concatenate([s, o, loop])
    dst = np.concatenate([o, s, loop])
    rel = np.concatenate([r, r + num_rels, np.full(num_nodes, 2 * num_rels)])
    deg = np.bincount(dst, minlength=num_nodes).astype(np.float32)
    norm = (1.0 / np.maximum(deg, 1)).astype(np.float32)
    picked = rng.choice(num_nodes, num_train + num_test, replace=False)
    return (src.astype(np.int64), dst.astype(np.int64), rel.astype(np.int64), norm,
            cls.astype(np.int64), picked[:num_train], picked[num_train:], 2 * num_rels + 1)


class EntityClassify(nn.Module):
    def __init__(self, num_nodes, h_dim, num_classes, num_rels, num_bases, udf):
        super(EntityClassify, self).__init__()
        kw = dict(bias=False, self_loop=False, regularizer="basis")
        self.layers = nn.ModuleList([
            RelGraphConv(num_nodes, h_dim, num_rels, num_bases, activation=F.relu, **kw),
            RelGraphConv(h_dim, num_classes, num_rels, num_bases, **kw)])
        self.udf = udf

    def forward(self, g, ids, etype, norm):
        h = ids
        for layer in self.layers:
            h = self._udf_layer(layer, g, h, etype, norm) if self.udf \
                else layer(g, h, etype, norm=norm)
        return h

    @staticmethod
    def _udf_layer(layer, g, h, etype, norm):
        """The reference's message functions (layers.py:86-98) in float64."""
        src, dst = g.edges()
        src, dst = src.to(etype.device), dst.to(etype.device)
        W = layer.relation_weights().double()
        if h.dtype == torch.int64:
            msg = W.view(-1, layer.out_feat)[etype * layer.in_feat + h[src]]
        else:
            msg = torch.bmm(h.double()[src].unsqueeze(1), W[etype]).squeeze(1)
        out = torch.zeros(norm.numel(), layer.out_feat, dtype=torch.float64, device=msg.device)
        out = out.index_add(0, dst, msg) * norm.double().unsqueeze(1)
        return layer.activation(out) if layer.activation else out


def run(args):
    device = torch.device("cpu") if args.gpu < 0 else torch.device("cuda", args.gpu)
    src, dst, rel, norm, labels, train_idx, test_idx, num_rels = synthetic_entities(
        args.num_nodes, args.num_edges, args.num_rels, args.num_classes, args.num_train,
        args.num_test, args.seed)
    torch.manual_seed(args.seed)
    g = DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)), multigraph=True)
    ids = torch.arange(args.num_nodes, device=device)
    etype = torch.from_numpy(rel).to(device)
    nrm = torch.from_numpy(norm).to(device)
    y = torch.from_numpy(labels).to(device)
    train_idx = torch.from_numpy(train_idx).to(device)
    test_idx = torch.from_numpy(test_idx).to(device)
    model = EntityClassify(args.num_nodes, args.n_hidden, args.num_classes, num_rels,
                           args.n_bases, args.udf).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.l2norm)
    dur, losses = [], []
    for epoch in range(args.n_epochs):
        if device.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.time()
        logits = model(g, ids, etype, nrm)
        loss = F.cross_entropy(logits[train_idx], y[train_idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        if device.type == "cuda":
            torch.cuda.synchronize()
        if epoch >= 3:
            dur.append(time.time() - t0)
        losses.append(float(loss.item()))
    with torch.no_grad():
        logits = model(g, ids, etype, nrm)
        acc = float((logits[test_idx].argmax(1) == y[test_idx]).float().mean())
    dur.sort()
    return {"epoch_s": sum(dur) / max(len(dur), 1),
            "epoch_s_median": dur[len(dur) // 2] if dur else 0.0,
            "epoch_s_min_max": [dur[0], dur[-1]] if dur else [],
            "graph_edges": len(src), "relations": num_rels, "losses": losses,
            "test_acc": acc, "fused": not args.udf}


def parser():
    p = argparse.ArgumentParser(description="R-GCN entity classification on the MI355X engine")
    p.add_argument("--gpu", type=int, default=-1)
    p.add_argument("--udf", action="store_true",
                   help="reference formulation (per-edge bmm + sum) in float64")
    p.add_argument("--n-hidden", type=int, default=16)
    p.add_argument("--n-bases", type=int, default=-1, help="<= 0: one basis per relation")
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--l2norm", type=float, default=0.0)
    p.add_argument("--n-epochs", type=int, default=50)
    p.add_argument("--num-nodes", type=int, default=8285)
    p.add_argument("--num-edges", type=int, default=29043)
    p.add_argument("--num-rels", type=int, default=45)
    p.add_argument("--num-classes", type=int, default=4)
    p.add_argument("--num-train", type=int, default=140)
    p.add_argument("--num-test", type=int, default=36)
    p.add_argument("--seed", type=int, default=0)
    return p


if __name__ == "__main__":
    print(run(parser().parse_args()))
