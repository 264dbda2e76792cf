"""The GraphSAGE example's opt-in ``--sample`` mode: mini-batches over sampled
neighbourhoods (dgl.contrib.sampling.NeighborSampler)."""
import pytest
import torch

from conftest import load_example

sage_train = load_example("graphsage/train.py", "sage_train_sampling")


def _gpu_arg(device):
    return "0" if device == "cuda" else "-1"


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_graphsage_sampled_two_batches(device):
    args = sage_train.parser().parse_args(
        ["--graph", "rmat", "--rmat-scale", "8", "--in-feats", "16", "--n-classes", "5",
         "--n-hidden", "16", "--gpu", _gpu_arg(device), "--sample", "4", "--batch-size", "32",
         "--max-batches", "2", "--n-epochs", "1"])
    res = sage_train.run(args)
    assert res["batches"] == 2 and res["sample"] == 4
    assert len(res["losses"]) == 2 and all(torch.isfinite(torch.tensor(res["losses"])))
    # two hops at fan-out 4 from 32 seeds: at most 32 * 4 + 32 * 4 * 4 edges a batch
    assert 0 < res["sampled_edges"] <= 2 * (32 * 4 + 32 * 16)


def test_sample_mode_is_off_by_default():
    args = sage_train.parser().parse_args([])
    assert args.sample == 0
