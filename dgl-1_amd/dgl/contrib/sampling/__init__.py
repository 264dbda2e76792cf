"""Subgraph samplers (python/dgl/contrib/sampling)."""
from __future__ import absolute_import

from .sampler import NeighborSampler  # noqa: F401
