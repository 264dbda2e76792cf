"""Contributed modules (python/dgl/contrib): ``sampling``."""
from __future__ import absolute_import

from . import sampling  # noqa: F401
