"""dglhip._CAPI_SegmentReduce through the PackedFunc registry on host
tensors: known integer answers (exact in float32), as
test_abi.test_registry_call_host_csr_and_spmm does for the g-SpMM."""
import pytest
import torch

import dgl
from dgl import _ffi, kernel
from dgl.base import DGLError


def test_registry_call_segment_reduce_host():
    assert "dglhip._CAPI_SegmentReduce" in dgl.list_global_func_names()
    x = torch.tensor([[1, 2], [3, 4], [5, 6], [7, -7], [9, 10]], dtype=torch.float32)
    off = torch.tensor([0, 2, 2, 5], dtype=torch.int64)
    y = torch.empty(3, 2)
    _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_SUM, off, x, None, y, None, None,
                     None)
    assert y.tolist() == [[4, 6], [0, 0], [21, 9]]
    w = torch.tensor([2, 1, 1, 1, 2], dtype=torch.float32)
    wsum = torch.empty(3)
    _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_SUM, off, x, w, y, wsum, None, None)
    assert y.tolist() == [[5, 8], [0, 0], [30, 19]] and wsum.tolist() == [3, 0, 4]
    _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_MEAN, off, x, None, y, None, None,
                     None)
    assert y.tolist() == [[2, 3], [0, 0], [7, 3]]
    arg = torch.empty(3, 2, dtype=torch.int64)
    _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_MAX, off, x, None, y, None, arg,
                     None)
    assert y.tolist() == [[3, 4], [0, 0], [9, 10]]
    assert arg.tolist() == [[1, 1], [-1, -1], [4, 4]]
    # the leading columns of wider rows are read in place
    wide = torch.arange(15, dtype=torch.float32).view(5, 3)
    _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_SUM, off, wide[:, :2], None, y,
                     None, None, None)
    assert y.tolist() == [[3, 5], [0, 0], [27, 30]]
    with pytest.raises(DGLError):  # offsets that do not end at the row count
        _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_SUM,
                         torch.tensor([0, 2, 2, 4]), x, None, y, None, None, None)
    with pytest.raises(DGLError):  # wrong dtype is rejected, not reinterpreted
        _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_SUM, off.int(), x, None, y,
                         None, None, None)
    with pytest.raises(DGLError):  # max takes no weight
        _ffi.call_packed("dglhip._CAPI_SegmentReduce", kernel.RED_MAX, off, x, w, y, None, arg,
                         None)
