// The item-row search and the argument checks of compact.h.
#include "compact.h"

namespace dglhip {

namespace {

__global__ __launch_bounds__(256) void item_rows_kernel(int64_t num_rows, int64_t bound,
                                                        const int64_t* __restrict__ item_ptr,
                                                        int32_t* __restrict__ item_row) {
  const int64_t j = block_linear() * blockDim.x + threadIdx.x;
  if (j >= bound) return;
  item_row[j] = static_cast<int32_t>(last_le(item_ptr, j, 0, num_rows));
}

}  // namespace

void launch_item_rows(int64_t num_rows, int64_t bound, const int64_t* item_ptr,
                      int32_t* item_row, hipStream_t stream) {
  hipLaunchKernelGGL(item_rows_kernel, grid_1d((bound + 255) / 256), dim3(256), 0, stream,
                     num_rows, bound, item_ptr, item_row);
}

void check_workspace(int64_t workspace_bytes, int64_t needed) {
  DGLHIP_CHECK(workspace_bytes >= needed, "workspace of " << workspace_bytes << " B, "
                                                          << needed << " needed");
}

void check_not_capturing(hipStream_t stream, const char* why) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_CALL(hipStreamIsCapturing(stream, &cap));
  DGLHIP_CHECK(cap == hipStreamCaptureStatusNone, why);
}

}  // namespace dglhip
