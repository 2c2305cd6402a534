// The masked instantiations of the query-resident flat scan kernels (cos_flat_search_masked_batch) and their launchers,
// launch_flat_scan_masked / launch_flat_scan_u8_masked: kernels_scan.hip compiled a second time for its MASKED half, beside the
// unmasked one (same flags: -mllvm -amdgpu-mfma-vgpr-form=1).
#define COS_SCAN_MASKED_TU 1
#include "kernels_scan.hip"
