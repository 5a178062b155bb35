// ngw_unit_rollout_dword.hip — the fused rollout kernels of the dword map mode.
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_rollout_dword) { return rollout<NGW_MAP_DWORD>(dspec, a, feat, grid, lds_bytes, stream); }
