// ngw_unit_rollout_byte.hip — the fused rollout kernels of the byte map mode (odd map sizes).
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_rollout_byte) { return rollout<NGW_MAP_BYTE>(dspec, a, feat, grid, lds_bytes, stream); }
