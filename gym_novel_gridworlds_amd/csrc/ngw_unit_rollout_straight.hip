// ngw_unit_rollout_straight.hip — the fused rollout kernels of the straight map mode.
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_rollout_straight) { return rollout<NGW_MAP_STRAIGHT>(dspec, a, feat, grid, lds_bytes, stream); }
