// ngw_unit_step_wire_boards.hip — the in-place step kernels with the host write-through and the bit-row lidar.
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_step_wire_boards) { return step_boards<true>(dspec, a, feat, grid, lds_bytes, stream); }
