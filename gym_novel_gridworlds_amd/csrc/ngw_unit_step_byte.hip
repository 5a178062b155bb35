// ngw_unit_step_byte.hip — the staged step kernels of the byte map mode (odd map sizes).
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_step_byte) { return step_staged<NGW_MAP_BYTE>(dspec, a, feat, grid, lds_bytes, stream); }
