// ngw_unit_step_dword.hip — the staged step kernels of the dword map mode.
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_step_dword) { return step_staged<NGW_MAP_DWORD>(dspec, a, feat, grid, lds_bytes, stream); }
