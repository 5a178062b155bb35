// ngw_unit_slot_rollout_path.hip — snapshot rollout (ngw_slot_rollout.inc), the PATH form: the key of every visited state, per-pair step limits.
#include "ngw_common.inc"
#include "ngw_slot_rollout.inc"

extern "C" hipError_t ngw_slot_rollout_path_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwSlotRollout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    return slot_rollout_launch<true>(dspec, a, x, ext, lds_bytes, stream);
}
