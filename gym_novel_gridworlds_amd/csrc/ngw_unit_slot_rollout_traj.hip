// ngw_unit_slot_rollout_traj.hip — snapshot rollout (ngw_slot_rollout.inc), the TRAJ form: per-step rewards and LidarInFront rows beside the PATH form's keys and limits.
#include "ngw_common.inc"
#include "ngw_slot_rollout.inc"

extern "C" hipError_t ngw_slot_rollout_traj_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwSlotRollout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    return slot_rollout_launch<true, true>(dspec, a, x, ext, lds_bytes, stream);
}
