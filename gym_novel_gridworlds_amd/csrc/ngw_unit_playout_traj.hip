// ngw_unit_playout_traj.hip — snapshot playout (ngw_playout.inc), the TRAJ form: per-step rewards, mask words and LidarInFront rows beside the PATH form's keys and limits.
#include "ngw_common.inc"
#include "ngw_playout.inc"

extern "C" hipError_t ngw_playout_traj_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    return playout_launch<true, true>(dspec, a, x, ext, lds_bytes, stream);
}
