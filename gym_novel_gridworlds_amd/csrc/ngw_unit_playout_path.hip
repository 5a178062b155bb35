// ngw_unit_playout_path.hip — snapshot playout (ngw_playout.inc), the PATH form: the key of every visited state, per-pair step limits.
#include "ngw_common.inc"
#include "ngw_playout.inc"

extern "C" hipError_t ngw_playout_path_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    return playout_launch<true>(dspec, a, x, ext, lds_bytes, stream);
}
