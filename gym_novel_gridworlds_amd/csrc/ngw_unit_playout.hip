// ngw_unit_playout.hip — snapshot playout (ngw_playout.inc), the plain form.
#include "ngw_common.inc"
#include "ngw_playout.inc"

extern "C" hipError_t ngw_playout_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    return playout_launch<false>(dspec, a, x, ext, lds_bytes, stream);
}
