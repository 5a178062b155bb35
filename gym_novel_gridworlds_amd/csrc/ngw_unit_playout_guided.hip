// ngw_unit_playout_guided.hip — snapshot playout (ngw_playout.inc), the GUIDED form: every step's weights chosen by a key-table look-up of the state the pair is in.
#include "ngw_common.inc"
#include "ngw_playout.inc"

extern "C" hipError_t ngw_playout_guided_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    return playout_launch<true, true, true>(dspec, a, x, ext, lds_bytes, stream);
}
