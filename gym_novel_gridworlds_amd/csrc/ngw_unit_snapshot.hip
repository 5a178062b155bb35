// ngw_unit_snapshot.hip — device-side snapshots (ngw_snapshot.inc).
#include "ngw_common.inc"
#include "ngw_snapshot.inc"

// p->count rows from p->src to p->dst through the index lists
extern "C" hipError_t ngw_snapshot_launch(const NgwSnap* p, hipStream_t stream) {
    if (p->count <= 0 || p->S2 < 9 || p->S2 > NGW_MAX_MAP_SIZE * NGW_MAX_MAP_SIZE || p->K < 1 || p->K > NGW_MAX_ITEMS || p->src_rows < 1 ||
        p->dst_rows < 1 || !p->flags)
        return hipErrorInvalidValue;
    constexpr int rows = NGW_SNAP_BLOCK / NGW_SNAP_GROUP;
    const dim3 grid((unsigned)((p->count + rows - 1) / rows)), block(NGW_SNAP_BLOCK);
    if (p->S2 % 16 == 0) return launch_kernel<ngw_snapshot_kernel<16>>(grid, block, 0, stream, *p);
    if (p->S2 % 4 == 0) return launch_kernel<ngw_snapshot_kernel<4>>(grid, block, 0, stream, *p);
    return launch_kernel<ngw_snapshot_kernel<1>>(grid, block, 0, stream, *p);
}
