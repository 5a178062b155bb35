// ngw_unit_slot_observe.hip — observations of saved states (ngw_slot_observe.inc): lidar rows, agent views, action masks.
#include "ngw_common.inc"
#include "ngw_slot_observe.inc"

// the lidar rows: a = the stand-alone lidar launch's layout with a.lout = the caller's rows; one wave per 64 pairs
extern "C" hipError_t ngw_slot_lidar_launch(const NgwLaunch* a, const NgwSlotObs* x, size_t lds_bytes, hipStream_t stream) {
    if (x->count <= 0 || x->rows < 1 || a->S < 3 || a->S > NGW_MAX_MAP_SIZE || a->K < 1 || a->K > NGW_MAX_ITEMS || a->MS < a->S2 || (a->MS & 3) || !x->flags ||
        !x->src.map || !a->lout || !a->lcfg || a->l_rb < 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks_for(x->count)), block(NGW_EPB);
    return with_row_piece(a->S2, [&](auto V) { return launch_kernel<ngw_slot_lidar_kernel<decltype(V)::value>>(grid, block, lds_bytes, stream, *a, *x); });
}

// the action masks: [count] words at `out`
extern "C" hipError_t ngw_slot_mask_launch(const NgwDevSpec* dspec, const NgwSlotObs* x, int S, int K, int ext, uint64_t* out, hipStream_t stream) {
    if (x->count <= 0 || x->rows < 1 || S < 3 || S > NGW_MAX_MAP_SIZE || K < 1 || K > NGW_MAX_ITEMS || !x->flags || !x->src.map || !out) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks_for(x->count)), block(NGW_EPB);
    return with_flag(ext != 0, [&](auto E) { return launch_kernel<ngw_slot_mask_kernel<decltype(E)::value>>(grid, block, 0, stream, dspec, *x, S, K, out); });
}

// the agent views (slice 0) and facing / inventory (slice 1); magicW is set here
extern "C" hipError_t ngw_slot_view_launch(const NgwSlotObs* x, hipStream_t stream) {
    if (x->count <= 0 || x->rows < 1 || x->S < 3 || x->S > NGW_MAX_MAP_SIZE || x->K < 1 || x->K > NGW_MAX_ITEMS || x->V < 1 || x->V > 127 || !x->flags ||
        !x->src.map || (!x->view && !x->facing && !x->inv))
        return hipErrorInvalidValue;
    NgwSlotObs p = *x;
    const uint32_t W = 2u * (uint32_t)p.V + 1u;
    p.magicW = (uint32_t)((0x100000000ull + W - 1) / W);                  // exact for operands < W * W
    uint64_t most = (uint64_t)p.count * (p.inv ? (uint64_t)p.K : 1u);
    if (p.view && p.n_dwords > most) most = p.n_dwords;
    uint64_t blocks = (most + 255u) / 256u;
    if (blocks > (1u << 20)) blocks = 1u << 20;                           // (both slices are grid-stride loops)
    return launch_kernel<ngw_slot_view_kernel>(dim3((unsigned)blocks, 2u), dim3(256), 0, stream, p);
}
