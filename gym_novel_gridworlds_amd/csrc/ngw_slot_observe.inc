// ngw_slot_observe.inc - observations of saved states (a unit of its own; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lidar_march.inc"     // lidar_epilogue: the row builder
#include "ngw_lean.inc"            // lane_mask, lean_gather_lane
#include "ngw_expand.inc"          // expand_rows_in: the gathered stage-in

namespace {
//
// The read-only side of a node pool: the LidarInFront row, the AgentMap window and the action mask of row slots[j] of a snapshot go to row j of
// the caller's buffer.  Nothing but those rows and the sticky error flags is stored, and nothing here restates a game rule or an observation: the
// lidar row is lidar_epilogue's, the mask is lane_mask's, the window is ngw_agent_view_kernel's gather.
//
// Every kernel treats an index the same way: lane / pair j reads slots[j] (NULL: j), checks it against the row count, and CLAMPS a bad one to
// row 0 - loads stay unconditional on the clamped index, nothing is ever addressed with the bad one -, marks the pair not live (its output row
// is zeros) and raises NGW_F_BAD_INDEX.

// ---------------------------------------------------------------- LidarInFront rows
// ngw_lidar_kernel with ngw_expand_kernel's stage-in.  One work-group is one wave: 64 consecutive pairs.  Lane l gathers its slot's pose into
// registers; the wave brings the 64 map and inventory rows into the STAND-ALONE lidar launch's LDS layout (guard | maps, row l at l * MS | guard |
// inventory rows, row l at l * KP: ngw_lidar_configure's lidar_proto) with expand_move_row, 16 lanes per row, four rows per round, the row index of
// a round's row out of its owner's register with ds_bpermute; then lidar_epilogue builds the 64 rows in its tile and stores the tile to rows
// 64 * blockIdx.x .. of a.lout = the caller's buffer (which is `count` rounded up to 64 rows long: the tile store stays whole; a lane that is
// not live leaves its zeroed tile row).
template <int VEC>
__global__ void __launch_bounds__(NGW_EPB) ngw_slot_lidar_kernel(const NgwLaunch a, const NgwSlotObs x) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S = a.S, K = a.K, S2 = a.S2;
    const bool inside = pair < (int64_t)x.count;
    int si = 0;
    if (inside) si = x.slots ? x.slots[pair] : (int)pair;
    const bool ok = inside && (uint32_t)si < (uint32_t)x.rows;
    const bool bad = inside && !ok && si != NGW_IDX_NONE;                          // (NGW_IDX_NONE: a pair that is not there)
    if (__ballot(ok) == 0) {                                                       // no live pair in this wave - a frontier's padding: a tile of zeros, nothing to stage
        const int npc = 4 * a.l_rb;                                                // 64 rows = 4 * rb pieces of 16 B
        GLOBAL_AS u32x4* g4 = (GLOBAL_AS u32x4*)(reinterpret_cast<char*>(a.lout) + (uint64_t)blockIdx.x * (uint32_t)(EPB * a.l_rb));
        for (int p = (int)tid; p < npc; p += EPB) g4[p] = u32x4{0u, 0u, 0u, 0u};
        if (bad) atomicOr(x.flags, NGW_F_BAD_INDEX);
        return;
    }
    const int sic = ok ? si : 0;
    uint32_t it = 0;
    if (tid < LIDAR_ITEM_DW) it = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[tid];
    const int2 rc = reinterpret_cast<const int2*>(x.src.loc)[sic];
    const int f = x.src.facing[sic];
    uint32_t* const lds_map = lds + a.off_map;
    int32_t* const lds_inv = reinterpret_cast<int32_t*>(lds + a.off_inv);
    if (tid < LIDAR_ITEM_DW) lds[a.off_litem + tid] = it;
    expand_rows_in<VEC>(x.src, sic, lds_map, lds_inv, a.MS >> 2, a.KP, S2, K, tid);
    if (bad) atomicOr(x.flags, NGW_F_BAD_INDEX);
    const int8_t* mp = reinterpret_cast<const int8_t*>(lds_map) + tid * a.MS;
    lidar_epilogue(a, lds, tid, ok, mp + rc.x * S + rc.y, f, lds_inv + tid * a.KP);   // (its first barrier makes the staging visible)
}

// ---------------------------------------------------------------- action masks
// ngw_mask_kernel over gathered lanes (lean_gather_lane, ngw_mask.inc): one lane per pair, every lane stays active through lane_mask (its walk is wave-uniform), a lane that is not
// live stores 0, stores are bounded by count.
template <bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_slot_mask_kernel(const NgwDevSpec* __restrict__ dspec, const NgwSlotObs x, int S, int K, uint64_t* __restrict__ out) {
    __shared__ int32_t inv_lds[NGW_EPB * (NGW_MAX_ITEMS | 1)];
    const int64_t pair = (int64_t)blockIdx.x * EPB + threadIdx.x;
    const bool inside = pair < (int64_t)x.count;
    int si = 0;
    if (inside) si = x.slots ? x.slots[pair] : (int)pair;
    const bool ok = inside && (uint32_t)si < (uint32_t)x.rows;
    const LeanLane l = lean_gather_lane(x.src, ok ? si : 0, ok, S, K, inv_lds);
    auto cell_at = [&](int cell) -> int { return (int)ldg<int8_t>(l.bmap, l.mapoff + (uint32_t)cell); };
    const uint64_t mask = lane_mask<EXT>(dspec, S, K, l.r, l.c, l.f, l.sel, l.inv, cell_at);
    if (inside) out[pair] = l.live ? mask : 0ull;
    if (inside && !ok && si != NGW_IDX_NONE) atomicOr(x.flags, NGW_F_BAD_INDEX);   // (NGW_IDX_NONE: a pair that is not there)
}

// ---------------------------------------------------------------- AgentMap windows, facing, inventory
// ngw_agent_view_kernel with one indirection: output row j is the window of slot slots[j].  Slice blockIdx.y == 0: one lane produces 4 consecutive
// output bytes (one coalesced dword store; the last dword's bytes past the end are 0); a dword lies in at most two rows (W * W >= 9), whose slots
// and agent cells the lane reads up front.  Slice 1 gathers facing and inventory with a grid-stride loop, and is where a bad index raises the
// flag (once per pair, whichever outputs were asked for).
__global__ __launch_bounds__(256) void ngw_slot_view_kernel(const NgwSlotObs x) {
    const uint32_t stride = gridDim.x * 256u, t0 = blockIdx.x * 256u + threadIdx.x;
    const uint32_t count = (uint32_t)x.count;
    if (blockIdx.y == 1) {
        const uint32_t K = (uint32_t)x.K;
        for (uint32_t j = t0; j < count; j += stride) {
            const int si = x.slots ? x.slots[j] : (int)j;
            const bool ok = (uint32_t)si < (uint32_t)x.rows;
            if (!ok && si != NGW_IDX_NONE) atomicOr(x.flags, NGW_F_BAD_INDEX);     // (NGW_IDX_NONE: a pair that is not there)
            const int v = x.src.facing[ok ? si : 0];
            if (x.facing) x.facing[j] = ok ? v : 0;
        }
        if (x.inv)
            for (uint64_t i = t0; i < (uint64_t)count * K; i += stride) {
                const uint32_t j = (uint32_t)(i / K), k = (uint32_t)(i - (uint64_t)j * K);
                const int si = x.slots ? x.slots[j] : (int)j;
                const bool ok = (uint32_t)si < (uint32_t)x.rows;
                const int v = x.src.inv[(size_t)(ok ? si : 0) * K + k];
                x.inv[i] = ok ? v : 0;
            }
        return;
    }
    if (!x.view) return;
    const int S = x.S, V = x.V;
    const uint32_t W = 2u * (uint32_t)V + 1u, WW = W * W;
    for (uint32_t t = t0; t < x.n_dwords; t += stride) {
        const uint32_t idx = t * 4u;
        const uint32_t e0 = idx / WW;                    // one full division per lane; the rest are small-operand magics
        uint32_t rem = idx - e0 * WW;
        // the two rows this dword can lie in (indices clamped into the list: a row past the end contributes zeros)
        int slot[2], ar[2], ac[2];
        bool live[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t e = e0 + (uint32_t)i;
            const uint32_t ec = min(e, count - 1u);
            const int si = x.slots ? x.slots[ec] : (int)ec;
            live[i] = e < count && (uint32_t)si < (uint32_t)x.rows;
            slot[i] = live[i] ? si : 0;
            const int2 rc = reinterpret_cast<const int2*>(x.src.loc)[slot[i]];
            ar[i] = rc.x; ac[i] = rc.y;
        }
        int cur = 0;
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = __umulhi(rem, x.magicW), c = rem - r * W;
            const int mr = (cur ? ar[1] : ar[0]) + (int)r - V, mc = (cur ? ac[1] : ac[0]) + (int)c - V;
            const bool lv = cur ? live[1] : live[0];
            const int sl = cur ? slot[1] : slot[0];
            uint32_t v = 0;
            if (lv && (unsigned)mr < (unsigned)S && (unsigned)mc < (unsigned)S) v = (uint8_t)x.src.map[(size_t)sl * (size_t)(S * S) + mr * S + mc];
            word |= v << (8 * j);
            if (++rem == WW) { rem = 0; cur = 1; }
        }
        x.view[t] = word;
    }
}

}  // namespace
