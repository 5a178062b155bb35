// ngw_expand.inc - snapshot expand (a unit of its own; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // lean_body and its table fetches

namespace {
//
// Pair j of a call: the parent is row si[j] of the source set (the state slab, or a snapshot), the child is the parent stepped ONCE with
// actions[j] by the rules of ngw_step_device, and goes to row di[j] of the destination snapshot as the step leaves it BEFORE any reset: no
// reset path is in this kernel (no new_episode_inline, no Philox, no prepared row), the episode counter is the parent's.  Nothing but the
// destination rows, the three report arrays and the sticky error flags is stored.  Nothing here restates a game rule: the step is lean_body.
//
// Shape: ngw_plans_lean's with a gathered stage-in and a scattered stage-out.  One work-group is one wave: 64 consecutive pairs.
//   1. Lane l reads pair l - parent, destination, action - checks both indices against the row counts of their sets, and gathers its parent's
//      pose, selected item, step count and episode counter into registers.  A pair with a bad index (and a lane past `count`) raises
//      NGW_F_BAD_INDEX (past `count`: nothing), stores nothing, and stages row 0 of the source instead - loads stay unconditional on a clamped
//      index, nothing is ever addressed with the bad one.
//   2. The wave brings the 64 parent rows into the handle's LDS layout (off_map / MS, off_inv / KP: row l is lane l's, as in every staged
//      kernel) the way the snapshot kernel moves rows: NGW_SNAP_GROUP = 16 lanes share one row, four rows per round, sixteen rounds;
//      consecutive lanes move consecutive 16-byte pieces (S*S a multiple of 16), dwords (a multiple of 4) or, for odd S*S, dwords at
//      whatever byte address the row starts (global memory takes them) and a byte tail; then the inventory dwords.  The row index of round
//      r's row comes out of its owner's register with ds_bpermute.  In LDS a row starts on a dword (MS is a multiple of 4), so every LDS
//      access is an aligned dword.  (Banks: a ds_write_b32 of 32 lanes covers two rows' 16-dword runs, MS / 4 - odd - dwords apart; where the
//      runs overlap modulo 32 that write is 2-way.  The rows' loads are 64 independent addresses in HBM: they dominate.)
//   3. Barrier; every lane runs lean_body<STAGE = true, WT = false, EXT> once on its row, the entry fetched with ds_bpermute (lane 63 holds
//      the all-zero entry: what an invalid id or a skipped pair runs - a no-op).
//   4. Barrier; the rows go out to the destination slots the same cooperative way, each lane stores its child's scalars and its three
//      reports (consecutive lanes, consecutive addresses).
// Source and destination may be the same allocation (a node pool in one buffer), so neither is __restrict__ against the other; within a wave
// every load of a parent row is done before the first store of a child row (the barriers), across waves the call's contract keeps them
// apart (no destination slot of a call is a parent of the same call).

// VEC = bytes per map piece in global memory: 16 / 4 (S2 a multiple of it: every row of both sets is that aligned), 1 = odd S2
template <int VEC, bool TO_LDS>
__device__ __forceinline__ void expand_move_row(int8_t* gmap, int32_t* ginv, uint32_t* lmap, int32_t* linv, int S2, int K, int g) {
    typedef uint32_t u32_any __attribute__((aligned(1)));                          // a dword at any byte address
    if (VEC == 16) {
        u32x4* g4 = reinterpret_cast<u32x4*>(gmap);
        for (int p = g; p < (S2 >> 4); p += NGW_SNAP_GROUP) {
            if (TO_LDS) { const u32x4 v = g4[p]; lmap[4 * p] = v.x; lmap[4 * p + 1] = v.y; lmap[4 * p + 2] = v.z; lmap[4 * p + 3] = v.w; }
            else g4[p] = u32x4{lmap[4 * p], lmap[4 * p + 1], lmap[4 * p + 2], lmap[4 * p + 3]};
        }
    } else if (VEC == 4) {
        uint32_t* g1 = reinterpret_cast<uint32_t*>(gmap);
        for (int p = g; p < (S2 >> 2); p += NGW_SNAP_GROUP) { if (TO_LDS) lmap[p] = g1[p]; else g1[p] = lmap[p]; }
    } else {
        u32_any* g1 = reinterpret_cast<u32_any*>(gmap);
        const int nd = S2 >> 2, tail = S2 & 3;
        for (int p = g; p < nd; p += NGW_SNAP_GROUP) { if (TO_LDS) lmap[p] = g1[p]; else g1[p] = lmap[p]; }
        uint8_t* lb = reinterpret_cast<uint8_t*>(lmap);
        if (g < tail) { if (TO_LDS) lb[4 * nd + g] = (uint8_t)gmap[4 * nd + g]; else gmap[4 * nd + g] = (int8_t)lb[4 * nd + g]; }
    }
    for (int p = g; p < K; p += NGW_SNAP_GROUP) { if (TO_LDS) linv[p] = ginv[p]; else ginv[p] = linv[p]; }
}

// The gathered stage-in of step 2, for every kernel that brings 64 saved rows into LDS (here, ngw_successors.inc, ngw_slot_observe.inc): row l - map at
// lmap + l * MSdw, inventory at linv + l * KP - is the one lane l names in `sic`, an index its owner has checked and clamped.
template <int VEC>
__device__ __forceinline__ void expand_rows_in(const NgwSnapRows& rows, int sic, uint32_t* lmap, int32_t* linv, int MSdw, int KP, int S2, int K, uint32_t tid) {
    const int g = (int)(tid % NGW_SNAP_GROUP), q = (int)(tid / NGW_SNAP_GROUP);
    constexpr int ROWS = EPB / NGW_SNAP_GROUP;                                     // rows per round
#pragma unroll 4
    for (int it = 0; it < EPB / ROWS; it++) {
        const int j = it * ROWS + q;
        const int sj = __builtin_amdgcn_ds_bpermute(j << 2, sic);
        expand_move_row<VEC, true>(rows.map + (size_t)sj * (size_t)S2, rows.inv + (size_t)sj * (size_t)K, lmap + j * MSdw, linv + j * KP, S2, K, g);
    }
}

template <int VEC, bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_expand_kernel(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a, const NgwExpand x) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S = a.S, K = a.K, S2 = a.S2;
    // ---- 1. this lane's pair
    const bool inside = pair < (int64_t)x.count;
    int si = 0, di = 0, action = 0;
    if (inside) {
        si = x.si ? x.si[pair] : (int)pair;
        di = x.di ? x.di[pair] : (int)pair;
        action = x.actions[pair];
    }
    const bool ok = inside && (uint32_t)si < (uint32_t)x.src_rows && (uint32_t)di < (uint32_t)x.dst_rows;
    uint32_t flags = (inside && !ok && si != NGW_IDX_NONE && di != NGW_IDX_NONE) ? NGW_F_BAD_INDEX : 0u;   // (NGW_IDX_NONE: a pair that is not there)
    if (__ballot(ok) == 0) {                                                       // no live pair in this wave - a frontier's padding: nothing to stage
        if (flags) atomicOr(a.b.flags, flags);
        return;
    }
    const int sic = ok ? si : 0, dic = ok ? di : -1;
    const int2 rc = reinterpret_cast<const int2*>(x.src.loc)[sic];
    int r = rc.x, c = rc.y;
    int f = x.src.facing[sic];
    int sel = x.src.selected[sic];
    int steps = x.src.step_count[sic];
    const uint32_t episode = x.src.episode[sic];
    LeanTable t = lean_fetch_table(dspec);
    if (tid >= NGW_MAX_ACTIONS) t = LeanTable{0u, 0u, 0u, 0u, 0u, 0u};             // (lane 63 holds the all-zero entry: a no-op)
    NgwStepU U;
    NgwExtU X;
    lean_fetch_uniforms<EXT>(dspec, U, X);
    // ---- 2. the 64 parent rows into the handle's LDS layout
    uint32_t* const lds_map = lds + a.off_map;
    int32_t* const lds_inv = reinterpret_cast<int32_t*>(lds + a.off_inv);
    const int g = (int)(tid % NGW_SNAP_GROUP), q = (int)(tid / NGW_SNAP_GROUP);
    const int MSdw = a.MS >> 2, KP = a.KP;
    constexpr int ROWS = EPB / NGW_SNAP_GROUP;                                     // rows per round
    expand_rows_in<VEC>(x.src, sic, lds_map, lds_inv, MSdw, KP, S2, K, tid);
    __syncthreads();
    // ---- 3. one step of this lane's row
    int8_t* const mp = reinterpret_cast<int8_t*>(lds_map) + tid * a.MS;
    int32_t* const inv = lds_inv + tid * KP;
    const bool valid = ok && (uint32_t)action < (uint32_t)U.n_actions;
    const int ai = (valid ? action : 63) << 2;
    const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t1);
    const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t3);
    const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t5);
    // (`ok` in the place of `live`: a skipped pair raises no NGW_F_INVALID_ACTION; STAGE without WT reads and writes LDS only)
    const LeanOut o = lean_body<true, false, EXT>(U, X, e0, e1, e2, e3, e4, e5, ok, valid, S, K, mp, inv, nullptr, nullptr, 0u, 0u, r, c, f, sel, steps,
                                                  a.autoreset, a.horizon);
    flags |= o.flags;
    __syncthreads();
    // ---- 4. the child rows to their slots, the scalars, the reports
#pragma unroll 4
    for (int it = 0; it < EPB / ROWS; it++) {
        const int j = it * ROWS + q;
        const int dj = __builtin_amdgcn_ds_bpermute(j << 2, dic);
        if (dj >= 0)
            expand_move_row<VEC, false>(x.dst.map + (size_t)dj * (size_t)S2, x.dst.inv + (size_t)dj * (size_t)K, lds_map + j * MSdw, lds_inv + j * KP, S2, K, g);
    }
    if (ok) {
        reinterpret_cast<int2*>(x.dst.loc)[di] = int2{o.r, o.c};
        x.dst.facing[di] = o.f;
        x.dst.selected[di] = (uint8_t)o.sel;
        x.dst.step_count[di] = o.steps;
        x.dst.episode[di] = episode;
        if (x.reward) x.reward[pair] = o.reward;                                   // (an invalid id: reward 0, info 0, not an end - lean_epilogue)
        if (x.done) x.done[pair] = (uint8_t)o.ended;
        if (x.info) x.info[pair] = o.info;
    }
    if (flags) atomicOr(a.b.flags, flags);
}

// what the launchers of the kernels that step saved rows several times (ngw_slot_rollout.inc, ngw_playout.inc: X = NgwSlotRollout / NgwPlayout) check alike
template <class X>
bool slot_step_args_ok(const NgwLaunch* a, const X* x) {
    return x->count > 0 && x->n_steps >= 1 && x->src_rows >= 1 && a->S >= 3 && a->S <= NGW_MAX_MAP_SIZE && a->K >= 1 && a->K <= NGW_MAX_ITEMS && a->MS >= a->S2 &&
           !(a->MS & 3) && a->b.flags && x->src.map && (!x->keep || (x->dst.map && x->dst_rows >= 1)) && (x->keep || !x->di);
}

}  // namespace
