// ngw_slot_rollout.inc - snapshot rollout (two units: the plain and the PATH form; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // lean_body and its table fetches
#include "ngw_expand.inc"          // expand_move_row: the row mover
#include "ngw_path.inc"            // the PATH form's keys and step limits
#include "ngw_traj.inc"            // the TRAJ form's per-step rewards and lidar rows

namespace {
//
// Pair j of a call: the parent is row si[j] of the source set (the state slab, or a snapshot); it is stepped on a private copy with the
// pair's n_steps actions by the rules of ngw_plan_eval - it stops at the first step whose `done` would be 1, that step counts, no reset ever
// runs - and reports ret / length / ended / info as ngw_plan_eval defines them.  With a destination snapshot the row as the LAST EXECUTED
// step leaves it goes to row di[j] (for a stopped pair: the state the episode ended in; the episode counter is the parent's).  Nothing but
// the destination rows, the four report arrays and the sticky error flags is stored.  Nothing here restates a game rule: the step is
// lean_body.
//
// Shape: ngw_expand_kernel's gathered stage-in and scattered stage-out around ngw_plans_lean's T-loop.  One work-group is one wave: 64
// consecutive pairs.
//   1. Stage-in, as ngw_expand.inc steps 1 - 2: lane l reads pair l and checks both indices (a skipped pair and a lane past `count` stage
//      row 0 of the source on a clamped index: nothing is ever addressed with a bad one), gathers pose, selected item, step count and
//      episode counter into registers, and the wave brings the 64 parent rows into the handle's LDS layout with expand_move_row (16 lanes
//      per row, the row index out of its owner's register with ds_bpermute).  The first action is requested together with these loads.
//   2. Barrier; the T-loop of ngw_plans.inc on the lane's own LDS row: the action of step t + 1 requested while step t runs, the entry
//      fetched with ds_bpermute (lane 63 holds the all-zero entry), lean_body<STAGE = true, WT = false, EXT> with `alive` in the place of
//      `live` (a skipped pair starts with alive = false).  A lane whose step ended the episode runs the remaining steps as no-ops - they
//      leave its row and its registers as they are - and stops accumulating; the loop ends once no lane of the wave is alive (wave-uniform:
//      the wave is the whole work-group).  A lane only ever touches its own row inside the loop: no barrier in it.
//   3. Barrier; with a destination (a kernel argument: a wave-uniform branch) the rows go out to their slots with expand_move_row and each
//      lane stores its five scalars; the four reports go to consecutive addresses; one atomicOr raises the flags.
// No reset path is in this kernel (no new_episode_inline, no Philox, no prepared row) and no store to a.b.* but the flags word.
// Source and destination may be the same allocation, so neither is __restrict__ against the other; within a wave every load of a parent
// row is done before the first store of an end state (the barriers), across waves the call's contract keeps them apart.
//
// PATH (ngw_snapshot_rollout_path): x.limits cuts pair j after min(n_steps, max(limits[j], 0)) steps - the limit folds into `alive` before the
// plan read is used, a cut pair is not `ended` -, and x.keys takes the key of the state after every executed step (ngw_path.inc), 0 for the
// others, 64 lanes on consecutive addresses.  PATH = false is the kernel as it was.
//
// TRAJ (ngw_snapshot_rollout_traj; a PATH form): x.rewards and x.obs take the reward and the LidarInFront rows of every step as ngw_traj.inc lays
// them out - 0 / zero rows for a step the pair did not execute; with x.obs the launch block is the stand-alone lidar launch's layout and every
// lane of the wave reaches every row set (the loop is wave-uniform).  TRAJ = false is the kernel as it was.
// x.vw (AgentMap views, ngw_traj.inc) takes the window, the facing id and the inventory of the same states by the same block rule under the PATH
// form's launch block: run-time outputs of this form, all nullptr = the form as it was.
//
// x.actions: int32, the action of pair j at step t at [t * x.stride + j] (stride >= count): 64 lanes read consecutive addresses.
template <int VEC, bool EXT, bool PATH = false, bool TRAJ = false>
__global__ void __launch_bounds__(NGW_EPB) ngw_slot_rollout_kernel(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a, const NgwSlotRollout x) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S = a.S, K = a.K, S2 = a.S2;
    const bool keep = x.keep != 0;
    // ---- 1. this lane's pair; its first action is requested with the stage-in's loads
    const bool inside = pair < (int64_t)x.count;
    int si = 0, di = 0, act_next = 0;
    const int32_t* const pl = x.actions + pair;
    if (inside) {
        si = x.si ? x.si[pair] : (int)pair;
        di = x.di ? x.di[pair] : (int)pair;
        act_next = pl[0];
    }
    const bool ok = inside && (uint32_t)si < (uint32_t)x.src_rows && (!keep || (uint32_t)di < (uint32_t)x.dst_rows);
    uint32_t flags = (inside && !ok && si != NGW_IDX_NONE && di != NGW_IDX_NONE) ? NGW_F_BAD_INDEX : 0u;   // (NGW_IDX_NONE: a pair that is not there)
    if (__ballot(ok) == 0) {                                                       // no live pair in this wave - a frontier's padding: nothing to stage,
        if constexpr (PATH)                                                        // every step is one no pair executed
            if (x.keys && inside)
                for (int s = 0; s < x.n_steps; s++) x.keys[pair + (int64_t)s * x.keys_stride] = 0ull;
        if constexpr (TRAJ) {
            if (x.rewards && inside)
                for (int s = 0; s < x.n_steps; s++) x.rewards[pair + (int64_t)s * x.rewards_stride] = 0;
            if (x.obs) traj_zero_tiles(a, tid, x.obs, x.obs_stride, -1, x.n_steps);      // (from -1: row block 0, the parents, too)
            if (traj_views_on(x.vw)) traj_zero_views(a, x.vw, tid, -1, x.n_steps);
        }
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
    // the 64 parent rows into the handle's LDS layout
    uint32_t* const lds_map = lds + a.off_map;
    int32_t* const lds_inv = reinterpret_cast<int32_t*>(lds + a.off_inv);
    const int g = (int)(tid % NGW_SNAP_GROUP), q = (int)(tid / NGW_SNAP_GROUP);
    const int MSdw = a.MS >> 2, KP = a.KP;
    constexpr int ROWS = EPB / NGW_SNAP_GROUP;                                     // rows per round
#pragma unroll 4
    for (int it = 0; it < EPB / ROWS; it++) {
        const int j = it * ROWS + q;
        const int sj = __builtin_amdgcn_ds_bpermute(j << 2, sic);
        expand_move_row<VEC, true>(x.src.map + (size_t)sj * (size_t)S2, x.src.inv + (size_t)sj * (size_t)K, lds_map + j * MSdw, lds_inv + j * KP, S2, K, g);
    }
    if constexpr (TRAJ)
        if (x.obs) traj_obs_begin(a, lds, tid);
    __syncthreads();
    // ---- 2. up to n_steps steps of this lane's row
    int8_t* const mp = reinterpret_cast<int8_t*>(lds_map) + tid * a.MS;
    int32_t* const inv = lds_inv + tid * KP;
    const int n_steps = x.n_steps;
    const int64_t tstride = x.stride;
    int autoreset = a.autoreset, horizon = a.horizon, n_actions = U.n_actions;
    const LeanUV UV = lean_uv(U);
    int Sv = S, Kv = K;                                                            // (as in the plan kernel: only vector instructions read them inside the loop)
    PIN_V(n_actions); PIN_V(Sv); PIN_V(Kv); PIN_V(autoreset); PIN_V(horizon);
    bool alive = ok;
    int ret = 0, len = 0, ended = 0;
    uint32_t info = 0;
    PathLane<PATH> pa;
    if constexpr (PATH) {
        pa.limit = x.limits && ok ? min(max(x.limits[pair], 0), n_steps) : n_steps;
        pa.kout = x.keys && inside ? x.keys + pair : nullptr;
        pa.kdone = 0;
        if (x.keys) pa.pk = path_begin(lds_map + tid * MSdw, inv, lds + x.off_shadow + tid * KP, S2, K, x.fields, episode);
    }
    TrajLane<TRAJ> tr;
    if constexpr (TRAJ) {
        tr.rew = x.rewards && inside ? x.rewards + pair : nullptr;
        tr.done = 0;
        if (x.obs) traj_obs_rows(a, lds, tid, ok, mp, S, r, c, f, inv, x.obs, x.obs_stride, 0);   // row block 0: the parents
        if (traj_views_on(x.vw)) traj_view_rows(a, x.vw, lds, tid, ok, r, c, f, 0);
    }
    for (int s = 0; s < n_steps; s++) {
        if constexpr (PATH) alive = alive && s < pa.limit;
        const int action = act_next;
        if (s + 1 < n_steps && inside) act_next = pl[(int64_t)(s + 1) * tstride];  // the next step's row is requested one step ahead
        const bool valid = alive && (uint32_t)action < (uint32_t)n_actions;
        const int ai = (valid ? action : 63) << 2;
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t1);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t3);
        const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t5);
        if constexpr (PATH)
            if (x.keys) pa.grp = path_front_group(pa.pk, Sv, r, c, f, pa.before);
        // `alive` in the place of `live`: an id outside the action list raises NGW_F_INVALID_ACTION only while the pair still runs
        const LeanOut o = lean_body<true, false, EXT>(UV, X, e0, e1, e2, e3, e4, e5, alive, valid, Sv, Kv, mp, inv, nullptr, nullptr, 0u, 0u, r, c, f, sel, steps,
                                                      autoreset, horizon);
        r = o.r; c = o.c; f = o.f; sel = o.sel; steps = o.steps;                   // (a no-op entry hands them back unchanged: an ended pair stays frozen)
        flags |= o.flags;
        if constexpr (PATH)
            if (x.keys) {                                                          // (wave-uniform; every lane walks it: path_after_step votes)
                const uint64_t key = path_after_step(pa.pk, o, pa.grp, pa.before, inv, Kv, x.fields);
                if (pa.kout) pa.kout[(int64_t)s * x.keys_stride] = alive ? key : 0ull;
                pa.kdone = s + 1;
            }
        if constexpr (TRAJ) {                                                      // (`alive` still says: this pair executed this step)
            if (tr.rew) tr.rew[(int64_t)s * x.rewards_stride] = alive ? o.reward : 0;
            if (x.obs) traj_obs_rows(a, lds, tid, alive, mp, S, r, c, f, inv, x.obs, x.obs_stride, s + 1);
            if (traj_views_on(x.vw)) traj_view_rows(a, x.vw, lds, tid, alive, r, c, f, s + 1);
            tr.done = s + 1;
        }
        if (alive) {                                                               // (an invalid id: reward 0, info 0, not an end - lean_epilogue)
            ret += o.reward; len += 1; info = o.info;
            if (o.ended) { ended = 1; alive = false; }                             // the ending step counts; no reset runs, the pair is over
        }
        if (!__any(alive)) break;
    }
    if constexpr (PATH)
        if (pa.kout)
            for (int s = pa.kdone; s < n_steps; s++) pa.kout[(int64_t)s * x.keys_stride] = 0ull;   // the steps no pair of this wave executed
    if constexpr (TRAJ) {
        if (tr.rew)
            for (int s = tr.done; s < n_steps; s++) tr.rew[(int64_t)s * x.rewards_stride] = 0;
        if (x.obs) traj_zero_tiles(a, tid, x.obs, x.obs_stride, tr.done, n_steps);
        if (traj_views_on(x.vw)) traj_zero_views(a, x.vw, tid, tr.done, n_steps);
    }
    __syncthreads();
    // ---- 3. the end states to their slots with the scalars (where they are kept), the reports
    if (keep) {
#pragma unroll 4
        for (int it = 0; it < EPB / ROWS; it++) {
            const int j = it * ROWS + q;
            const int dj = __builtin_amdgcn_ds_bpermute(j << 2, dic);
            if (dj >= 0)
                expand_move_row<VEC, false>(x.dst.map + (size_t)dj * (size_t)S2, x.dst.inv + (size_t)dj * (size_t)K, lds_map + j * MSdw, lds_inv + j * KP, S2, K, g);
        }
        if (ok) {
            reinterpret_cast<int2*>(x.dst.loc)[di] = int2{r, c};
            x.dst.facing[di] = f;
            x.dst.selected[di] = (uint8_t)sel;
            x.dst.step_count[di] = steps;
            x.dst.episode[di] = episode;
        }
    }
    if (ok) {
        if (x.ret) x.ret[pair] = ret;
        if (x.length) x.length[pair] = len;
        if (x.ended) x.ended[pair] = (uint8_t)ended;
        if (x.info) x.info[pair] = info;
    }
    if (flags) atomicOr(a.b.flags, flags);
}

// a = the handle's rollout layout with a.autoreset, a.horizon; one wave per 64 pairs.  PATH: lds_bytes = NGW_PATH_LDS_BYTES(the handle's, KP).
// TRAJ: as PATH, or with x->obs the stand-alone lidar launch's layout (ngw_device.h, ngw_slot_rollout_traj_launch)
template <bool PATH, bool TRAJ = false>
hipError_t slot_rollout_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwSlotRollout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    if (!slot_step_args_ok(a, x) || x->stride < x->count || !x->actions ||
        (PATH && !TRAJ && !path_args_ok(a, x->count, x->keys, x->keys_stride, x->fields, x->off_shadow, lds_bytes)) ||
        (TRAJ && !traj_args_ok(a, x->count, x->keys, x->keys_stride, x->fields, x->off_shadow, lds_bytes, x->rewards, x->rewards_stride, nullptr, 0, x->obs,
                               x->obs_stride, x->vw)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks_for(x->count)), block(NGW_EPB);
    NgwSlotRollout y = *x;
    if (TRAJ) y.vw = traj_views_ready(x->vw);
    return with_row_piece(a->S2, [&](auto V) {
        return with_flag(ext != 0, [&](auto E) {
            return launch_kernel<ngw_slot_rollout_kernel<decltype(V)::value, decltype(E)::value, PATH, TRAJ>>(grid, block, lds_bytes, stream, dspec, *a, y);
        });
    });
}

}  // namespace
