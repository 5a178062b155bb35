// ngw_playout.inc - snapshot playout (two units: the plain and the PATH form; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // lean_body, lean_mask_walk
#include "ngw_expand.inc"          // expand_move_row: the row mover
#include "ngw_sample.inc"          // the choice among the valid actions
#include "ngw_path.inc"            // the PATH form's keys and step limits
#include "ngw_traj.inc"            // the TRAJ form's per-step rewards, mask words and lidar rows
#include "ngw_table.inc"           // table_find: the GUIDED form's look-up

namespace {
//
// Pair j of a call: the parent is row si[j] of the source set (the state slab, or a snapshot); it is stepped on a private copy up to n_steps
// times by the rules of ngw_slot_rollout_kernel - it stops at the first step whose `done` would be 1, that step counts, no reset ever runs -
// with actions DRAWN HERE: at every step uniformly among the actions that would succeed from the state the pair is in (include/ngw.h, the
// choice rule of ngw_snapshot_playout: mask word, Philox word, the k-th set bit; playout_kth_bit is ngw_sample.inc's).  Nothing here restates a game rule: the mask is
// lean_mask_walk's, the step is lean_body, the generator is philox_block.
//
// Shape: ngw_slot_rollout_kernel's, with the choice in the place of the plan read.  One work-group is one wave: 64 consecutive pairs.
//   1. Stage-in, as ngw_slot_rollout.inc step 1: indices checked, loads on clamped indices (a skipped pair and a lane past `count` stage row 0
//      of the source), pose / selected item / step count / episode counter into registers, the 64 parent rows into the handle's LDS layout
//      with expand_move_row.
//   2. Barrier; the T-loop on the lane's own LDS row.  Each iteration: the mask of the lane's state (lean_mask_walk over the table the lanes
//      hold - entries read with v_readlane, a wave-uniform loop: EVERY lane runs it, the lanes of ended or skipped pairs on their frozen rows,
//      and discard the result), one Philox block every fourth step, the k-th set bit, the entry fetched with ds_bpermute (lane 63 holds the
//      all-zero entry), lean_body<STAGE = true, WT = false, EXT> with `alive` in the place of `live`.  The loop ends once no lane of the wave
//      is alive (wave-uniform: the wave is the whole work-group); the steps a pair did not execute are recorded as -1.
//   3. Barrier; the end states to their slots (where they are kept), the reports, the flags - as ngw_slot_rollout.inc step 3; a skipped pair's
//      reports are stored as 0 and its first action as -1.
// No reset path is in this kernel and no store to a.b.* but the flags word.  Source and destination may be the same allocation (see
// ngw_slot_rollout.inc).
//
// WEIGHTED (ngw_snapshot_playout_weighted): x.weights holds one float32 per action, lane a keeps x.weights[a] in a register, and the choice of
// every step is sample_choice (ngw_sample.inc) on the step's own m and w - the weighted rule of ngw_sample_actions, the uniform rule where
// the valid actions' mass is 0.  WEIGHTED = false is the kernel as it was.
//
// PATH (ngw_snapshot_playout_path): x.limits and x.keys as in ngw_slot_rollout_kernel<.., PATH = true> - the limit folds into `alive` before the
// choice, so a limited playout is the prefix of the unlimited one and the actions beyond the limit are recorded as -1.  PATH = false is the
// kernel as it was.
//
// TRAJ (ngw_snapshot_playout_traj; a PATH form): x.rewards, x.masks and x.obs take the reward, the mask word m (after the all-actions replacement)
// and the LidarInFront rows of every step as ngw_traj.inc lays them out - 0 / zero rows for a step the pair did not execute; with x.obs the launch
// block is the stand-alone lidar launch's layout and every lane of the wave reaches every row set (the loop is wave-uniform).  TRAJ = false is
// the kernel as it was.  x.vw (AgentMap views, ngw_traj.inc) takes the window, the facing id and the inventory of the same states by the same block
// rule under the PATH form's launch block: run-time outputs of this form, all nullptr = the form as it was.
//
// GUIDED (ngw_snapshot_playout_guided; a PATH and TRAJ form, instantiated in ngw_unit_playout_guided.hip alone): the rule of include/ngw.h.  The
// running key is kept whether or not x.keys is set, and the key a step leaves is the key the next step looks up: one key per step.  Before the
// choice an alive lane walks the table (table_find: per-lane divergent, read-only, bounded by the buckets, waits for nobody) for the key of the
// state it is in; x.stop with a miss clears `alive` there, in the place of the limit.  The step's weights are the lane's ROW: x.table_weights +
// b * x.tw_stride on a hit, x.weights on a miss - nullptr reads as zeros, and mass 0 is the uniform rule on the same w, so the form needs no
// WEIGHTED twin -, read in place by sample_choice: 2 * A dwords per lane and step, a row contiguous.  A frozen lane (b = -1) reads x.weights or
// nothing and its result, its F_BAD_WEIGHT included, is discarded.  x.where[t * x.where_stride + j] takes b of every executed step (-1: a miss,
// or not executed), x.depth[j] the leading executed steps with b >= 0.  The wave-uniform parts - lean_mask_walk, sample_choice's two walks,
// path_after_step's votes - are outside the divergent walk.  GUIDED = false is the kernel as it was.
//
// x.actions (may be nullptr): int32, the action of pair j at step t to [t * x.stride + j] (stride >= count) - the layout ngw_slot_rollout_kernel reads.

template <int VEC, bool EXT, bool WEIGHTED, bool PATH = false, bool TRAJ = false, bool GUIDED = false>
__global__ void __launch_bounds__(NGW_EPB) ngw_playout_kernel(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a, const NgwPlayout x) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S = a.S, K = a.K, S2 = a.S2;
    const bool keep = x.keep != 0;
    // ---- 1. this lane's pair
    const bool inside = pair < (int64_t)x.count;
    int si = 0, di = 0;
    if (inside) {
        si = x.si ? x.si[pair] : (int)pair;
        di = x.di ? x.di[pair] : (int)pair;
    }
    const bool ok = inside && (uint32_t)si < (uint32_t)x.src_rows && (!keep || (uint32_t)di < (uint32_t)x.dst_rows);
    uint32_t flags = (inside && !ok && si != NGW_IDX_NONE && di != NGW_IDX_NONE) ? NGW_F_BAD_INDEX : 0u;   // (NGW_IDX_NONE: a pair that is not there)
    if (__ballot(ok) == 0) {                                                       // no live pair in this wave - a frontier's padding: nothing to stage,
        const int T = x.n_steps;                                                   // every step is one no pair executed
        if constexpr (PATH)
            if (x.keys && inside)
                for (int s = 0; s < T; s++) x.keys[pair + (int64_t)s * x.keys_stride] = 0ull;
        if constexpr (TRAJ) {
            if (x.rewards && inside)
                for (int s = 0; s < T; s++) x.rewards[pair + (int64_t)s * x.rewards_stride] = 0;
            if (x.masks && inside)
                for (int s = 0; s < T; s++) x.masks[pair + (int64_t)s * x.masks_stride] = 0ull;
            if (x.obs) traj_zero_tiles(a, tid, x.obs, x.obs_stride, -1, T);              // (from -1: row block 0, the parents, too)
            if (traj_views_on(x.vw)) traj_zero_views(a, x.vw, tid, -1, T);
        }
        if constexpr (GUIDED) {
            if (x.where && inside)
                for (int s = 0; s < T; s++) x.where[pair + (int64_t)s * x.where_stride] = -1;
            if (x.depth && inside) x.depth[pair] = 0;
        }
        if (inside) {
            if (x.actions)
                for (int s = 0; s < T; s++) x.actions[pair + (int64_t)s * x.stride] = -1;
            if (x.ret) x.ret[pair] = 0;
            if (x.length) x.length[pair] = 0;
            if (x.ended) x.ended[pair] = (uint8_t)0;
            if (x.info) x.info[pair] = 0u;
            if (x.first_action) x.first_action[pair] = -1;
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
    float xw = 0.0f;                                                               // WEIGHTED: lane a holds x[a], the walk reads it with v_readlane
    if constexpr (WEIGHTED)
        if ((int)tid < min(U.n_actions, NGW_MAX_ACTIONS)) xw = x.weights[tid];     // (the array holds n_actions floats and no more)
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
    int32_t* const rec = x.actions ? x.actions + pair : nullptr;                   // (only ever dereferenced by a lane inside `count`)
    const int A = min(U.n_actions, NGW_MAX_ACTIONS);                               // the walk's bound: a scalar
    const uint64_t all_actions = (1ull << A) - 1ull;                               // (A <= 48)
    int autoreset = a.autoreset, horizon = a.horizon;
    const LeanUV UV = lean_uv(U);
    int Sv = S, Kv = K;                                                            // (as in the plan kernel: only vector instructions read them inside the loop)
    PIN_V(Sv); PIN_V(Kv); PIN_V(autoreset); PIN_V(horizon);
    // the pair's stream: key = (lo32(seed), hi32(seed) ^ NGW_PLAYOUT_TAG), counter = (t >> 2, 0, lo32(p), hi32(p)) with p = first_pair + j
    const uint64_t p = x.first_pair + (uint64_t)pair;
    uint32_t key0 = (uint32_t)x.seed, key1 = (uint32_t)(x.seed >> 32) ^ NGW_PLAYOUT_TAG;
    PIN_V(key0); PIN_V(key1);                                                      // (in VGPRs, as in the fused rollout: the round keys are not hoisted into SGPRs)
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    auto cell_at = [&](int cell) -> int { return (int)mp[cell]; };
    bool alive = ok;
    int ret = 0, len = 0, ended = 0, first = -1;
    uint32_t info = 0;
    PathLane<PATH> pa;
    if constexpr (PATH) {
        pa.limit = x.limits && ok ? min(max(x.limits[pair], 0), n_steps) : n_steps;
        pa.kout = x.keys && inside ? x.keys + pair : nullptr;
        if (GUIDED || x.keys) pa.pk = path_begin(lds_map + tid * MSdw, inv, lds + x.off_shadow + tid * KP, S2, K, x.fields, episode);
    }
    uint64_t kcur = 0;                                                             // GUIDED: the key of the state the pair is in before the step under way
    int depth = 0;
    int32_t* wrec = nullptr;
    if constexpr (GUIDED) {
        kcur = path_key(pa.pk, x.fields, r, c, f, sel, steps);
        wrec = x.where && inside ? x.where + pair : nullptr;
    }
    TrajLane<TRAJ> tr;
    if constexpr (TRAJ) {
        tr.rew = x.rewards && inside ? x.rewards + pair : nullptr;
        tr.msk = x.masks && inside ? x.masks + pair : nullptr;
        if (x.obs) traj_obs_rows(a, lds, tid, ok, mp, S, r, c, f, inv, x.obs, x.obs_stride, 0);   // row block 0: the parents
        if (traj_views_on(x.vw)) traj_view_rows(a, x.vw, lds, tid, ok, r, c, f, 0);
    }
    int s = 0;
    for (; s < n_steps; s++) {
        if constexpr (PATH) alive = alive && s < pa.limit;
        if ((s & 3) == 0) philox_block((uint32_t)s >> 2, 0u, (uint32_t)p, (uint32_t)(p >> 32), key0, key1, w0, w1, w2, w3);   // (uniform: s is a scalar)
        // the choice: uniform over the actions that would succeed from here; every action where none would
        uint64_t m = lean_mask_walk<EXT>(t, UV, X, A, Sv, Kv, r, c, f, sel, inv, cell_at);
        if (m == 0) m = all_actions;
        const uint32_t qq = (uint32_t)s & 3u;
        const uint32_t w = qq == 0 ? w0 : (qq == 1 ? w1 : (qq == 2 ? w2 : w3));
        int action;
        if constexpr (GUIDED) {
            const int b = (alive && kcur) ? table_find(x.tkey, x.tmask, kcur) : -1;     // (only alive lanes walk; key 0 is never stored)
            if (x.stop && b < 0) alive = false;                                    // the leaf: as if limits[j] were s
            if (wrec) wrec[(int64_t)s * x.where_stride] = alive ? b : -1;
            if (alive && b >= 0 && depth == s) depth++;
            const float* const row = b >= 0 ? x.table_weights + (size_t)b * (size_t)x.tw_stride : x.weights;
            float mass;
            uint32_t wf = 0;
            const int drawn = sample_choice(m, w, A, [&](int a) -> float { return row ? row[a] : 0.0f; }, mass, wf);
            if (alive) flags |= wf;                                                // (a bad weight counts where its row was read for a step that ran)
            action = alive ? drawn : -1;
        } else if constexpr (WEIGHTED) {                                                  // rules 3 - 6 of ngw_sample_actions on this m and this w; every lane walks
            float mass;
            const int drawn = sample_choice(m, w, A, [&](int a) -> float { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xw), a)); },
                                            mass, flags);
            action = alive ? drawn : -1;
        } else {                                                                   // (written as it always was: the instruction stream of this form is unchanged)
            const uint32_t k = __umulhi(w, (uint32_t)__popcll(m));
            action = alive ? playout_kth_bit(m, k) : -1;
        }
        if (rec && inside) rec[(int64_t)s * tstride] = action;
        if (s == 0) first = action;
        const int ai = (alive ? action : 63) << 2;
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t1);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t3);
        const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t.t5);
        if constexpr (PATH)
            if (GUIDED || x.keys) pa.grp = path_front_group(pa.pk, Sv, r, c, f, pa.before);
        const LeanOut o = lean_body<true, false, EXT>(UV, X, e0, e1, e2, e3, e4, e5, alive, alive, Sv, Kv, mp, inv, nullptr, nullptr, 0u, 0u, r, c, f, sel, steps,
                                                      autoreset, horizon);
        r = o.r; c = o.c; f = o.f; sel = o.sel; steps = o.steps;                   // (a no-op entry hands them back unchanged: an ended pair stays frozen)
        flags |= o.flags;
        if constexpr (PATH)
            if (GUIDED || x.keys) {                                                // (wave-uniform; every lane walks it: path_after_step votes)
                const uint64_t key = path_after_step(pa.pk, o, pa.grp, pa.before, inv, Kv, x.fields);
                if (pa.kout) pa.kout[(int64_t)s * x.keys_stride] = alive ? key : 0ull;
                if constexpr (GUIDED) kcur = key;                                  // (a frozen lane's row did not move: its key stays what it was)
            }
        if constexpr (TRAJ) {                                                      // (`alive` still says: this pair executed this step)
            if (tr.rew) tr.rew[(int64_t)s * x.rewards_stride] = alive ? o.reward : 0;
            if (tr.msk) tr.msk[(int64_t)s * x.masks_stride] = alive ? m : 0ull;
            if (x.obs) traj_obs_rows(a, lds, tid, alive, mp, S, r, c, f, inv, x.obs, x.obs_stride, s + 1);
            if (traj_views_on(x.vw)) traj_view_rows(a, x.vw, lds, tid, alive, r, c, f, s + 1);
        }
        if (alive) {
            ret += o.reward; len += 1; info = o.info;
            if (o.ended) { ended = 1; alive = false; }                             // the ending step counts; no reset runs, the pair is over
        }
        if (!__any(alive)) { s++; break; }
    }
    if constexpr (PATH)
        if (pa.kout)
            for (int u = s; u < n_steps; u++) pa.kout[(int64_t)u * x.keys_stride] = 0ull;
    if constexpr (TRAJ) {
        if (tr.rew)
            for (int u = s; u < n_steps; u++) tr.rew[(int64_t)u * x.rewards_stride] = 0;
        if (tr.msk)
            for (int u = s; u < n_steps; u++) tr.msk[(int64_t)u * x.masks_stride] = 0ull;
        if (x.obs) traj_zero_tiles(a, tid, x.obs, x.obs_stride, s, n_steps);
        if (traj_views_on(x.vw)) traj_zero_views(a, x.vw, tid, s, n_steps);
    }
    if constexpr (GUIDED) {
        if (wrec)
            for (int u = s; u < n_steps; u++) wrec[(int64_t)u * x.where_stride] = -1;
        if (x.depth && inside) x.depth[pair] = depth;
    }
    if (rec && inside)
        for (; s < n_steps; s++) rec[(int64_t)s * tstride] = -1;                   // the steps no pair of this wave executed
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
    if (inside) {                                                                  // (a skipped pair: alive was never set, so these are 0 / -1)
        if (x.ret) x.ret[pair] = ret;
        if (x.length) x.length[pair] = len;
        if (x.ended) x.ended[pair] = (uint8_t)ended;
        if (x.info) x.info[pair] = info;
        if (x.first_action) x.first_action[pair] = first;
    }
    if (flags) atomicOr(a.b.flags, flags);
}

// a = the handle's rollout layout with a.autoreset, a.horizon; one wave per 64 pairs.  PATH: lds_bytes = NGW_PATH_LDS_BYTES(the handle's, KP).
// TRAJ: as PATH, or with x->obs the stand-alone lidar launch's layout (ngw_device.h, ngw_playout_traj_launch)
// GUIDED: as TRAJ, with the shadows behind the layout whether or not x->keys is set, the table, the rows and x->where / x->depth
template <bool PATH, bool TRAJ = false, bool GUIDED = false>
hipError_t playout_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream) {
    if (!slot_step_args_ok(a, x) || (x->actions && x->stride < x->count) ||
        (PATH && !TRAJ && !path_args_ok(a, x->count, x->keys, x->keys_stride, x->fields, x->off_shadow, lds_bytes)) ||
        (TRAJ && !traj_args_ok(a, x->count, x->keys, x->keys_stride, x->fields, x->off_shadow, lds_bytes, x->rewards, x->rewards_stride, x->masks, x->masks_stride,
                               x->obs, x->obs_stride, x->vw)))
        return hipErrorInvalidValue;
    if constexpr (GUIDED)
        if (!x->tkey || !x->table_weights || x->tmask < 1 || x->tmask >= 0x7FFFFFFFull || (x->tmask & (x->tmask + 1)) || x->tw_stride < 1 ||
            (x->where && x->where_stride < x->count) || !x->fields || (x->fields & ~NGW_KEY_ALL) ||
            ((size_t)x->off_shadow + (size_t)NGW_EPB * (size_t)a->KP) * 4u > lds_bytes ||
            ((size_t)a->off_inv + (size_t)NGW_EPB * (size_t)a->KP) * 4u > (size_t)x->off_shadow * 4u)
            return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks_for(x->count)), block(NGW_EPB);
    NgwPlayout y = *x;
    if (TRAJ) y.vw = traj_views_ready(x->vw);
    return with_row_piece(a->S2, [&](auto V) {
        return with_flag(ext != 0, [&](auto E) {
            if constexpr (GUIDED)                                                  // (the weights are run-time rows: no WEIGHTED twin)
                return launch_kernel<ngw_playout_kernel<decltype(V)::value, decltype(E)::value, false, true, true, true>>(grid, block, lds_bytes, stream, dspec, *a, y);
            else
                return with_flag(x->weights != nullptr, [&](auto W) {
                    return launch_kernel<ngw_playout_kernel<decltype(V)::value, decltype(E)::value, decltype(W)::value, PATH, TRAJ>>(grid, block, lds_bytes, stream, dspec, *a, y);
                });
        });
    });
}

}  // namespace
