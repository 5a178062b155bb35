// ngw_lookahead.inc - one-step lookahead tables (a unit of its own).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // the predicate and the functions lean_body is made of

namespace {
//
// Entry (i, a) of the table is what ngw_get_step_out would report for env i if ngw_step_device were called now with action a for that env:
// reward, done and the packed info word, under the handle's spec (every novelty and wrapper predicate) and its autoreset setting.  Nothing
// is committed: the kernel reads the state and stores nothing but the table.  Nothing here restates a game rule either: the predicate is the
// mask kernel's (lean_cond_bits, lean_outcome, lean_break_ext, lean_result), and what follows it - the report of an outcome, the reward rule,
// which cells and which inventory slot a success changes, what the pick-up adds to the goal count, the FireWall check at the new position,
// the goal / horizon epilogue - are the functions lean_body itself is made of (ngw_lean_body.inc).
//
// Shape: the mask kernel's.  One lane per env, 64 envs per wave.  The lane reads its pose, the block in front, its 4-neighbourhood, the cell
// two ahead (Jump) and the 3 x 3 windows around the three cells it can stand on after a step - where it is, the cell in front, two ahead -
// ONCE, lands its inventory row in a private LDS row, then walks the n_actions entries.  The entries are wave-uniform (lane l holds entry l,
// the loop reads entry a out of lane a with v_readlane), so every entry field is a scalar and every branch on one is a uniform branch.  What
// an action would change stays in registers: the goal count is carried as a number, the one cell write and the picked-up cells are applied
// to the window's values, not to the map.  Per action the lane stores 9 bytes into the action-major table [A][n_pad]: consecutive lanes
// store consecutive addresses.

// The 3 x 3 window around cell `ac` (row-major, k = 3 * (dy + 1) + dx + 1) when `ok` (the cell is inside the wall ring: every address is a
// cell of this env's map), else around `fallback` (the agent's own cell) - a window that no successful move can select.
template <class CELL>
__device__ __forceinline__ void look_window(int (&w)[9], bool ok, int ac, int fallback, int S, const CELL& cell_at) {
    const int base = ok ? ac : fallback;
#pragma unroll
    for (int k = 0; k < 9; k++) w[k] = cell_at(base + (k / 3 - 1) * S + (k % 3 - 1));
}

template <bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_lookahead_kernel(const NgwDevSpec* __restrict__ dspec, const NgwBufs b, uint32_t n32, int S, int K,
                                                                int autoreset, int horizon, uint64_t n_pad, int32_t* __restrict__ out_reward,
                                                                uint8_t* __restrict__ out_done, uint32_t* __restrict__ out_info) {
    __shared__ int32_t inv_lds[NGW_EPB * (NGW_MAX_ITEMS | 1)];
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    const LeanLane l = lean_load_lane(b, n32, S, K, inv_lds);                      // (the mask kernel's prologue, ngw_mask.inc)
    const bool live = l.live;
    const int r = l.r, c = l.c, f = l.f, sel = l.sel;
    const int32_t* const inv = l.inv;
    const int steps0 = ldg<int>(reinterpret_cast<const char*>(b.step_count) + (uint64_t)bid * (EPB * 4), tid * 4u);
    auto cell_at = [&](int cell) -> int { return (int)ldg<int8_t>(l.bmap, l.mapoff + (uint32_t)cell); };
    const LeanTable t = lean_fetch_table(dspec);
    NgwStepU U;
    NgwExtU X;
    lean_fetch_uniforms<EXT>(dspec, U, X);
    const LeanFront q = lean_front_cells(U, S, r, c, f, cell_at);
    const int fr = q.fr, fc = q.fc, fcell = q.fcell, dcell = q.dcell, front = q.front, fr2 = q.fr2, fc2 = q.fc2;
    // ---- the windows the pick-up and the FireWall check read at the new position, one per cell a step can end on
    const bool need_win = U.n_entities != 0 || (EXT && X.fire_item != 0);
    const int ac0 = r * S + c;
    int w0[9], w1[9], w2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { w0[k] = 0; w1[k] = 0; w2[k] = 0; }
    if (need_win) {
        look_window(w0, true, ac0, ac0, S, cell_at);
        look_window(w1, q.okN && q.okS && q.okW && q.okE, fcell, ac0, S, cell_at);
        if (U.feat & NGW_FEAT_JUMP) look_window(w2, fr2 > 0 && fr2 < S - 1 && fc2 > 0 && fc2 < S - 1, fcell + dcell, ac0, S, cell_at);
    }
    const int inv_place = inv[U.place_item], inv_axe = inv[U.axe_item], inv_goal = inv[U.goal_item];
    const int goal_item = U.goal_item;
    const int A = min(U.n_actions, NGW_MAX_ACTIONS);
    char* const o_rew = reinterpret_cast<char*>(out_reward) + (uint64_t)bid * (EPB * 4);
    char* const o_done = reinterpret_cast<char*>(out_done) + (uint64_t)bid * EPB;
    char* const o_info = reinterpret_cast<char*>(out_info) + (uint64_t)bid * (EPB * 4);
    for (int a = 0; a < A; a++) {
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)t.t0, a), e1 = (uint32_t)__builtin_amdgcn_readlane((int)t.t1, a);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_readlane((int)t.t2, a), e3 = (uint32_t)__builtin_amdgcn_readlane((int)t.t3, a);
        const uint32_t e4 = (uint32_t)__builtin_amdgcn_readlane((int)t.t4, a), e5 = (uint32_t)__builtin_amdgcn_readlane((int)t.t5, a);
        const int aarg = (e0 >> 8) & 255;
        const int inv_arg = inv[min(aarg, K - 1)];
        const int iv0 = inv[e1 & 255], iv1 = inv[(e1 >> 8) & 255], iv2 = inv[(e1 >> 16) & 255], iv3 = inv[e1 >> 24];
        const int slot = lean_slot(e3, e5, front);
        const int inv_slot = inv[slot];
        // ---- the predicate (the mask kernel's walk)
        bool axe_ok;
        uint32_t missing;
        const uint32_t cb = lean_cond_bits(U, e0, e2, front, q.front2, q.ok2, q.okN, q.okS, q.okW, q.okE, q.nbN, q.nbS, q.nbW, q.nbE, inv_place, inv_axe,
                                           inv_arg, iv0, iv1, iv2, iv3, sel, axe_ok, missing);
        const uint32_t s = lean_outcome(cb, e4);
        LeanRep p = lean_report(U, e0, e4, e5, s, front, missing, axe_ok);
        LeanBreakX xb = {false, false, false};
        if (EXT) {
            xb = lean_break_ext(U, X, lean_is_break(e0) && live, front, S, r, c, f, fr, fc, fcell, cell_at);
            if (xb.restricted) lean_report_restricted(p, e5);
        }
        // ---- what follows it: reward, the effects of a success as far as the outcome depends on them
        int rew = lean_reward(U, e0, e5, cb, p.succ, axe_ok);
        const uint32_t mv = lean_move(e4, p.succ);
        const bool wcell = lean_writes_cell(e4, p.succ);
        const int cellv = lean_cell_value(e3);
        const int delta = lean_delta(U, e0, e3, front, axe_ok);
        const bool upd = lean_updates_slot(e5, p.succ);
        int goal_cnt = lean_goal_slot(upd, slot, goal_item, inv_slot, delta, inv_goal);
        if (EXT && xb.crate_now) goal_cnt += lean_crate_goal(X, goal_item, K);
        if (lean_crafts(e0, p.succ)) goal_cnt -= lean_craft_goal_used(e0, e1, e2, goal_item);
        const int nr = mv == 1 ? fr : (mv == 2 ? fr2 : r), nc = mv == 1 ? fc : (mv == 2 ? fc2 : c);
        const int ac = nr * S + nc;
        int win[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int v = mv == 1 ? w1[k] : (mv == 2 ? w2[k] : w0[k]);
            win[k] = (wcell && ac + (k / 3 - 1) * S + (k % 3 - 1) == fcell) ? cellv : v;   // (the step writes the cell before it looks around)
        }
        if (U.n_entities) {
#pragma unroll
            for (int k = 0; k < 9; k++) {
                if (live && lean_grabs(U, win[k])) { goal_cnt += win[k] == goal_item; win[k] = 0; }
            }
        }
        int done = lean_goal_done(U, goal_cnt, rew);
        int twice = 0;
        if (EXT) {
            if (xb.fence_twice) { lean_report_fence_twice(p, e5); twice = 1; }
            if (lean_fire_on(X, live, e0) && lean_burning(X, win[1], win[7], win[3], win[5])) lean_report_fire(X, p, rew, done);
        }
        LeanOut o;
        lean_epilogue(o, live, live, steps0, twice, rew, done, p, autoreset, horizon);
        const uint64_t row = (uint64_t)a * n_pad;
        stg<int>(o_rew + row * 4u, tid * 4u, o.reward);
        stg<uint8_t>(o_done + row, tid, (uint8_t)o.ended);
        stg<uint32_t>(o_info + row * 4u, tid * 4u, o.info);
    }
}

}  // namespace
