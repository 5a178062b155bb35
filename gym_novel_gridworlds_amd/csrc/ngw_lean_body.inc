// ngw_lean_body.inc - THE step (included by ngw_lean.inc): one branch-free body driven by the action's micro-op entry, used by every per-launch step kernel,
// the fused rollouts and the one-env resident loop.

// Bit k of `x` as a lane mask-free 0 / 1 value with a per-lane k.
__device__ __forceinline__ uint32_t bit_of(uint32_t x, uint32_t k) { return (x >> k) & 1u; }

// ---- THE success predicate, shared by lean_body (every step kernel, the fused rollouts, the one-env loop) and the action-mask kernel
//      (ngw_mask.inc): whatever decides info['result'] lives here and nowhere else, so the mask cannot drift from the step.
// Condition bits NGW_CB_* of one lane for one action entry: most bits depend on the state only (the block in front, its 4-neighbourhood,
// the cell two ahead, the uniform inventory slots); MISSING, NEED_TABLE and NO_ARG_ITEM depend on the entry (recipe inputs in e1 / e2 -
// the caller read their slots iv0..iv3 -, the table flag and argument of e0).  axe_ok / missing: what lean_body needs of them besides.
// NEAR2 = false: the caller knows that both "near" rules look for the same item (the plain step kernel's spec class): no second test at all.
template <bool NEAR2 = true, class UT>
__device__ __forceinline__ uint32_t lean_cond_bits(const UT& U, uint32_t e0, uint32_t e2, int front, int front2, bool ok2, bool okN, bool okS, bool okW,
                                                   bool okE, int nbN, int nbS, int nbW, int nbE, int inv_place, int inv_axe, int inv_arg,
                                                   int iv0, int iv1, int iv2, int iv3, int sel, bool& axe_ok, uint32_t& missing) {
    const int axe_item = U.axe_item;
    axe_ok = axe_item && inv_axe >= 1 && sel == axe_item;                          // novelty_wrappers.py:155
    const int nearP = U.place_near, nearE = U.ext_near;
    const bool near_place = (okN && nbN == nearP) || (okS && nbS == nearP) || (okW && nbW == nearP) || (okE && nbE == nearP);
    bool near_ext = near_place;                                                    // Pogostick: both rules look for a tree_log
    // (scalar parameters: a uniform skip where both rules look for the same item; parameters pinned in VGPRs - the fused rollout - : no branch)
    if (NEAR2 && (!__is_same(UT, NgwStepU) || nearE != nearP)) {
        const bool ne = !nearE || (okN && nbN == nearE) || (okS && nbS == nearE) || (okW && nbW == nearE) || (okE && nbE == nearE);
        near_ext = nearE != nearP ? ne : near_place;
    }
    missing = (iv0 < (int)(e2 & 255u) ? 1u : 0u) | (iv1 < (int)((e2 >> 8) & 255u) ? 2u : 0u) |
              (iv2 < (int)((e2 >> 16) & 255u) ? 4u : 0u) | (iv3 < (int)(e2 >> 24) ? 8u : 0u);   // :422-427
    const uint32_t fbit = 1u << front;
    uint32_t cb = 1u << NGW_CB_TRUE;
    cb |= front != 0 ? 1u << NGW_CB_FRONT_NZ : 0u;
    cb |= (ok2 && front2 == 0) ? 0u : 1u << NGW_CB_JUMP_BLOCKED;
    cb |= (U.brk_mask & fbit) ? 0u : 1u << NGW_CB_NOT_BRK;
    cb |= inv_place >= 1 ? 0u : 1u << NGW_CB_NO_PLACE_ITEM;
    cb |= front == U.ext_src ? 0u : 1u << NGW_CB_NOT_SRC;
    cb |= near_ext ? 0u : 1u << NGW_CB_NOT_NEAR;
    cb |= missing ? 1u << NGW_CB_MISSING : 0u;
    cb |= (((e0 >> 7) & 1u) && front != U.table_item) ? 1u << NGW_CB_NEED_TABLE : 0u;
    cb |= inv_arg >= 1 ? 0u : 1u << NGW_CB_NO_ARG_ITEM;
    cb |= (!axe_ok && U.axe_required) ? 1u << NGW_CB_NEED_AXE : 0u;
    cb |= near_place ? 1u << NGW_CB_NEAR_PLACE : 0u;
    cb |= (axe_ok || (!axe_item && (U.rew_mask & fbit))) ? 1u << NGW_CB_BRK_REWARD : 0u;
    return cb;
}

// outcome of an entry: s = 1 if its condition A holds, else 2 if B holds, else 0 (success)
__device__ __forceinline__ uint32_t lean_outcome(uint32_t cb, uint32_t e4) {
    const uint32_t cA = bit_of(cb, e4 & 15u), cB = bit_of(cb, (e4 >> 4) & 15u);
    return cA ? 1u : (cB << 1);
}

// The wrappers' predicates around Break (EXT), the only ones that are not table entries.  brk_act: this lane's action is a valid Break.
//   restricted:  FenceRestriction.step :924-946 refuses the Break (the step fails, whatever the table said)
//   fence_twice: FenceRestriction let it through - the wrapper runs env.step() AND its own epilogue, which reports success (:949-972)
//   crate_now:   Crate.step :1086-1089 hands out the crate's ingredients first - unless the Crate wrapper sits BELOW FenceRestriction
//                (NGW_XF_CRATE_IN_FENCE): then a restricted Break never reaches it
// The cells the fence rule reads are fetched only when some lane of the wave breaks a breakable block (a wave-uniform skip).
struct LeanBreakX { bool restricted, fence_twice, crate_now; };
template <class UT, class CELL>
__device__ __forceinline__ LeanBreakX lean_break_ext(const UT& U, const NgwExtU& X, bool brk_act, int front, int S, int r, int c, int f, int fr, int fc,
                                                     int fcell, const CELL& cell_at) {
    LeanBreakX xb = {false, false, false};
    const uint32_t fbit = 1u << front;
    xb.crate_now = brk_act && X.crate_item && front == X.crate_item;
    if (X.fence_mode && __any(brk_act && (U.brk_mask & fbit))) {                    // FenceRestriction.step :924-946
        const int ac0 = r * S + c, fence = X.fence_item;
        bool restricted;
        if (X.fence_mode == 1) {                                                   // medium: fence beside the AGENT, across its facing
            const int side = f <= 1 ? 1 : S;
            restricted = cell_at(ac0 - side) == fence || cell_at(ac0 + side) == fence;
        } else {                                                                   // hard: any fence in the 3x3 around the block in front
            restricted = false;
            const bool in3 = fr > 0 && fr < S - 1 && fc > 0 && fc < S - 1;         // (a breakable block is never on the border)
            const int base = in3 ? fcell : ac0;
#pragma unroll
            for (int k = 0; k < 9; k++) restricted |= cell_at(base + (k / 3 - 1) * S + (k % 3 - 1)) == fence;
            restricted &= in3;
        }
        if (brk_act && (U.brk_mask & fbit)) {
            if (restricted && front != fence) {
                xb.restricted = true;
                if (X.nest & NGW_XF_CRATE_IN_FENCE) xb.crate_now = false;
            } else xb.fence_twice = true;
        }
    }
    return xb;
}

// result of one entry: the table's outcome, then the wrappers' Break predicates (lean_body reaches the same value through `succ`)
__device__ __forceinline__ bool lean_result(uint32_t s, const LeanBreakX& xb) { return xb.fence_twice || (s == 0 && !xb.restricted); }

// ---- what follows the predicate, shared by lean_body and the lookahead kernel (ngw_lookahead.inc): how an outcome is reported, the reward
//      rule, what a success changes, what the goal test counts, the FireWall check at the new position and the goal / horizon epilogue.
//      lean_body applies the effects to the state; the lookahead kernel keeps them in registers.  Neither restates a rule.
__device__ __forceinline__ bool lean_is_break(uint32_t e0) { return (e0 >> 24) & 1u; }
// how outcome s of an entry is reported: result, message code and argument, cost code (a Break with the selected axe costs axe_cost :155-165)
struct LeanRep { bool succ; int msg, arg, cost; };
template <class UT>
__device__ __forceinline__ LeanRep lean_report(const UT& U, uint32_t e0, uint32_t e4, uint32_t e5, uint32_t s, int front, uint32_t missing, bool axe_ok) {
    LeanRep p;
    const int aarg = (e0 >> 8) & 255;
    p.succ = s == 0;                                                               // (a no-op entry "succeeds" at doing nothing)
    p.msg = (int)((e4 >> (8u + 4u * s)) & 15u);
    const uint32_t asel = (e4 >> (20u + 2u * s)) & 3u;
    p.arg = (asel == 1 ? front : 0) | (asel == 2 ? (int)((e0 >> 16) & 255u) : 0) | (asel == 3 ? (int)(((uint32_t)aarg << 8) | missing) : 0);
    p.cost = (int)((e5 >> (14u + 6u * s)) & 63u);
    if (p.succ && lean_is_break(e0) && axe_ok) p.cost = U.axe_cost;                 // novelty_wrappers.py:155-165
    return p;
}
// FenceRestriction refused the Break (:924-946) / let it through and reports success itself (:949-972)
__device__ __forceinline__ void lean_report_restricted(LeanRep& p, uint32_t e5) { p.succ = false; p.msg = NGW_MSG_FENCE_RESTRICTION; p.arg = 0; p.cost = (int)((e5 >> 14) & 63u); }
__device__ __forceinline__ void lean_report_fence_twice(LeanRep& p, uint32_t e5) { p.succ = true; p.cost = (int)((e5 >> 14) & 63u); p.msg = NGW_MSG_NONE; p.arg = 0; }
// reward of a step before the goal test: the entry's const, or the axe / break-reward rule of Break, when it succeeds under its reward condition
template <class UT>
__device__ __forceinline__ int lean_reward(const UT& U, uint32_t e0, uint32_t e5, uint32_t cb, bool succ, bool axe_ok) {
    const int rew_val = lean_is_break(e0) ? (axe_ok ? (int)U.axe_reward : U.break_reward) : (int)(int8_t)(e5 & 255u);
    return (succ && bit_of(cb, (e5 >> 8) & 15u)) ? rew_val : U.reward_step;
}
// effects of a success: the move (0 stay, 1 the cell in front, 2 two ahead), the front-cell write, the slot it changes and by how much
__device__ __forceinline__ uint32_t lean_move(uint32_t e4, bool succ) { return succ ? (e4 >> 26) & 3u : 0u; }
__device__ __forceinline__ bool lean_writes_cell(uint32_t e4, bool succ) { return succ && ((e4 >> 30) & 1u); }
__device__ __forceinline__ int lean_cell_value(uint32_t e3) { return (int)((e3 >> 8) & 255u); }
__device__ __forceinline__ int lean_slot(uint32_t e3, uint32_t e5, int front) { return ((e5 >> 12) & 3) == 1 ? front : (int)(e3 & 255u); }
__device__ __forceinline__ bool lean_updates_slot(uint32_t e5, bool succ) { return succ && ((e5 >> 12) & 3) != 0; }
template <class UT>
__device__ __forceinline__ int lean_delta(const UT& U, uint32_t e0, uint32_t e3, int front, bool axe_ok) {
    return lean_is_break(e0) ? (axe_ok ? (int)U.axe_qty : 1 + (int)((U.brk2_mask >> front) & 1u)) : ((int)e3 >> 16);
}
__device__ __forceinline__ bool lean_crafts(uint32_t e0, bool succ) { return succ && (e0 & 0x70u) != 0; }   // n_inputs > 0: a recipe
// how many goal items the inventory holds after the step (:354-357), piece by piece: the slot a success changes ...
__device__ __forceinline__ int lean_goal_slot(bool upd, int slot, int goal_item, int inv_slot, int delta, int inv_goal) {
    return (upd && slot == goal_item) ? inv_slot + delta : inv_goal;
}
// ... what a crate holds of item i (Crate.step :1086-1089; the crate's own slot 0 holds no ingredient), and of the goal item
__device__ __forceinline__ int lean_crate_qty(const NgwExtU& X, int i) {
    const uint32_t w0 = X.crate_add[0], w1 = X.crate_add[1], w2 = X.crate_add[2];   // (by value: a select between the three ADDRESSES would keep X in memory)
    const uint32_t w = i < 8 ? w0 : (i < 16 ? w1 : w2);
    return (int)((w >> (4 * (i & 7))) & 15u);
}
__device__ __forceinline__ int lean_crate_goal(const NgwExtU& X, int goal_item, int K) { return (goal_item >= 1 && goal_item < K) ? lean_crate_qty(X, goal_item) : 0; }
// ... what a recipe consumes of it (:455-474; ids of a recipe are distinct)
__device__ __forceinline__ int lean_craft_goal_used(uint32_t e0, uint32_t e1, uint32_t e2, int goal_item) {
    const int nin = (e0 >> 4) & 7;
    const int in0 = e1 & 255, in1 = (e1 >> 8) & 255, in2 = (e1 >> 16) & 255, in3 = e1 >> 24;
    const int nd0 = e2 & 255, nd1 = (e2 >> 8) & 255, nd2 = (e2 >> 16) & 255, nd3 = e2 >> 24;
    return (nin > 0 && in0 == goal_item ? nd0 : 0) + (nin > 1 && in1 == goal_item ? nd1 : 0) +
           (nin > 2 && in2 == goal_item ? nd2 : 0) + (nin > 3 && in3 == goal_item ? nd3 : 0);
}
// ... and the pick-up (grab_entities :538-554): a cell of the 3 x 3 around the new position that holds an entity is taken
template <class UT>
__device__ __forceinline__ bool lean_grabs(const UT& U, int id) { return id != 0 && ((U.ent_mask >> id) & 1u); }
// the goal test: done while the inventory holds a goal item, with the forced reward (:354-357)
template <class UT>
__device__ __forceinline__ int lean_goal_done(const UT& U, int goal_cnt, int& rew) {
    const int done = goal_cnt >= 1;
    if (done) rew = U.reward_done;
    return done;
}
// FireWall.step :1168-1189, after the wrapped step: does the check run for this entry (wrapper nesting), is a 4-neighbour of the new cell on fire
__device__ __forceinline__ bool lean_fire_on(const NgwExtU& X, bool valid, uint32_t e0) {
    const uint32_t kind = e0 & 15u, aarg = (e0 >> 8) & 255u;
    return X.fire_item && valid && !((X.nest & NGW_XF_FIRE_SKIP_BREAK) && kind == NGW_ACT_BREAK) &&
           !((X.nest >> 8) && kind == NGW_ACT_CRAFT && aarg + 1u == (X.nest >> 8));
}
__device__ __forceinline__ bool lean_burning(const NgwExtU& X, int n, int s, int w, int e) {
    const int fire = X.fire_item;
    return n == fire || s == fire || w == fire || e == fire;
}
__device__ __forceinline__ void lean_report_fire(const NgwExtU& X, LeanRep& p, int& rew, int& done) { rew = X.fire_reward; done = 1; p.msg = NGW_MSG_FIRE_WALL; p.arg = 0; }

// What one step computes, shared by the per-launch kernel and the fused rollout.  STAGE: the lane's map is in LDS (`mp`), else its
// cells are read from HBM (`bmap` + `mapoff`).  WT: write every change through to the observation buffers in HBM (per-launch
// kernel); the fused rollout keeps the state in LDS / registers and stores it once, when the launch ends.
struct LeanOut { int r, c, f, sel, steps, reward, ended; uint32_t info, flags; bool do_reset;
                 bool wcell; int cellv; uint32_t grab; };   // the cell writes of this step, for whoever keeps the occupancy bit rows: front cell := cellv; bit k of grab: cell k of the 3 x 3 around the NEW position was picked up

// the step's outputs: step count (:362; FenceRestriction's own epilogue counts a second time :966), reward, the packed info word, and
// whether the episode ends - done, or the horizon under the same-step autoreset (done = 1 for both, info bit 1 only for goal-done)
__device__ __forceinline__ void lean_epilogue(LeanOut& o, bool live, bool valid, int steps0, int twice, int rew, int done, const LeanRep& p,
                                              int autoreset, int horizon) {
    o.flags = 0; o.reward = 0; o.ended = 0; o.steps = steps0; o.info = 0; o.do_reset = false;
    if (valid) {
        o.steps = steps0 + 1 + twice;                                              // :362
        o.reward = rew; o.ended = done;
        o.info = (p.succ ? 1u : 0u) | ((uint32_t)done << 1) | ((uint32_t)p.cost << 2) | ((uint32_t)p.msg << 8) | ((uint32_t)p.arg << 16);
        if (autoreset && (done || (horizon > 0 && o.steps >= horizon))) { o.do_reset = true; o.ended = 1; }   // same-step autoreset
    } else if (live) o.flags = NGW_F_INVALID_ACTION;
}

// The uniform step parameters as lean_body reads them, unpacked.  The per-launch kernel hands NgwStepU itself (scalars: used once);
// the fused rollout hands this struct with the fields that only ever feed vector instructions PINNED IN VGPRS (every lane holds the
// same value): a loop-invariant scalar costs an SGPR for the whole launch, the loop needs ~110 of them with these, and what does not
// fit the compiler parks in VGPR lanes and fetches back with a v_readlane at every use - 83 of them in the T-loop before this.
struct LeanUV {
    int place_item, axe_item, goal_item, place_near, ext_near, ext_src, table_item, axe_required, axe_cost, axe_reward, axe_qty;
    int break_reward, reward_step, reward_done;
    uint32_t brk_mask, rew_mask, brk2_mask, ent_mask;
    int n_entities, feat;                                                          // (these two decide uniform branches: scalars)
};
__device__ __forceinline__ LeanUV lean_uv(const NgwStepU& U) {
    LeanUV V;
    V.place_item = U.place_item; V.axe_item = U.axe_item; V.goal_item = U.goal_item; V.place_near = U.place_near; V.ext_near = U.ext_near;
    V.ext_src = U.ext_src; V.table_item = U.table_item; V.axe_required = U.axe_required; V.axe_cost = U.axe_cost; V.axe_reward = U.axe_reward;
    V.axe_qty = U.axe_qty; V.break_reward = U.break_reward; V.reward_step = U.reward_step; V.reward_done = U.reward_done;
    V.brk_mask = U.brk_mask; V.rew_mask = U.rew_mask; V.brk2_mask = U.brk2_mask; V.ent_mask = U.ent_mask;
    V.n_entities = U.n_entities; V.feat = U.feat;
    PIN_V(V.place_item); PIN_V(V.axe_item); PIN_V(V.goal_item); PIN_V(V.place_near); PIN_V(V.ext_near); PIN_V(V.ext_src); PIN_V(V.table_item);
    PIN_V(V.axe_required); PIN_V(V.axe_cost); PIN_V(V.axe_reward); PIN_V(V.axe_qty); PIN_V(V.break_reward); PIN_V(V.reward_step); PIN_V(V.reward_done);
    PIN_V(V.brk_mask); PIN_V(V.rew_mask); PIN_V(V.brk2_mask); PIN_V(V.ent_mask);
    return V;
}

// HOOK: work of the caller that only needs data of the FIRST round trip (the bit-row lidar's rotations of its rows): run once the step's
// cell reads are out and nothing of them has been waited for yet - a wave that is alone on its SIMD has nothing else to do there.
struct NoHook { __device__ __forceinline__ void operator()() const {} };
// TR: what the spec can hold at all, as compile-time facts.  LeanFull: everything, behind the wave-uniform skips below.  LeanPlain: the plain
// step kernel's spec class (ngw_lean_step.inc: no Jump action, no entities, one "near" item) - the skips and what they guard are not compiled.
struct LeanFull { static constexpr bool jump = true, entities = true, near2 = true; };
struct LeanPlain { static constexpr bool jump = false, entities = false, near2 = false; };
template <bool STAGE, bool WT, bool EXT, bool HW = false, class TR = LeanFull, class UT, class HOOK = NoHook>
__device__ __forceinline__ LeanOut lean_body(const UT& U, const NgwExtU& X, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t e4, uint32_t e5, bool live,
                                             bool valid, int S, int K, int8_t* mp, int32_t* inv, char* bmap, char* binv, uint32_t mapoff,
                                             uint32_t rowoff, int r, int c, int f, int sel, int steps0, int autoreset, int horizon, const HOOK& hook = HOOK(),
                                             char* hmap = nullptr, char* hinv = nullptr /* HW: the same block's rows in the host's mirror */) {
    // ---- L0: every LDS read whose address is known now: the inventory slots with a uniform id or an id from the entry ...
    const int place_item = U.place_item, axe_item = U.axe_item, goal_item = U.goal_item;
    const int aarg = (e0 >> 8) & 255;
    int inv_place = inv[place_item], inv_axe = inv[axe_item], inv_arg = inv[min(aarg, K - 1)], inv_goal = inv[goal_item];
    int iv0 = inv[e1 & 255], iv1 = inv[(e1 >> 8) & 255], iv2 = inv[(e1 >> 16) & 255], iv3 = inv[e1 >> 24];
    // ---- L0: every LDS read whose address is known now (block in front :369-389, its 4-neighbourhood :391-411, two
    //      cells ahead for Jump, the inventory slots with a uniform id or an id from the entry)
    const int dr = (f == 0) ? -1 : (f == 1 ? 1 : 0), dc = (f == 2) ? -1 : (f == 3 ? 1 : 0);
    const int fr = r + dr, fc = c + dc, dcell = dr * S + dc, fcell = r * S + c + dcell;
    auto cell_at = [&](int cell) -> int { return STAGE ? (int)mp[cell] : (int)ldg<int8_t>(bmap, mapoff + (uint32_t)cell); };
    int front = cell_at(fcell);
    const bool okN = fr > 0, okS = fr < S - 1, okW = fc > 0, okE = fc < S - 1;     // only in-bounds cells count
    int nbN = cell_at(okN ? fcell - S : fcell), nbS = cell_at(okS ? fcell + S : fcell);
    int nbW = cell_at(okW ? fcell - 1 : fcell), nbE = cell_at(okE ? fcell + 1 : fcell);
    const int fr2 = fr + dr, fc2 = fc + dc;
    const bool ok2 = TR::jump && fr2 >= 0 && fr2 <= S - 1 && fc2 >= 0 && fc2 <= S - 1;
    int front2 = 1;
    if (TR::jump && (U.feat & NGW_FEAT_JUMP)) front2 = cell_at(ok2 ? fcell + dcell : fcell);
    hook();
    PIN_V(front); PIN_V(nbN); PIN_V(nbS); PIN_V(nbW); PIN_V(nbE);
    if (TR::jump) PIN_V(front2);
    PIN_V(inv_place); PIN_V(inv_axe); PIN_V(inv_arg); PIN_V(inv_goal); PIN_V(iv0); PIN_V(iv1); PIN_V(iv2); PIN_V(iv3);
    // ---- L1: the slot a success changes (the block in front, or the entry's const slot)
    const int slot = lean_slot(e3, e5, front);
    int inv_slot = inv[slot];
    PIN_V(inv_slot);

    // ---- condition bits NGW_CB_* of this lane
    bool axe_ok;
    uint32_t missing;
    const uint32_t cb = lean_cond_bits<TR::near2>(U, e0, e2, front, front2, ok2, okN, okS, okW, okE, nbN, nbS, nbW, nbE, inv_place, inv_axe, inv_arg,
                                       iv0, iv1, iv2, iv3, sel, axe_ok, missing);

    // ---- outcome: s = 1 if condition A holds, else 2 if B holds, else 0 (success)
    const uint32_t s = lean_outcome(cb, e4);
    LeanRep p = lean_report(U, e0, e4, e5, s, front, missing, axe_ok);
    const bool is_break = lean_is_break(e0);
    // ---- wrappers around Break (FenceRestriction, Crate): the only predicates that are not table entries
    bool fence_twice = false, crate_now = false;
    if (EXT) {
        const LeanBreakX xb = lean_break_ext(U, X, is_break && valid, front, S, r, c, f, fr, fc, fcell, cell_at);
        crate_now = xb.crate_now; fence_twice = xb.fence_twice;
        if (xb.restricted) lean_report_restricted(p, e5);
    }
    // reward of a success: the entry's const, or the axe / break-reward rule of Break
    const bool succ = p.succ;                                                      // (what the wrappers report beyond this point changes no effect)
    int rew = lean_reward(U, e0, e5, cb, succ, axe_ok);
    // ---- effects of a success
    const uint32_t mv = lean_move(e4, succ);
    const int nr = mv == 1 ? fr : (TR::jump && mv == 2 ? fr2 : r), nc = mv == 1 ? fc : (TR::jump && mv == 2 ? fc2 : c);
    // turn LUT: 2 bits per (turn, facing): none {0,1,2,3}, left {2,3,1,0} (:258-268), right {3,2,0,1} (:269-279)
    const int nf = (int)((0x4B1EE4u >> (((e4 >> 25) & 0x18u) + 2u * (uint32_t)f)) & 3u);
    const int nsel = (succ && (e4 >> 31)) ? aarg : sel;
    const bool wcell = lean_writes_cell(e4, succ);
    const int cellv = lean_cell_value(e3);
    const int delta = lean_delta(U, e0, e3, front, axe_ok);
    const bool upd = lean_updates_slot(e5, succ);
    const bool crafted = lean_crafts(e0, succ);

    // ---- apply: LDS (the reset path reads it) and write-through to HBM
    // how many goal items the inventory holds after this step (:354-357), from registers
    int goal_cnt = lean_goal_slot(upd, slot, goal_item, inv_slot, delta, inv_goal);
    if (EXT && __any(crate_now)) {                                                 // Crate.step :1086-1089 (the crate's own slot holds no ingredient)
        for (int i = 1; i < K; i++) {
            const int q = lean_crate_qty(X, i);
            if (q && crate_now) {
                const int nv = inv[i] + q;
                inv[i] = nv; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)i, nv); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)i, nv);
            }
        }
        if (crate_now) goal_cnt += lean_crate_goal(X, goal_item, K);
    }
    if (wcell) { if (STAGE) mp[fcell] = (int8_t)cellv; if (WT) stg<int8_t>(bmap, mapoff + (uint32_t)fcell, (int8_t)cellv); if (HW) stgs<int8_t>(hmap, mapoff + (uint32_t)fcell, (int8_t)cellv); }
    if (__any(crafted)) {                                                          // :455-474 (ids of a recipe are distinct)
        if (crafted) {
            const int nin = (e0 >> 4) & 7;
            const int in0 = e1 & 255, in1 = (e1 >> 8) & 255, in2 = (e1 >> 16) & 255, in3 = e1 >> 24;
            const int nd0 = e2 & 255, nd1 = (e2 >> 8) & 255, nd2 = (e2 >> 16) & 255, nd3 = e2 >> 24;
            if (nin > 0) { inv[in0] = iv0 - nd0; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)in0, iv0 - nd0); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)in0, iv0 - nd0); }
            if (nin > 1) { inv[in1] = iv1 - nd1; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)in1, iv1 - nd1); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)in1, iv1 - nd1); }
            if (nin > 2) { inv[in2] = iv2 - nd2; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)in2, iv2 - nd2); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)in2, iv2 - nd2); }
            if (nin > 3) { inv[in3] = iv3 - nd3; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)in3, iv3 - nd3); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)in3, iv3 - nd3); }
            goal_cnt -= lean_craft_goal_used(e0, e1, e2, goal_item);
        }
    }
    if (upd) { inv[slot] = inv_slot + delta; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)slot, inv_slot + delta); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)slot, inv_slot + delta); }
    uint32_t grab = 0;
    if (TR::entities && U.n_entities) {                                            // grab_entities :538-554 (3x3 incl. own cell)
        const int ac = nr * S + nc;
        int ev[9];
        bool found = false;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            ev[k] = cell_at(ac + (k / 3 - 1) * S + (k % 3 - 1));
            found |= lean_grabs(U, ev[k]);
        }
        found &= valid;
        if (__any(found)) {
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const int id = ev[k];
                if (found && lean_grabs(U, id)) {
                    const int qc = ac + (k / 3 - 1) * S + (k % 3 - 1);
                    if (STAGE) mp[qc] = 0;
                    if (WT) stg<int8_t>(bmap, mapoff + (uint32_t)qc, (int8_t)0); if (HW) stgs<int8_t>(hmap, mapoff + (uint32_t)qc, (int8_t)0);
                    const int nv = inv[id] + 1;
                    inv[id] = nv; if (WT) stg<int>(binv, rowoff + 4u * (uint32_t)id, nv); if (HW) stgs<int>(hinv, rowoff + 4u * (uint32_t)id, nv);
                    goal_cnt += id == goal_item;
                    grab |= 1u << k;
                }
            }
        }
    }
    int done = lean_goal_done(U, goal_cnt, rew);                                   // :354-357
    int twice = 0;
    if (EXT) {
        if (fence_twice) { lean_report_fence_twice(p, e5); twice = 1; }            // FenceRestriction.step :949-972: its own info + a second step_count += 1 (:966)
        const bool fire_on = lean_fire_on(X, valid, e0);
        if (__any(fire_on)) {                                                      // FireWall.step :1168-1189, after the wrapped step
            const int ac = nr * S + nc;
            const bool burning = lean_burning(X, cell_at(ac - S), cell_at(ac + S), cell_at(ac - 1), cell_at(ac + 1));
            if (fire_on && burning) lean_report_fire(X, p, rew, done);
        }
    }
    LeanOut o;
    lean_epilogue(o, live, valid, steps0, twice, rew, done, p, autoreset, horizon);
    o.r = nr; o.c = nc; o.f = nf; o.sel = nsel;
    o.wcell = wcell; o.cellv = cellv; o.grab = grab;
    return o;
}

// STAGE = false: the no-stage form for big maps - the <= 14 map cells a step needs are read straight from HBM (a second,
// dependent round trip) instead of staging S*S bytes per env through LDS; no barrier, ~3 KB of LDS per wave.
// The arguments every load of the prologue needs come FIRST and as plain scalars: the compiler preloads the leading 14 dwords of
// the argument block into SGPRs (-mllvm -amdgpu-kernarg-preload-count=14, Makefile), so they are there when the wave starts -
// fetched through s_load they arrived 290 (graph replay) to 600 cycles (eager launches) after wave entry, with nothing to do
// until then (tools/exp/preload_probe.hip: 12 cycles against 392).  The six state arrays the prologue reads are ONE allocation
// (ngw_abi.cpp: state slab), so a base and five 32-bit offsets (16-byte units) name them all:
//   sbase = the map rows; o_* = offset of inventory / location / facing / selected / step_count; s2k = S*S | K << 16.
// The spec pointer is in the window too (the action entries and the uniform parameters are fetched through it).  Everything else
// stays in the argument struct and arrives while the loads are in flight.  (8 + 8 + 8 + 8 + 6 * 4 = 56 bytes = the 14 dwords.)
// LIDAR with STAGE: the fused LidarInFront epilogue marches over the map in LDS (lidar_epilogue).  LIDAR without STAGE (NR > 0): the O(1)
// form on the occupancy bit rows (ngw_boards.inc) - the lane's NR >= BS bit rows arrive with the prologue loads (o_brd: their offset
// in the state slab, like the other arrays), the step's own cell writes keep them coherent, the observation is built from them.
