// ngw_plans.inc - plan evaluation (a unit of its own).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // the fused rollout's stage-in and lean_body

namespace {
//
// Result (i, p) is what env i would collect if the caller's plan p - n_steps action ids - were stepped from its CURRENT state with
// ngw_step_device: the sum of the rewards, the number of steps taken, whether the plan ran into an episode end, and the info word of its last
// step.  The plan stops at the first step that ends the episode (goal, FireWall death, the horizon under autoreset); that step counts.
// Nothing is committed: the kernel reads the state and stores nothing but the four result arrays (and the sticky error flags).
//
// Shape: the fused rollout's (ngw_lean_rollout.inc, SUPPLIED = true) without what makes a rollout a rollout.  One work-group is one wave:
// 64 consecutive envs of ONE plan.  It stages those envs exactly as the rollout does (rollout_stage_in: pose in registers, inventory rows
// and maps in the handle's LDS layout), steps them n_steps times on lean_body - the action of step t + 1 requested while step t runs, the
// entry fetched with ds_bpermute - and never stores the state back: no stage-out, no write-through, no reset path (no new_episode_inline, no
// Philox, no store to a.b.*).  A lane whose step ended the episode runs the remaining steps as no-ops (valid = false: the all-zero entry)
// and stops accumulating; the loop ends early once no lane of the wave is alive.
//
// Block order (NgwPlan::plan_major = 0, the default): env-block-major, bid = env_block * n_plans + p - the P work-groups that stage the same
// 64 maps are neighbours in dispatch order.  plan_major = 1 is the other order (bid = p * env_blocks + env_block), kept for the A/B of
// tools/plan_cost.py (DESIGN.md 4.6 has the figures).
//
// a.actions = the plans, int32 [n_steps][n_plans][a.t0] with a.t0 = the env stride (>= n): 64 lanes read consecutive addresses.
// Results are plan-major [n_plans][n_pad]: 64 lanes store consecutive addresses; columns of padding envs are 0.
template <int MAPMODE, bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_plans_lean(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a, const NgwPlan pa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t nblk = (uint32_t)(a.n_pad / EPB), P = (uint32_t)pa.n_plans;
    uint32_t eb, p;                                                                // (wave-uniform: one scalar division per launch)
    if (pa.plan_major) { p = blockIdx.x / nblk; eb = blockIdx.x - p * nblk; }
    else { eb = blockIdx.x / P; p = blockIdx.x - eb * P; }
    const int S = a.S, K = a.K;
    const int npieces = 4 * a.S2;
    const int64_t env0 = (int64_t)eb * EPB, e = env0 + tid;
    const int nlive = (int)min((int64_t)EPB, a.n - env0);
    const bool live = (int)tid < nlive;
    char* const bmap = reinterpret_cast<char*>(a.b.map) + (uint64_t)eb * (uint32_t)(EPB * a.S2);
    char* const binv = reinterpret_cast<char*>(a.b.inv) + (uint64_t)eb * (uint32_t)(EPB * 4 * K);
    const char* const bloc = reinterpret_cast<const char*>(a.b.loc) + (uint64_t)eb * (EPB * 8);
    const char* const bfac = reinterpret_cast<const char*>(a.b.facing) + (uint64_t)eb * (EPB * 4);
    const char* const bsel = reinterpret_cast<const char*>(a.b.selected) + (uint64_t)eb * EPB;
    const char* const bstp = reinterpret_cast<const char*>(a.b.step_count) + (uint64_t)eb * (EPB * 4);
    // the first action is requested with the stage-in's loads
    const int32_t* const pl = a.actions + ((int64_t)p * a.t0 + e);
    const int64_t tstride = (int64_t)P * a.t0;
    int act_next = live ? pl[0] : 0;
    u32x4 buf[PB];
    NgwStepU U;
    NgwExtU X;
    const RolloutLane L = rollout_stage_in<MAPMODE, EXT>(dspec, a, lds, tid, K, npieces, bmap, binv, bloc, bfac, bsel, bstp, buf, U, X);
    int r = L.r, c = L.c, f = L.f, sel = L.sel, steps = L.steps;
    __syncthreads();

    int n_steps = a.n_steps, autoreset = a.autoreset, horizon = a.horizon, n_actions = U.n_actions;
    const LeanUV UV = lean_uv(U);
    int Sv = S, Kv = K;                                                            // (as in the rollout: only vector instructions read them inside the loop)
    PIN_V(n_actions); PIN_V(Sv); PIN_V(Kv); PIN_V(autoreset); PIN_V(horizon);
    bool alive = live;
    int ret = 0, len = 0, ended = 0;
    uint32_t info = 0, flags = 0;
    for (int t = 0; t < n_steps; t++) {
        const int action = act_next;
        if (t + 1 < n_steps && live) act_next = pl[(int64_t)(t + 1) * tstride];   // the next step's row is requested one step ahead
        const bool valid = alive && (uint32_t)action < (uint32_t)n_actions;
        const int ai = (valid ? action : 63) << 2;                                 // (lane 63 holds the all-zero entry: a no-op)
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)L.t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)L.t1);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)L.t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)L.t3);
        const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)L.t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)L.t5);
        // `alive` in the place of `live`: an id outside the action list raises NGW_F_INVALID_ACTION only while the plan still runs
        const LeanOut o = lean_body<true, false, EXT>(UV, X, e0, e1, e2, e3, e4, e5, alive, valid, Sv, Kv, L.mp, L.inv, bmap, binv, 0u, L.rowoff, r, c, f, sel,
                                                      steps, autoreset, horizon);
        r = o.r; c = o.c; f = o.f; sel = o.sel; steps = o.steps;
        flags |= o.flags;
        if (alive) {                                                               // (an invalid id: reward 0, info 0, not an end - lean_epilogue)
            ret += o.reward; len += 1; info = o.info;
            if (o.ended) { ended = 1; alive = false; }                             // the ending step counts; no reset runs, the plan is over
        }
        if (!__any(alive)) break;
    }
    // ---- the four results of this (env, plan); nothing else is stored
    const uint64_t col = (uint64_t)p * (uint64_t)a.n_pad + (uint64_t)env0;
    stg<int>(pa.ret + col, tid * 4u, ret);
    stg<int>(pa.length + col, tid * 4u, len);
    stg<uint8_t>(pa.ended + col, tid, (uint8_t)ended);
    stg<uint32_t>(pa.info + col, tid * 4u, info);
    if (flags) atomicOr(a.b.flags, flags);
    raise_host_flags(a.b.flags_host, flags);
}

}  // namespace
