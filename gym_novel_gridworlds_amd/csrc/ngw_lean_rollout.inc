// ngw_lean_rollout.inc - the fused rollout kernel (included by ngw_lean.inc) and its launcher.

// ---------------------------------------------------------------- stage-in of a wave's 64 envs (fused rollouts, plan evaluation)
// What a kernel that keeps the state on chip for several steps reads before its first step, as ONE memory round trip: pose, selected item and
// step count into registers, the inventory rows and the map chunk (coalesced 16-B pieces, `buf` is the caller's piece registers) into the
// handle's LDS layout (off_map / off_inv, MS, KP), lane l's micro-op entry, and the uniform step parameters U (and X when EXT).  The caller
// puts the barrier behind it.  bmap .. bstp: the wave's first row of each state array.
struct RolloutLane { int r, c, f, sel, steps; uint32_t rowoff, t0, t1, t2, t3, t4, t5; uint32_t* lds_map; int8_t* mp; int32_t* inv; };
template <int MAPMODE, bool EXT>
__device__ __forceinline__ RolloutLane rollout_stage_in(const NgwDevSpec* __restrict__ dspec, const NgwLaunch& a, uint32_t* lds, uint32_t tid, int K, int npieces,
                                                        const char* bmap, const char* binv, const char* bloc, const char* bfac, const char* bsel,
                                                        const char* bstp, u32x4 (&buf)[PB], NgwStepU& U, NgwExtU& X) {
    const int2 rc = ldg<int2>(bloc, tid * 8u);
    int r = rc.x, c = rc.y;
    int f = ldg<int>(bfac, tid * 4u);
    int sel = ldg<uint8_t>(bsel, tid);
    int steps = ldg<int>(bstp, tid * 4u);
    const uint32_t rowoff = tid * 4u * (uint32_t)K;
    u32x4 q[IQ];
#pragma unroll
    for (int j = 0; j < IQ; j++)
        q[j] = (4 * j < K) ? ldg<u32x4>(binv, rowoff + 4u * (uint32_t)min(4 * j, K - 4)) : u32x4{0u, 0u, 0u, 0u};
    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
    if (tid < NGW_MAX_ACTIONS) {
        const uint2* ld = reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(dspec->act_lean) + tid * (4u * NGW_LEAN_DW));
        const uint2 x0 = ld[0], x1 = ld[1], x2 = ld[2];
        t0 = x0.x; t1 = x0.y; t2 = x1.x; t3 = x1.y; t4 = x2.x; t5 = x2.y;
    }
#pragma unroll
    for (int j = 0; j < PB; j++) buf[j] = ldg<u32x4>(bmap, 16u * (uint32_t)min((int)tid + EPB * j, npieces - 1));
    {
        const uint32_t* up = reinterpret_cast<const uint32_t*>(&dspec->u);
        uint32_t uw[16];
#pragma unroll
        for (int i = 0; i < 16; i++) uw[i] = up[i];
        __builtin_memcpy(&U, uw, sizeof(U));
    }
    X = NgwExtU{};                                                                // wrapper predicates (FireWall, FenceRestriction, Crate): 9 more dwords
    if (EXT) {
        const uint32_t* xp = reinterpret_cast<const uint32_t*>(&dspec->x);
        uint32_t xw[9];
#pragma unroll
        for (int i = 0; i < 9; i++) xw[i] = xp[i];
        __builtin_memcpy(&X, xw, sizeof(X));
    }
    uint32_t* lds_map = lds + a.off_map;
    int8_t* mp = reinterpret_cast<int8_t*>(lds_map) + tid * a.MS;
    int32_t* inv = reinterpret_cast<int32_t*>(lds + a.off_inv) + tid * a.KP;
#pragma unroll
    for (int j = 0; j < IQ; j++)
        if (4 * j < K) {
            const int o = min(4 * j, K - 4);
            inv[o] = (int)q[j].x; inv[o + 1] = (int)q[j].y; inv[o + 2] = (int)q[j].z; inv[o + 3] = (int)q[j].w;
        }
    pieces_lds<true, MAPMODE>(buf, a, lds_map, 0, npieces, tid);
    for (int base = EPB * PB; base < npieces; base += EPB * PB) {
#pragma unroll
        for (int j = 0; j < PB; j++) buf[j] = ldg<u32x4>(bmap, 16u * (uint32_t)min(base + (int)tid + EPB * j, npieces - 1));
        pieces_lds<true, MAPMODE>(buf, a, lds_map, base, npieces, tid);
    }
    RolloutLane L;
    L.r = r; L.c = c; L.f = f; L.sel = sel; L.steps = steps; L.rowoff = rowoff;
    L.t0 = t0; L.t1 = t1; L.t2 = t2; L.t3 = t3; L.t4 = t4; L.t5 = t5;
    L.lds_map = lds_map; L.mp = mp; L.inv = inv;
    return L;
}

// ---------------------------------------------------------------- fused rollout of the plain configurations
// T steps in one launch on the SAME branch-free step (lean_body).  The state lives in LDS (maps, inventory rows) and registers
// (pose, selected item, step count) for the whole launch and goes back to HBM ONCE, when the launch ends, as the wave's coalesced
// chunk - nobody can observe the buffers in between - so a step issues no global store at all unless the caller asked for
// the per-step reward / done rows (ngw_rollout_outputs).  The general kernel wrote every change through on every step (7
// vector-memory stores per wave-step) and dispatched the action kinds through a divergent switch.
// SUPPLIED = false: uniform actions from Philox (ngw_rollout; one block per four steps); true: the caller's [T, N] rows.
// LIDAR: the fused LidarInFront observation of the state the launch ENDS in (the observation buffer holds one row per env, so
// the steps in between have no observer; up to round 3 the general kernel rebuilt it after every step of a rollout).
template <int MAPMODE, bool SUPPLIED, bool EXT, bool LIDAR>
__global__ void __launch_bounds__(NGW_EPB) ngw_rollout_lean(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    const int S = a.S, K = a.K;
    const int npieces = 4 * a.S2;
    const int64_t env0 = (int64_t)bid * EPB, e = env0 + tid;
    const int nlive = (int)min((int64_t)EPB, a.n - env0);
    const bool live = (int)tid < nlive;
    char* const bmap = reinterpret_cast<char*>(a.b.map) + (uint64_t)bid * (uint32_t)(EPB * a.S2);
    char* const binv = reinterpret_cast<char*>(a.b.inv) + (uint64_t)bid * (uint32_t)(EPB * 4 * K);
    char* const bloc = reinterpret_cast<char*>(a.b.loc) + (uint64_t)bid * (EPB * 8);
    char* const bfac = reinterpret_cast<char*>(a.b.facing) + (uint64_t)bid * (EPB * 4);
    char* const bsel = reinterpret_cast<char*>(a.b.selected) + (uint64_t)bid * EPB;
    char* const bstp = reinterpret_cast<char*>(a.b.step_count) + (uint64_t)bid * (EPB * 4);
    // ---- stage in: pose, inventory rows, micro-op entries, map chunk (rollout_stage_in, shared with the plan evaluator)
    u32x4 buf[PB];
    NgwStepU U;
    NgwExtU X;
    const RolloutLane L = rollout_stage_in<MAPMODE, EXT>(dspec, a, lds, tid, K, npieces, bmap, binv, bloc, bfac, bsel, bstp, buf, U, X);
    int r = L.r, c = L.c, f = L.f, sel = L.sel, steps = L.steps;
    const uint32_t rowoff = L.rowoff;
    const uint32_t t0 = L.t0, t1 = L.t1, t2 = L.t2, t3 = L.t3, t4 = L.t4, t5 = L.t5;
    uint32_t* const lds_map = L.lds_map;
    int8_t* const mp = L.mp;
    int32_t* const inv = L.inv;
    // the cold path's placement sequence: staged once for the whole launch
    if (tid < NGW_MAX_PLACE / 4) lds[a.off_act + tid] = reinterpret_cast<const uint32_t*>(dspec->place_seq)[tid];
    __syncthreads();

    const uint64_t env_global = (uint64_t)(a.env_base + e);
    uint32_t key0 = (uint32_t)a.action_seed, key1 = (uint32_t)(a.action_seed >> 32) ^ 0xA511E9B3u;
    // (the Philox keys in VGPRs: as scalars the compiler hoists the twenty round keys of a block out of the T-loop - twenty more
    //  loop-invariant SGPRs, which it then parks in VGPR lanes and fetches back one v_readlane per round)
    PIN_V(key0); PIN_V(key1);
    // the absolute step number, in a VGPR pair (every lane the same value): as a scalar pair it ended up inside an 8-register tuple
    // that the allocator wrote to VGPR lanes and read back whole on every iteration (8 + 8 moves per step)
    uint32_t tt_lo = (uint32_t)a.t0, tt_hi = (uint32_t)((uint64_t)a.t0 >> 32);
    PIN_V(tt_lo); PIN_V(tt_hi);
    uint32_t aw0 = 0, aw1 = 0, aw2 = 0, aw3 = 0;
    int n_steps = a.n_steps, autoreset = a.autoreset, horizon = a.horizon, n_actions = U.n_actions;
    const LeanUV UV = lean_uv(U);
    PIN_V(n_actions);
    int Sv = S, Kv = K;                                                            // (same reason: only vector instructions read them inside the loop)
    PIN_V(Sv); PIN_V(Kv); PIN_V(autoreset); PIN_V(horizon);
    uint32_t episode = live ? a.b.episode[e] : 0u;
    int acc_ret = 0, acc_len = 0, acc_sum = 0, acc_eps = 0;
    if (a.acc && live) { acc_ret = a.acc[e]; acc_len = a.acc[a.n_pad + e]; acc_sum = a.acc[2 * a.n_pad + e]; acc_eps = a.acc[3 * a.n_pad + e]; }
    uint32_t flags = 0;
    int reward = 0, ended = 0;
    uint32_t info = 0;
    int act_next = 0;
    if (SUPPLIED) act_next = live ? a.actions[e] : 0;
    // action(t, env) = (w * A) >> 32 with w = word (t & 3) of philox(key = action_seed ^ tag; ctr = (t >> 2, env)): the block of the
    // first step now, the following ones where a step crosses into them (no first-iteration case inside the loop: the compiler
    // peeled it into a second copy of the whole step, cold path included)
    if (!SUPPLIED)
        philox_block((tt_lo >> 2) | (tt_hi << 30), tt_hi >> 2, (uint32_t)env_global, (uint32_t)(env_global >> 32), key0, key1, aw0, aw1, aw2, aw3);
    for (int t = 0; t < n_steps; t++) {
        int action;
        if (SUPPLIED) {                                                            // the next step's row is requested one step ahead
            action = act_next;
            if (t + 1 < n_steps && live) act_next = a.actions[(int64_t)(t + 1) * a.t0 + e];
        } else {
            const uint32_t qq = tt_lo & 3u;
            const uint32_t w = qq == 0 ? aw0 : (qq == 1 ? aw1 : (qq == 2 ? aw2 : aw3));
            action = (int)__umulhi(w, (uint32_t)n_actions);
            tt_lo += 1u;
            tt_hi += tt_lo == 0u ? 1u : 0u;
            if ((__builtin_amdgcn_readfirstlane((int)tt_lo) & 3) == 0)            // (uniform) the next step starts a block
                philox_block((tt_lo >> 2) | (tt_hi << 30), tt_hi >> 2, (uint32_t)env_global, (uint32_t)(env_global >> 32), key0, key1, aw0, aw1, aw2, aw3);
        }
        const bool valid = live && (uint32_t)action < (uint32_t)n_actions;
        const int ai = (valid ? action : 63) << 2;
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t1);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t3);
        const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t5);
        const LeanOut o = lean_body<true, false, EXT>(UV, X, e0, e1, e2, e3, e4, e5, live, valid, Sv, Kv, mp, inv, bmap, binv, 0u, rowoff, r, c, f, sel, steps,
                                                      autoreset, horizon);
        r = o.r; c = o.c; f = o.f; sel = o.sel; steps = o.steps;
        flags |= o.flags;
        if (valid || !live) { reward = o.reward; ended = o.ended; info = o.info; }
        else { reward = 0; ended = 0; info = 0; }                                  // invalid id: the env is left untouched (:236)
        if (__any(o.do_reset)) {                                                   // cold path: a prepared row if there is one, else the placement loop
            // (inlined, and with every uniform argument read from the HBM blob in here - the LDS offsets too - so that the loop's own
            //  scalars are not kept alive across, or spilled around, this region: round 3's out-of-line call left 67 v_readlane in the loop)
            if (o.do_reset) {
                const GLOBAL_AS NgwLaunch* lp = (const GLOBAL_AS NgwLaunch*)&dspec->lp;
                const uint32_t c_cand = lp->off_cand, c_act = lp->off_act, c_perm = lp->off_perm;
                {   // Terminal observations (ngw_set_terminal_capture; NgwTerm): the state this episode ENDED in - the lane's map and inventory
                    // row in LDS, its pose in registers - goes to the side set before the next episode overwrites it.  (The per-launch step
                    // kernels copy the rows from the observation buffers, terminal_capture above; here the state lives on chip.)  Off: one
                    // scalar load inside this cold region.
                    const GLOBAL_AS NgwTerm* tp = (const GLOBAL_AS NgwTerm*)&dspec->term;
                    int8_t* const tmap = tp->map;
                    if (tmap) {
                        const int c_S2 = lp->S2, c_K = lp->K;
                        GLOBAL_AS uint8_t* tm = (GLOBAL_AS uint8_t*)tmap + (uint64_t)e * (uint32_t)c_S2;
                        const LDS_AS uint32_t* m4 = (const LDS_AS uint32_t*)mp;
                        const LDS_AS uint8_t* m1 = (const LDS_AS uint8_t*)mp;
                        const int nd = c_S2 >> 2;
                        for (int i = 0; i < nd; i++) *(GLOBAL_AS uint32_t*)(tm + 4 * i) = m4[i];     // (rows of odd-sized maps start anywhere: global memory takes the unaligned dwords)
                        for (int i = 4 * nd; i < c_S2; i++) tm[i] = m1[i];
                        GLOBAL_AS int32_t* ti = (GLOBAL_AS int32_t*)tp->inv + (uint64_t)e * (uint32_t)c_K;
                        for (int k = 0; k < c_K; k++) ti[k] = inv[k];
                        ((GLOBAL_AS int32_t*)tp->loc)[2 * e] = o.r; ((GLOBAL_AS int32_t*)tp->loc)[2 * e + 1] = o.c;
                        ((GLOBAL_AS int32_t*)tp->facing)[e] = o.f;
                    }
                }
                episode++;
                uint32_t rr = new_episode_inline(dspec, (LDS_AS int8_t*)mp, (LDS_AS int32_t*)inv, (LDS_AS uint32_t*)(lds + c_cand + tid),
                                                 (const LDS_AS uint8_t*)(lds + c_act), (LDS_AS uint16_t*)(lds + c_perm), env_global, e, episode, true);
                rr &= ~(uint32_t)NGW_F_ROWS_STORED;
                flags |= rr & 0xFFu;
                r = (int)((rr >> 8) & 0xFFu); c = (int)((rr >> 16) & 0xFFu); f = (int)(rr >> 24);
                sel = 0; steps = 0;
            }
        }
        if (live) {
            if (a.row_reward) a.row_reward[(int64_t)t * a.row_stride + e] = reward;
            if (a.row_done) a.row_done[(int64_t)t * a.row_stride + e] = (uint8_t)ended;
            acc_ret += reward; acc_len += 1;
            if (ended) { acc_sum += acc_ret; acc_eps += 1; acc_ret = 0; acc_len = 0; }
        }
    }
    // ---- stage out: the wave's map / inventory chunk as coalesced 16-B pieces, then the per-env scalars and the last step's outputs
    if (LIDAR) {
        if (tid < LIDAR_ITEM_DW) lds[a.off_litem + tid] = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[tid];
        lidar_epilogue(a, lds, (int)tid, live, mp + r * S + c, f, inv);
    }
    __syncthreads();
    {
        g_u32x4* gmap = (g_u32x4*)(reinterpret_cast<u32x4*>(bmap) + tid);
        for (int base = 0; base < npieces; base += EPB * PB) {
            pieces_lds<false, MAPMODE>(buf, a, lds_map, base, npieces, tid);
#pragma unroll
            for (int j = 0; j < PB; j++)
                if (base + (int)tid + EPB * j < npieces) gmap[base + EPB * j] = buf[j];
        }
        u32x4 iq[IQ];
        g_u32x4* ginv = (g_u32x4*)(reinterpret_cast<u32x4*>(binv) + tid);
        inv_lds<false>(iq, a, reinterpret_cast<int32_t*>(lds + a.off_inv), tid);
#pragma unroll
        for (int j = 0; j < IQ; j++) { if (j * EPB < 16 * K && (int)tid + EPB * j < 16 * K) ginv[EPB * j] = iq[j]; }
    }
    if (live) {
        stg<int2>(bloc, tid * 8u, int2{r, c});
        stg<int>(bfac, tid * 4u, f);
        stg<uint8_t>(bsel, tid, (uint8_t)sel);
        stg<int>(bstp, tid * 4u, steps);
        a.b.episode[e] = episode;
        a.b.reward[e] = reward;
        a.b.done[e] = (uint8_t)ended;
        a.b.info[e] = info;
        if (a.acc) { a.acc[e] = acc_ret; a.acc[a.n_pad + e] = acc_len; a.acc[2 * a.n_pad + e] = acc_sum; a.acc[3 * a.n_pad + e] = acc_eps; }
    }
    if (flags) atomicOr(a.b.flags, flags);
    raise_host_flags(a.b.flags_host, flags);
}

// fused rollout: ngw_rollout_lean, one unit per map addressing mode (eight kernels each: the heaviest to compile)
template <int MM>
hipError_t rollout(const NgwDevSpec* dspec, const NgwLaunch* a, int feat, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    return with_flag(a->mode == NGW_MODE_ROLLOUT_ACT, [&](auto SUP) {
        return with_flag((feat & NGW_FEAT_LIDAR) != 0, [&](auto L) {
            return with_flag((feat & NGW_FEAT_EXT) != 0, [&](auto E) {
                return launch_kernel<ngw_rollout_lean<MM, decltype(SUP)::value, decltype(E)::value, decltype(L)::value>>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, dspec, *a);
            });
        });
    });
}

