// ngw_solo.inc — the one-env handle's resident step loop.
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // lean_body: the one step

namespace {
//
// BASELINE configs[0] is ONE env driven from a Python loop (reference tests/random_action.py:51-64).  A launch per step() costs such
// a handle ~3 us of hipLaunchKernel on the host and ~7 us until the results are visible - more than the reference's own Python spends on a
// whole step - and 63 of the wave's 64 lanes idle.  This kernel stays resident between steps for as long as the caller keeps stepping,
// and uses the idle lanes to have the NEXT step's answer ready before it is asked for:
//   * every lane keeps a private copy of the env's map and inventory row in LDS (all identical between steps);
//   * SPECULATE: lane j applies action j to its copy with the one step implementation (lean_body) and writes the outcome - reward, done,
//     info word, pose, the cell write, the picked-up entities, the inventory row - as record j into page-locked host memory, undoes its
//     changes from the shared master copy, and lane 0 publishes the sequence number of the state the records belong to;
//   * the host's step(a) therefore finds its answer in record a (a table lookup: no launch, no wait unless it steps faster than the device
//     speculates), applies it to its mirror of the state and posts (a, sequence + 1) into the mailbox;
//   * COMMIT: the wave picks the command up (lane 0 polls the mailbox across PCIe), every lane applies action a to its copy - they stay
//     identical -, lane 0 writes the changes through to the state in HBM, and the loop speculates again.
// The loop ENDS - every wave (there is one) reaches the exit - when the mailbox says so (any other call on the handle stops the loop first:
// its stream is busy while the loop runs) or when no command has arrived for `timeout_ticks` of the 100 MHz chip clock; the state in HBM is
// current at every exit, the host relaunches on its next step().  Same lean_body, same tables: bit-identical with the per-launch kernels
// (tests/test_env_adapter.py and the golden adapter replays run through it).  Reference semantics only (no autoreset: `done` is sticky).

template <bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_solo_kernel(const NgwDevSpec* __restrict__ dspec, const NgwSolo p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const int S = p.S, S2 = p.S2, K = p.K, A = p.A;
    int8_t* mp = reinterpret_cast<int8_t*>(lds + p.off_map) + tid * p.MSp;          // this lane's private map
    int8_t* master = reinterpret_cast<int8_t*>(lds + p.off_master);
    int32_t* inv = reinterpret_cast<int32_t*>(lds + p.off_inv) + tid * p.KP;
    int32_t* invb = reinterpret_cast<int32_t*>(lds + p.off_invb) + tid * p.KP;
    // ---- tables: lane l holds the micro-op entry of action l (ngw_step_lean does the same)
    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
    if (tid < NGW_MAX_ACTIONS) {
        const uint2* ld = reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(dspec->act_lean) + tid * (4u * NGW_LEAN_DW));
        const uint2 x0 = ld[0], x1 = ld[1], x2 = ld[2];
        t0 = x0.x; t1 = x0.y; t2 = x1.x; t3 = x1.y; t4 = x2.x; t5 = x2.y;
    }
    NgwStepU U;
    {
        const uint32_t* up = reinterpret_cast<const uint32_t*>(&dspec->u);
        uint32_t uw[16];
#pragma unroll
        for (int i = 0; i < 16; i++) uw[i] = up[i];
        __builtin_memcpy(&U, uw, sizeof(U));
    }
    NgwExtU X = {};
    if (EXT) {
        const uint32_t* xp = reinterpret_cast<const uint32_t*>(&dspec->x);
        uint32_t xw[9];
#pragma unroll
        for (int i = 0; i < 9; i++) xw[i] = xp[i];
        __builtin_memcpy(&X, xw, sizeof(X));
    }
    // ---- the env's state: every lane reads the same rows (broadcast loads) into its own copy
    {
        const uint32_t* g4 = reinterpret_cast<const uint32_t*>(p.b.map);
        uint32_t* m4 = reinterpret_cast<uint32_t*>(mp);
        const int nd = S2 >> 2;
        for (int i = 0; i < nd; i++) m4[i] = g4[i];
        for (int i = 4 * nd; i < S2; i++) mp[i] = p.b.map[i];
        if (tid == 0) for (int i = 0; i < S2; i++) master[i] = p.b.map[i];
        for (int k = 0; k < K; k++) { const int v = p.b.inv[k]; inv[k] = v; invb[k] = v; }
    }
    int r = p.b.loc[0], c = p.b.loc[1], f = p.b.facing[0], sel = p.b.selected[0], steps = p.b.step_count[0];
    wave_lds_sync();
    uint32_t seq = p.k0;
    int pending = p.commit0;
    for (;;) {
        if (pending >= 0) {
            // ---- COMMIT: every lane applies the posted action to its copy (they stay identical); lane 0 writes the changes through
            const int a = pending;
            const bool valid = (uint32_t)a < (uint32_t)U.n_actions;
            const int ai = (valid ? a : 63) << 2;
            const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t1);
            const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t3);
            const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t5);
            const int dr = (f == 0) ? -1 : (f == 1 ? 1 : 0), dc = (f == 2) ? -1 : (f == 3 ? 1 : 0);
            const int fcell = (r + dr) * S + c + dc;
            const LeanOut o = lean_body<true, false, EXT>(U, X, e0, e1, e2, e3, e4, e5, true, valid, S, K, mp, inv, nullptr, nullptr, 0u, 0u, r, c, f, sel, steps, 0, 0);
            r = o.r; c = o.c; f = o.f; sel = o.sel; steps = o.steps;
            for (int k = 0; k < K; k++) invb[k] = inv[k];
            if (tid == 0) {
                if (o.wcell) { master[fcell] = (int8_t)o.cellv; p.b.map[fcell] = (int8_t)o.cellv; }
                if (o.grab) {
                    const int ac = o.r * S + o.c;
                    for (int k = 0; k < 9; k++)
                        if ((o.grab >> k) & 1u) { const int q = ac + (k / 3 - 1) * S + (k % 3 - 1); master[q] = 0; p.b.map[q] = 0; }
                }
                for (int k = 0; k < K; k++) p.b.inv[k] = inv[k];
                p.b.loc[0] = r; p.b.loc[1] = c; p.b.facing[0] = f; p.b.selected[0] = (uint8_t)sel; p.b.step_count[0] = steps;
                p.b.reward[0] = o.reward; p.b.done[0] = (uint8_t)o.ended; p.b.info[0] = o.info;
            }
            seq++;
            wave_lds_sync();
        }
        // ---- SPECULATE: lane j applies action j
        {
            const bool valid = (int)tid < A && tid < (uint32_t)U.n_actions;
            const int ai = (valid ? (int)tid : 63) << 2;
            const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t1);
            const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t3);
            const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t5);
            const int dr = (f == 0) ? -1 : (f == 1 ? 1 : 0), dc = (f == 2) ? -1 : (f == 3 ? 1 : 0);
            const int fcell = (r + dr) * S + c + dc;
            const LeanOut o = lean_body<true, false, EXT>(U, X, e0, e1, e2, e3, e4, e5, true, valid, S, K, mp, inv, nullptr, nullptr, 0u, 0u, r, c, f, sel, steps, 0, 0);
            if ((int)tid < A) {
                uint32_t* rec = p.out + NGW_SOLO_REC0 + tid * (uint32_t)p.rec_dw;
                rec[0] = (uint32_t)o.reward; rec[1] = o.info;
                rec[2] = (uint32_t)(o.ended & 1) | ((uint32_t)o.r << 8) | ((uint32_t)o.c << 16) | ((uint32_t)o.f << 24);
                rec[3] = (uint32_t)o.sel | ((o.wcell ? 1u : 0u) << 8) | ((uint32_t)(o.cellv & 255) << 16);
                rec[4] = (uint32_t)o.steps; rec[5] = (uint32_t)fcell; rec[6] = o.grab; rec[7] = o.flags;
                for (int k = 0; k < K; k++) rec[8 + k] = (uint32_t)inv[k];
            }
            // undo: the lane's copy goes back to the committed state
            if (o.wcell) mp[fcell] = master[fcell];
            if (o.grab) {
                const int ac = o.r * S + o.c;
                for (int k = 0; k < 9; k++)
                    if ((o.grab >> k) & 1u) { const int q = ac + (k / 3 - 1) * S + (k % 3 - 1); mp[q] = master[q]; }
            }
            for (int k = 0; k < K; k++) inv[k] = invb[k];
        }
        __builtin_amdgcn_s_waitcnt(0);                                             // the records are out ...
        __threadfence_system();                                                    // ... and ordered before the number that announces them
        if (tid == 0) *(volatile uint32_t*)(p.out + 0) = seq;
        // ---- wait for the next command (lane 0 polls the mailbox across PCIe), the quit word, or the idle limit
        int cmd = -2;                                                              // -2 keep waiting, -1 leave, >= 0 the action
        const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
        while (cmd == -2) {
            uint32_t c0 = 0, act = 0, quit = 0;
            if (tid == 0) {
                c0 = __hip_atomic_load(const_cast<uint32_t*>(p.mbox) + 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
                act = __hip_atomic_load(const_cast<uint32_t*>(p.mbox) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                quit = __hip_atomic_load(const_cast<uint32_t*>(p.mbox) + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)c0); act = (uint32_t)__builtin_amdgcn_readfirstlane((int)act);
            quit = (uint32_t)__builtin_amdgcn_readfirstlane((int)quit);
            if (c0 == seq + 1u) cmd = (int)act;                                    // (a posted command is taken even when the quit word is up: the host counts on it)
            else if (quit || __builtin_amdgcn_s_memrealtime() - t_start > (uint64_t)p.timeout_ticks) cmd = -1;
            else __builtin_amdgcn_s_sleep(8);
        }
        if (cmd < 0) break;
        pending = cmd;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __threadfence_system();
    if (tid == 0) *(volatile uint32_t*)(p.out + 1) = 1u;                           // exited: the state in HBM is the committed one, sequence number out[0]
}

}  // namespace
