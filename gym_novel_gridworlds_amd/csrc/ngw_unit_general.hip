// ngw_unit_general.hip — ngw_launch, the entry every batched step / rollout / reset launch comes through, and the general new-episode kernel.
#include "ngw_common.inc"
#include "ngw_newepisode.inc"      // new_episode, the signals towards the host
#include "ngw_lidar_march.inc"     // lidar_epilogue

namespace {

// ---------------------------------------------------------------- the general new-episode kernel
// Explicit resets (NGW_MODE_RESET) and refills of the prepared next episodes (NGW_MODE_REFILL) of every configuration the dedicated
// new-episode kernel (ngw_reset.inc) does not take: reset passes that read the map (Fence, ReplaceItem of an interior item), stacks
// of passes, the v0 tree tap, 10 x 10 plain maps, and resets that refresh the fused LidarInFront observation.  The wave stages its
// 64 maps and inventory rows into LDS, the lanes that reset run new_episode there (a prepared row if there is one, else the
// placement loop), and the chunk goes back with coalesced 16-byte pieces.  Steps and fused rollouts live in ngw_lean.inc - up to
// round 3 this kernel also carried a switch-dispatched step; there is ONE step implementation now (lean_body).
template <int MAPMODE, int MODE, bool LIDAR>
__global__ void __launch_bounds__(NGW_EPB) ngw_kernel(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    if (MODE == NGW_MODE_DBG_NOP) return;
    STAMP_DECL;
    STAMP(0);
    const int tid = threadIdx.x;
    const int64_t env0 = (int64_t)blockIdx.x * EPB;
    const int64_t e = env0 + tid;                                                  // local env index of this lane
    const bool live = e < a.n;
    const int S = a.S, K = a.K;
    const int npieces = 4 * a.S2;                                                  // EPB * S2 / 16

    // LDS carve-up (dword offsets): maps | inventory [64][KP] | candidate masks [CW][64] | placement sequence
    uint32_t* lds_map = lds + a.off_map;
    int32_t* lds_inv = reinterpret_cast<int32_t*>(lds + a.off_inv);
    int8_t* mp = reinterpret_cast<int8_t*>(lds_map) + tid * a.MS;                 // this lane's map
    int32_t* inv = lds_inv + tid * a.KP;                                           // this lane's inventory row
    uint32_t* cand = lds + a.off_cand + tid;

    // ---- issue EVERY global load of the prologue before touching LDS: placement sequence, first map round, scalars, inventory
    const uint32_t psv = reinterpret_cast<const uint32_t*>(dspec->place_seq)[min(tid, NGW_MAX_PLACE / 4 - 1)];
    uint32_t lit = 0;
    if (LIDAR && tid < LIDAR_ITEM_DW) lit = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[tid];
    int r = 1, c = 1, f = 0, sel = 0, steps = 0, action = 0;
    uint32_t episode = 0, nx_old = 0;
    if (MODE == NGW_MODE_REFILL) {
        // a.b is ONE SLOT of the shadow set (a.autoreset = its number, a.horizon = depth - 1); a.actions carries the main
        // episode[].  The slot belongs to the one episode E of (main, main + depth] with E & (depth - 1) == slot; its row is
        // stale unless it was prepared for exactly E.  Waves without a stale row leave before touching anything else.
        if (live) {
            nx_old = a.b.episode[e];
            const uint32_t main_ep = reinterpret_cast<const uint32_t*>(a.actions)[e];
            const uint32_t target = main_ep + 1u + (((uint32_t)a.autoreset - main_ep - 1u) & (uint32_t)a.horizon);
            if (nx_old != target) { action = 1; episode = target - 1u; } else episode = nx_old;
        }
        if (!__any(action)) return;
    }
    // A whole wavefront of envs that ALL get a new episode (an unmasked reset; a refill behind a batch that ended its episodes together): nothing of
    // the old rows survives, so they are not staged - the prologue's round trip and S*S + 4 K bytes per env less (a C2 reset of every env 21.6 -> 20.x us).
    const bool all_new = (int64_t)EPB <= a.n - env0 &&
                         ((MODE == NGW_MODE_RESET && !a.reset_mask) || (MODE == NGW_MODE_REFILL && __all(action != 0)));
    u32x4 buf[PB];
    const u32x4* gin = reinterpret_cast<const u32x4*>(a.b.map + env0 * a.S2);
    if (!all_new) pieces_load(buf, gin, 0, npieces, tid);
    if (live) {
        if (!all_new) {
            const int2 rc = reinterpret_cast<const int2*>(a.b.loc)[e];
            r = rc.x; c = rc.y;
            f = a.b.facing[e];
        }
        if (MODE != NGW_MODE_REFILL) {
            if (!all_new) {
                sel = a.b.selected[e];
                steps = a.b.step_count[e];
            }
            episode = a.b.episode[e];
        }
        if (MODE == NGW_MODE_RESET) action = a.reset_mask ? (int)a.reset_mask[e] : 1;
    }
    u32x4 iq[IQ];
    if (!all_new) {
        const u32x4* gi = reinterpret_cast<const u32x4*>(a.b.inv + env0 * K);
#pragma unroll
        for (int j = 0; j < IQ; j++) iq[j] = (j * EPB < 16 * K) ? gi[min(tid + EPB * j, 16 * K - 1)] : u32x4{0u, 0u, 0u, 0u};
    }
    STAMP(1);
    // ---- land them in LDS
    if (tid < NGW_MAX_PLACE / 4) lds[a.off_act + tid] = psv;
    if (!all_new) {
        pieces_lds<true, MAPMODE>(buf, a, lds_map, 0, npieces, tid);
        for (int base = EPB * PB; base < npieces; base += EPB * PB) {              // big maps: further rounds
            pieces_load(buf, gin, base, npieces, tid);
            pieces_lds<true, MAPMODE>(buf, a, lds_map, base, npieces, tid);
        }
        inv_lds<true>(iq, a, lds_inv, tid);
    }
    if (LIDAR && tid < LIDAR_ITEM_DW) lds[a.off_litem + tid] = lit;
    __syncthreads();
    STAMP(2);

    uint32_t flags = 0;
    g_u32x4* gmap = (g_u32x4*)(reinterpret_cast<u32x4*>(a.b.map + env0 * a.S2) + tid);     // the wave's coalesced chunk
    g_u32x4* ginv = (g_u32x4*)(reinterpret_cast<u32x4*>(a.b.inv + env0 * K) + tid);
    const uint64_t env_global = (uint64_t)(a.env_base + e);
    if (MODE == NGW_MODE_REFILL && blockIdx.x == 0 && tid == 0) {                  // what the host reads (without a sync) before the next refill
        uint32_t* const sh = dspec->nx.slow_host;                                 // (one report per refill: the launch of slot 0 makes it)
        if (sh && a.autoreset == 0) { sh[0] = dspec->nx.slow[0]; sh[1] = atomicAdd(dspec->nx.slow + 1, 1u) + 1u; }
    }
    STAMP(3);
    bool do_reset = live && (MODE == NGW_MODE_RESET || MODE == NGW_MODE_REFILL) && action != 0;
    bool renewed = false;                                                          // this lane's map in LDS is a new episode's
    if (do_reset) {                                                                // out of line: new_episode
        episode++;
        uint32_t rr = new_episode(dspec, (LDS_AS int8_t*)mp, (LDS_AS int32_t*)inv, (LDS_AS uint32_t*)cand, (const LDS_AS uint8_t*)(lds + a.off_act),
                                  (LDS_AS uint16_t*)(lds + a.off_perm), env_global, e, episode, MODE != NGW_MODE_REFILL,
                                  MODE != NGW_MODE_RESET);   // (an explicit reset that finds nothing prepared is not a miss)
        do_reset = !(rr & NGW_F_ROWS_STORED);                                      // from here on: "the wave must store its chunk"
        rr &= ~(uint32_t)NGW_F_ROWS_STORED;
        renewed = !(MODE == NGW_MODE_REFILL && (rr & 0xFFu));
        if (MODE == NGW_MODE_REFILL && (rr & 0xFFu)) { rr &= ~0xFFu; episode = nx_old; }   // failed placement: leave the row
                                                                                   // stale, the real reset raises the flag
        flags |= rr & 0xFFu;
        r = (int)((rr >> 8) & 0xFFu); c = (int)((rr >> 16) & 0xFFu); f = (int)(rr >> 24);
        sel = 0; steps = 0;
    }
    STAMP(4);
    // ---- a reset rewrote whole maps / inventory rows in LDS: store the wave's chunk back with coalesced 16-B pieces
    if (MODE == NGW_MODE_DBG_COPY || __any(do_reset)) {
        __syncthreads();
        for (int base = 0; base < npieces; base += EPB * PB) {
            pieces_lds<false, MAPMODE>(buf, a, lds_map, base, npieces, tid);
#pragma unroll
            for (int j = 0; j < PB; j++)
                if (base + tid + EPB * j < npieces) gmap[base + EPB * j] = buf[j];
        }
        inv_lds<false>(iq, a, lds_inv, tid);
#pragma unroll
        for (int j = 0; j < IQ; j++) { if (j * EPB < 16 * K && tid + EPB * j < 16 * K) ginv[EPB * j] = iq[j]; }
        __syncthreads();
    }
    if (live) {
        reinterpret_cast<int2*>(a.b.loc)[e] = int2{r, c};
        a.b.facing[e] = f;
        if (MODE != NGW_MODE_REFILL) {
            a.b.selected[e] = (uint8_t)sel;
            a.b.step_count[e] = steps;
        }
        a.b.episode[e] = episode;
    }
    // Boards mode (a.b.brd: the bit-row lidar is on): the occupancy bit rows of the maps this launch made, from the lane's map in LDS - one word per
    // row, bit c = cell (r, c) holds a block.  (Behind this kernel the host used to rebuild the bit rows of EVERY map with another launch: with
    // FireWall's refill every 18 steps over four prepared slots that was the larger part of a 35 us lidar step.)
    if ((MODE == NGW_MODE_RESET || MODE == NGW_MODE_REFILL) && a.b.brd && renewed) {
        GLOBAL_AS uint32_t* br = (GLOBAL_AS uint32_t*)a.b.brd + e * a.BS;
        const LDS_AS uint8_t* m8 = (const LDS_AS uint8_t*)mp;
        for (int rr_ = 0; rr_ < S; rr_++) {
            uint32_t w = 0;
            for (int cc = 0; cc < S; cc++) w |= (m8[rr_ * S + cc] != 0 ? 1u : 0u) << cc;
            br[rr_] = w;
        }
        for (int rr_ = S; rr_ < a.BS; rr_++) br[rr_] = 0u;
    }
    if (LIDAR) lidar_epilogue(a, lds, tid, live, mp + r * S + c, f, inv);          // the observation of the state this reset produced
    if (flags) atomicOr(a.b.flags, flags);
    raise_host_flags(a.b.flags_host, flags);
    if (MODE == NGW_MODE_RESET) {
        if (a.seq) mirror_wave(dspec, a.b, a.S2, a.K, a.n);
        signal_host_seq(a.b.flags_host, a.seq);
    }
#ifdef NGW_STAMPS
    STAMP(5);
    __builtin_amdgcn_s_waitcnt(0);                                                 // every store acknowledged
    STAMP(6);
    STAMP_FLUSH(a);
#endif
}

__global__ void ngw_nop_kernel(const NgwDevSpec* dspec, const NgwLaunch a) {}

// the general new-episode kernel: explicit resets (with or without the fused lidar observation), refills, diagnostics
template <int MAPMODE>
hipError_t launch_general(const NgwDevSpec* dspec, const NgwLaunch* a, bool lidar, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    const dim3 g(grid), b(NGW_EPB);
    switch (a->mode) {
    case NGW_MODE_RESET:
        return with_flag(lidar, [&](auto L) { return launch_kernel<ngw_kernel<MAPMODE, NGW_MODE_RESET, decltype(L)::value>>(g, b, lds_bytes, stream, dspec, *a); });
    case NGW_MODE_REFILL: return launch_kernel<ngw_kernel<MAPMODE, NGW_MODE_REFILL, false>>(g, b, lds_bytes, stream, dspec, *a);
    case NGW_MODE_DBG_COPY: return launch_kernel<ngw_kernel<MAPMODE, NGW_MODE_DBG_COPY, false>>(g, b, lds_bytes, stream, dspec, *a);
    case NGW_MODE_DBG_NOP: return launch_kernel<ngw_kernel<MAPMODE, NGW_MODE_DBG_NOP, false>>(g, b, lds_bytes, stream, dspec, *a);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

extern "C" hipError_t ngw_launch(const NgwDevSpec* dspec, const NgwLaunch* a, int map_mode, int feat, unsigned grid,
                                 size_t lds_bytes, hipStream_t stream) {
    if (a->mode >= NGW_MODE_DBG_WG256 && a->mode <= NGW_MODE_DBG_WG128_LDS2) {   // diagnostics: empty kernels with other workgroup shapes over the same lanes
        const unsigned tpb = a->mode == NGW_MODE_DBG_WG256 ? 256 : (a->mode == NGW_MODE_DBG_WG1024 ? 1024 : 128);
        return launch_kernel<ngw_nop_kernel>(dim3(grid * NGW_EPB / tpb), dim3(tpb), a->mode == NGW_MODE_DBG_WG128_LDS2 ? lds_bytes * 2 : 0, stream, dspec, *a);
    }
    if (a->mode == NGW_MODE_DBG_FLOOR)          // the launch floor: an empty kernel in the STEP kernel's launch shape (ngw_debug_launch_floor)
        return launch_kernel<ngw_nop_kernel>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, dspec, *a);
    if (a->mode == NGW_MODE_STEP) return ngw_part_step(dspec, a, map_mode, feat, grid, lds_bytes, stream);
    if (a->mode == NGW_MODE_ROLLOUT || a->mode == NGW_MODE_ROLLOUT_ACT) {
        switch (map_mode) {
        case NGW_MAP_STRAIGHT: return ngw_part_rollout_straight(dspec, a, feat, grid, lds_bytes, stream);
        case NGW_MAP_DWORD: return ngw_part_rollout_dword(dspec, a, feat, grid, lds_bytes, stream);
        default: return ngw_part_rollout_byte(dspec, a, feat, grid, lds_bytes, stream);
        }
    }
    return with_map_mode(map_mode, [&](auto MM) { return launch_general<decltype(MM)::value>(dspec, a, (feat & NGW_FEAT_LIDAR) != 0, grid, lds_bytes, stream); });
}
