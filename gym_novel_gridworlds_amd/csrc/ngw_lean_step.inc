// ngw_lean_step.inc - the per-launch step kernel (included by ngw_lean.inc): prologue, lean_body, two tails, the bit-row lidar epilogue, the host write-through
// form, and its launcher.

// ---------------------------------------------------------------- host write-through (NgwWT: ngw_step_host_packed's steady state)
// The step kernel's HW form stores what the step changes straight into the caller's page-locked block (mapped into the GPU's address space):
// lean_body's write-through sites store twice (state in HBM, mirror on the host), the tails add pose / reward / done / info of every env
// and - cold tail - the whole rows of the envs that started a new episode.  Every block then counts itself done; the last one publishes the
// error flags and the launch's sequence number, which the host polls instead of synchronising the stream.
__device__ __forceinline__ NgwWT load_wt(const NgwDevSpec* dspec) {
    const GLOBAL_AS uint64_t* wp = (const GLOBAL_AS uint64_t*)&dspec->wt;          // uniform: scalar loads
    uint64_t w[9];
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = wp[i];
    NgwWT W;
    __builtin_memcpy(&W, w, sizeof(W));
    return W;
}
static_assert(sizeof(NgwWT) == 72, "NgwWT is fetched as 9 qwords");

__device__ __forceinline__ void wire_outputs(const NgwWT& W, uint32_t bid, uint32_t tid, bool live, int r, int c, int f, int sel, int reward, int ended, uint32_t info) {
    if (live) {                                                                    // (the block's sections are n long, not n_pad)
        const uint32_t pose = (uint32_t)(r & 255) | ((uint32_t)(c & 255) << 8) | ((uint32_t)(f & 255) << 16) | ((uint32_t)sel << 24);
        stgs<uint32_t>(reinterpret_cast<char*>(W.pose) + (uint64_t)bid * (EPB * 4), tid * 4u, pose);
        stgs<int>(reinterpret_cast<char*>(W.reward) + (uint64_t)bid * (EPB * 4), tid * 4u, reward);
        stgs<uint8_t>(reinterpret_cast<char*>(W.done) + (uint64_t)bid * EPB, tid, (uint8_t)ended);
        stgs<uint32_t>(reinterpret_cast<char*>(W.info) + (uint64_t)bid * (EPB * 4), tid * 4u, info);
    }
}

// cold tail: the envs that started a new episode had their map and inventory rows rewritten in HBM by this wave (prepared-episode copies or
// the inline placement): the rows are read back (agent-scope loads: nothing stale) and stored into the mirror, one env after the other
__device__ __forceinline__ void wire_rows(const NgwWT& W, const NgwLaunch& c, int do_reset, uint32_t tid, uint32_t gbid) {
    uint64_t m = __ballot(do_reset != 0);
    const int S2 = c.S2, K = c.K;
    while (m) {
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint64_t env = (uint64_t)gbid * EPB + (uint64_t)l;
        const int8_t* src = c.b.map + env * (uint64_t)S2;
        int8_t* dst = W.map + env * (uint64_t)S2;
        if ((S2 & 3) == 0) {
            for (int i = (int)tid; i < (S2 >> 2); i += EPB)
                __hip_atomic_store(reinterpret_cast<uint32_t*>(dst) + i, __hip_atomic_load(reinterpret_cast<const uint32_t*>(src) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            for (int i = (int)tid; i < S2; i += EPB)
                __hip_atomic_store(dst + i, __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if ((int)tid < K)
            __hip_atomic_store(W.inv + env * (uint64_t)K + tid, __hip_atomic_load(c.b.inv + env * (uint64_t)K + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__device__ __forceinline__ void wire_done(const NgwWT& W, const uint32_t* dev_flags, uint32_t seq, uint32_t nblocks, uint32_t tid) {
    __builtin_amdgcn_s_waitcnt(0);                                                 // this wave's stores are acknowledged: the ones into the host's memory went out at system scope (stgs), i.e. they have left the chip
    if (tid == 0) {
        const uint32_t old = __hip_atomic_fetch_add(W.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == nblocks - 1u) {                                                 // the launch's last block: every other block's stores went out before its count
            __hip_atomic_store(W.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t fl = __hip_atomic_load(dev_flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(W.flags, fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(W.flags + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// VIEW: the fused AgentMap window (ngw_agent_view_kernel's observation, ngw_agent_view_fuse) - after the step's stores and, where the launch started
// new episodes, after the cold path has put their rows in place, the wave builds the W x W windows (W = 2 * V + 1, unrotated, 0 outside the map) of
// its 64 envs.  Wave-cooperative, the shape of traj_view_rows (ngw_traj.inc): the 64 windows are ONE aligned run of 16 * W * W dwords of the view
// buffer and lane l builds dwords l, l + 64, ... of it - consecutive addresses across the wave whatever W is; a dword lies in at most two envs'
// windows (W * W >= 9) and their agent cells come from the owner lanes with ds_bpermute.  The map bytes are read from HBM where the step left them:
// four dwords' sixteen byte loads are issued together, on coordinates clamped into the map (the value of a cell outside it is dropped), so a
// round costs one trip to the L1 / L2 the step has just filled.
//
// Visibility.  A lane reads cells that OTHER lanes of its wave stored in this launch (the step's cell write, an entity pick-up, a new episode's
// row).  Writer and reader are the same wavefront, so the same CU and the same vector L1, which is write-through and coherent with its own CU's
// stores: what is needed is that the stores have completed before the loads are issued - a workgroup-scope fence, which on this target is the
// wait for the vector-memory counter and no cache operation (the LLVM AMDGPU memory model, gfx942 family, non-tgsplit: "no special action for
// coherence between wavefronts in the same work-group").  The explicit s_waitcnt behind it is the wait itself, in case the fence's own is elided.
// Nothing here is visible to another CU before the kernel ends, and nothing needs to be: the buffer's readers are later launches.
__device__ __forceinline__ void view_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// every lane of the wave calls it (ds_bpermute inside); maps: the wave's 64 map rows; gbid: the wave's block in the whole batch; r, c: this lane's agent cell
__device__ __forceinline__ void view_rows(const NgwLaunchView& v, const char* maps, int S, int S2, uint32_t gbid, uint32_t tid, bool live, int r, int c) {
    const int V = v.V;
    const uint32_t W = 2u * (uint32_t)V + 1u, WW = W * W, nd = 16u * WW;          // the wave's tile: 64 * W * W bytes
    const uint32_t d0 = gbid * nd;                                                 // (the buffer is below 4 GiB: ngw_agent_view_fuse)
    const uint32_t left = v.n_dwords - min(d0, v.n_dwords);                        // the buffer ends with env n - 1, inside the last wave's tile
    const int pose = live ? (r | (c << 8) | (1 << 16)) : 0;
    GLOBAL_AS uint32_t* const g = (GLOBAL_AS uint32_t*)v.view + d0;
#ifdef NGW_EXP_VIEW_PERLANE
    // (experiment build, DESIGN.md 4.20: the rejected shape - every lane builds its own env's window, byte by byte; rows start at any byte)
    GLOBAL_AS uint8_t* const gb = (GLOBAL_AS uint8_t*)g + tid * WW;
    if (live) {
        for (uint32_t wr = 0; wr < W; wr++) {
            for (uint32_t wc = 0; wc < W; wc++) {
                const int mr = r + (int)wr - V, mc = c + (int)wc - V;
                const bool in = (unsigned)mr < (unsigned)S && (unsigned)mc < (unsigned)S;
                const uint32_t cell = ldgg<uint8_t>(maps, tid * (uint32_t)S2 + (uint32_t)(in ? mr * S + mc : 0));
                gb[wr * W + wc] = (uint8_t)(in ? cell : 0u);
            }
        }
    }
    (void)left; (void)pose;
#else
    constexpr int U = 4;                                                           // dwords per lane and round: 16 byte loads in flight
    for (uint32_t base = 0; base < nd; base += U * EPB) {                          // (a wave-uniform trip count: ds_bpermute reads every lane)
        uint32_t word[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t p = base + (uint32_t)(u * EPB) + tid;
            const uint32_t idx = min(p, nd - 1u) * 4u;                             // this dword's first byte in the tile
            const uint32_t e = __umulhi(idx, v.magicWW);                           // ... lies in env e of the wave (and its last one in e or e + 1)
            uint32_t rem = idx - e * WW;
            const int p0 = __builtin_amdgcn_ds_bpermute((int)(e << 2), pose);
            const int p1 = __builtin_amdgcn_ds_bpermute((int)(min(e + 1u, (uint32_t)EPB - 1u) << 2), pose);
            uint32_t cur = 0, w = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t wr = __umulhi(rem, v.magicW), wc = rem - wr * W;
                const int pz = cur ? p1 : p0;
                const int mr = (pz & 255) + (int)wr - V, mc = ((pz >> 8) & 255) + (int)wc - V;
                const bool in = (pz >> 16) && (unsigned)mr < (unsigned)S && (unsigned)mc < (unsigned)S;
                const uint32_t en = min(e + cur, (uint32_t)EPB - 1u);              // (the tile's last byte ends env 63: nothing is read behind it)
                const uint32_t cell = ldgg<uint8_t>(maps, en * (uint32_t)S2 + (uint32_t)(in ? mr * S + mc : 0));
                w |= (in ? cell : 0u) << (8 * j);
                if (++rem == WW) { rem = 0; cur = 1; }
            }
            word[u] = w;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t p = base + (uint32_t)(u * EPB) + tid;
            if (p < nd && p < left) g[p] = word[u];
        }
    }
#endif
}

// MASK: the fused action masks - after the step, every lane evaluates the mask of the state it leaves (the post-step pose and cells, or the
// new episode's first state where the launch started one) with lane_mask (ngw_mask.inc) and stores it to NgwDevSpec::amask.  Plain steps
// only (no lidar epilogue, no host write-through): with those the library runs the standalone mask kernel behind the step.
//
// PLAIN: the instantiation for the plain spec class (ngw_step_plain_class, ngw_device.h: in place, nothing fused, K <= 12, no Jump action, no
// entities, one "near" item, every array within 4 GB of the slab's base) and launches that bring the caller's int32 action row.  What the class
// never has is not compiled: three inventory chunks instead of six, one action load and no select, no Jump cell / entity block / second
// neighbourhood test in lean_body.  A `PLAIN ? x : y` below picks at compile time: the general form compiles y alone.  Every address is the ONE preloaded
// scalar base plus a 32-bit lane offset that already holds the block's share, so no 64-bit scalar base is built per array.
template <int MAPMODE, bool STAGE, bool EXT, bool LIDAR, int NR = 0, bool HW = false, bool MASK = false, bool PLAIN = false, bool VIEW = false>
__global__ void __launch_bounds__(NGW_EPB) ngw_step_lean(char* sbase, const int32_t* actions, uint32_t n32, uint32_t o_brd, const NgwDevSpec* __restrict__ dspec,
                                                         uint32_t o_inv, uint32_t o_loc, uint32_t o_fac, uint32_t o_sel, uint32_t o_stp, uint32_t s2k,
                                                         const std::conditional_t<VIEW, NgwLaunchView, NgwLaunch> a) {
    static_assert(!VIEW || (!STAGE && !LIDAR && !HW && !MASK), "the fused AgentMap window is the in-place step's, with nothing else fused");
    static_assert(!LIDAR || STAGE || NR > 0, "the fused LidarInFront epilogue marches over the map in LDS, or reads NR bit rows");
    static_assert(!HW || !STAGE, "the host write-through form is the in-place kernel's");
    static_assert(!MASK || (!LIDAR && !HW), "the fused masks are the plain step's");
    static_assert(!PLAIN || (!STAGE && !EXT && !LIDAR && !HW && !MASK), "the plain class: in place, nothing fused");
    constexpr bool BRD = LIDAR && !STAGE;
    constexpr int NQ = PLAIN ? 3 : IQ;                                             // 16-byte chunks of an inventory row (PLAIN: K <= 12)
    using TR = std::conditional_t<PLAIN, LeanPlain, LeanFull>;
    constexpr int NRR = NR > 0 ? NR : 4;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    STAMP_DECL;
    STAMP(0);
    // Addresses are a per-block SCALAR base (SGPR pair) + a 32-bit per-lane offset: no 64-bit vector arithmetic anywhere.
    // PLAIN: ONE scalar base, the slab's, for every state array; the array's offset and the block's share are in the lane's 32-bit offset
    // (the launcher checked the spans).
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)n32;
    const int S2 = (int)(s2k & 0xFFFFu), K = (int)((s2k >> 16) & 0xFFu);
    const int Sb = (int)(s2k >> 24), BSb = (Sb + 3) & ~3;                           // (map size and board stride: the prologue's board loads need them)
    const int npieces = 4 * S2;
    // every state array is n_pad long  (PLAIN: n < 2^32 and bid * 64 < n: 32 bits hold the difference)
    const int nlive = PLAIN ? (int)min((uint32_t)EPB, n32 - bid * (uint32_t)EPB) : (int)min((int64_t)EPB, n - (int64_t)bid * EPB);
    const bool live = (int)tid < nlive;
    char* const bmap = PLAIN ? sbase : sbase + (uint64_t)bid * (uint32_t)(EPB * S2);
    char* const binv = PLAIN ? sbase : sbase + 16ull * o_inv + (uint64_t)bid * (uint32_t)(EPB * 4 * K);
    char* const bloc = PLAIN ? sbase : sbase + 16ull * o_loc + (uint64_t)bid * (EPB * 8);
    char* const bfac = PLAIN ? sbase : sbase + 16ull * o_fac + (uint64_t)bid * (EPB * 4);
    char* const bsel = PLAIN ? sbase : sbase + 16ull * o_sel + (uint64_t)bid * EPB;
    char* const bstp = PLAIN ? sbase : sbase + 16ull * o_stp + (uint64_t)bid * (EPB * 4);
    char* const bbrd = sbase + 16ull * o_brd + (uint64_t)bid * (uint32_t)(EPB * 4 * BSb);
    const uint32_t brow = tid * 4u * (uint32_t)BSb;                                // this lane's bit rows inside the block's chunk
    const char* const bact = PLAIN ? reinterpret_cast<const char*>(actions) : reinterpret_cast<const char*>(actions) + (uint64_t)bid * (EPB * 4);

    // ---- every global load of the launch, issued back to back.  The small per-env loads go FIRST: vmcnt retires in issue
    //      order, so the action's descriptor fetch (ds_bpermute), the address arithmetic and the inventory rows' way into
    //      LDS proceed while the 7 KB of map pieces are still in flight.
    const uint32_t oloc = PLAIN ? 16u * o_loc + bid * (uint32_t)(EPB * 8) + tid * 8u : tid * 8u;
    const int2 rc = ldg<int2>(bloc, oloc);
    const uint32_t ofac = PLAIN ? 16u * o_fac + bid * (uint32_t)(EPB * 4) + tid * 4u : tid * 4u;
    const int f = ldg<int>(bfac, ofac);
    const uint32_t oact = 4u * ((PLAIN ? bid * (uint32_t)EPB : 0u) + (uint32_t)min((int)tid, nlive - 1));   // the caller's array is n long
    const int action_ld = ldg<int>(bact, oact);
    // (the host step's narrow wire format, use_action0 == 2: the same buffer holds ONE BYTE per env - ngw_step_host_packed's own
    //  page-locked staging, 4 n bytes long, read in place across PCIe; both loads go out, the launch block says which one counts)
    //  (PLAIN: the launcher sends only int32 rows here)
    int action = action_ld;
    if constexpr (!PLAIN) {
        const int action_u8 = ldg<uint8_t>(reinterpret_cast<const char*>(actions) + (uint64_t)bid * EPB, (uint32_t)min((int)tid, nlive - 1));
        action = a.use_action0 == 1 ? a.action0 : (a.use_action0 == 2 ? action_u8 : action_ld);   // (1: one-env handles, the action came with the arguments)
    }
    const uint32_t osel = PLAIN ? 16u * o_sel + bid * (uint32_t)EPB + tid : tid;
    const int sel = ldg<uint8_t>(bsel, osel);
    const uint32_t ostp = PLAIN ? 16u * o_stp + bid * (uint32_t)(EPB * 4) + tid * 4u : tid * 4u;
    const int steps0 = ldg<int>(bstp, ostp);
    // lane l holds the micro-op entry of action l (zeros beyond the table: what an invalid action id fetches)
    uint32_t t0, t1, t2, t3, t4, t5;
    {   // (lanes beyond the table hold a copy of its last entry: no lane fetches from them - an invalid action id reads lane 63's
        //  zeros, see below - and an unconditional load needs no exec-mask bracket)
        const uint2* ld = reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(dspec->act_lean) + min(tid, (uint32_t)(NGW_MAX_ACTIONS - 1)) * (4u * NGW_LEAN_DW));
        const uint2 x0 = ld[0], x1 = ld[1], x2 = ld[2];
        const bool in_table = tid < NGW_MAX_ACTIONS;
        t0 = in_table ? x0.x : 0u; t1 = in_table ? x0.y : 0u; t2 = in_table ? x1.x : 0u; t3 = in_table ? x1.y : 0u; t4 = in_table ? x2.x : 0u; t5 = in_table ? x2.y : 0u;
    }
    // this lane's inventory row inside the block's chunk  (PLAIN: inside the slab; built while the loads above are in flight)
    const uint32_t rowoff = (PLAIN ? 16u * o_inv + bid * (uint32_t)(EPB * 4 * K) : 0u) + tid * 4u * (uint32_t)K;
    // 16-B chunks of the inventory row, every one clamped to the row end (K >= 4): a chunk beyond the row re-reads the last one -
    // ALL of them unconditionally.  (A uniform "K <= 12: skip the upper three" around the loads looked cheaper and cost a full
    // memory round trip: the values of the skipped chunks were merged with copies of chunk 2 where the branch ends, behind a
    // wait for every load issued so far - and the map pieces below went out only after that.)
    u32x4 q[NQ];
    const bool inv_short = PLAIN || K <= 12;
#pragma unroll
    for (int j = 0; j < NQ; j++) q[j] = ldg<u32x4>(binv, rowoff + 4u * (uint32_t)min(4 * j, K - 4));
    u32x4 buf[PB];
    if (STAGE) {
#pragma unroll
        for (int j = 0; j < PB; j++) buf[j] = ldg<u32x4>(bmap, 16u * (uint32_t)min((int)tid + EPB * j, npieces - 1));
    }
    u32x4 bq[NRR / 4];                                                             // the lane's occupancy bit rows (rows >= S are zero words)
    if (BRD) {
#pragma unroll
        for (int j = 0; j < NRR / 4; j++) bq[j] = ldg<u32x4>(bbrd, brow + 16u * (uint32_t)min(j, BSb / 4 - 1));
    }
    __builtin_amdgcn_sched_barrier(0);                                             // (the order above is the order the data is needed in)
    NgwStepU U;                                                                    // uniform: 16 dwords, one scalar load
    {
        const uint32_t* up = reinterpret_cast<const uint32_t*>(&dspec->u);
        uint32_t uw[16];
#pragma unroll
        for (int i = 0; i < 16; i++) uw[i] = up[i];
        __builtin_memcpy(&U, uw, sizeof(U));
    }
    static_assert(sizeof(NgwStepU) == 64, "NgwStepU is fetched as 16 dwords");
    static_assert(sizeof(NgwExtU) == 36, "NgwExtU is fetched as 9 dwords");
    NgwExtU X = {};                                                                // wrapper predicates (FireWall, FenceRestriction, Crate): 9 more dwords
    if (EXT) {
        const uint32_t* xp = reinterpret_cast<const uint32_t*>(&dspec->x);
        uint32_t xw[9];
#pragma unroll
        for (int i = 0; i < 9; i++) xw[i] = xp[i];
        __builtin_memcpy(&X, xw, sizeof(X));
    }
    NgwWT W = {};                                                                  // host write-through: the mirror's sections (8 more qwords)
    if (HW) W = load_wt(dspec);
    char* const hmap = HW ? reinterpret_cast<char*>(W.map) + (uint64_t)bid * (uint32_t)(EPB * S2) : nullptr;
    char* const hinv = HW ? reinterpret_cast<char*>(W.inv) + (uint64_t)bid * (uint32_t)(EPB * 4 * K) : nullptr;
    uint32_t lit = 0;                                                              // fused lidar: the two item tables (12 dwords; lanes beyond re-read the last)
    if (LIDAR) lit = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[min(tid, (uint32_t)(LIDAR_ITEM_DW - 1))];
    uint32_t lid0 = 0, lid1 = 0;                                                   // bit-row form: the first eight item ids of the observation's inventory tail (uniform)
    if (BRD) { const uint32_t* ip = reinterpret_cast<const uint32_t*>(a.lcfg->inv_item); lid0 = ip[0]; lid1 = ip[1]; }
    STAMP(1);
    if (LIDAR) lidar_zero_tile(a, lds, (int)tid);                                  // (while the loads above are in flight)

    // ---- land maps and inventory rows in LDS
    uint32_t* lds_map = lds + a.off_map;
    int8_t* mp = reinterpret_cast<int8_t*>(lds_map) + tid * a.MS;                 // this lane's map
    int32_t* inv = reinterpret_cast<int32_t*>(lds + a.off_inv) + tid * a.KP;       // this lane's inventory row
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int o = min(4 * j, K - 4);
        inv[o] = (int)q[j].x; inv[o + 1] = (int)q[j].y; inv[o + 2] = (int)q[j].z; inv[o + 3] = (int)q[j].w;
    }
    if (!inv_short) {
#pragma unroll
        for (int j = 3; j < NQ; j++) {
            const int o = min(4 * j, K - 4);
            inv[o] = (int)q[j].x; inv[o + 1] = (int)q[j].y; inv[o + 2] = (int)q[j].z; inv[o + 3] = (int)q[j].w;
        }
    }
    // this lane's entry out of the lane that holds it; an action id outside [0, n_actions) fetches the all-zero no-op
    const bool valid = live && (uint32_t)action < (uint32_t)U.n_actions;          // reference: ValueError before any change (:236)
    const int ai = (valid ? action : 63) << 2;
    const uint32_t e0 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t0), e1 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t1);
    const uint32_t e2 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t2), e3 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t3);
    const uint32_t e4 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t4), e5 = (uint32_t)__builtin_amdgcn_ds_bpermute(ai, (int)t5);
    if (STAGE) {
        pieces_lds<true, MAPMODE>(buf, a, lds_map, 0, npieces, tid);
        for (int base = EPB * PB; base < npieces; base += EPB * PB) {              // big maps: further rounds
#pragma unroll
            for (int j = 0; j < PB; j++) buf[j] = ldg<u32x4>(bmap, 16u * (uint32_t)min(base + (int)tid + EPB * j, npieces - 1));
            pieces_lds<true, MAPMODE>(buf, a, lds_map, base, npieces, tid);
        }
    }
    if (LIDAR) lds[a.off_litem + min(tid, (uint32_t)(LIDAR_ITEM_DW - 1))] = lit;
    if (STAGE) __syncthreads();                                                    // (no-stage: every LDS row is lane-private; the lidar's shared pieces are fenced where they are read)
    STAMP(2);

    STAMP(3);
    // Bit rows: the lane's NR words came with the prologue loads.  While the step's cell reads are in flight (the hook below runs right after
    // they are issued): the rows go into the lane's LDS scratch, from where the rows the agent can stand in after this step - its own, the
    // one in front (also the row a cell write of this step changes), two ahead (Jump) - come back by index; and every row is rotated by its
    // own index, right (Rd) and left (Ra), so that the agent's diagonal and anti-diagonal are ONE bit position in every row of them.
    const int bdr = (f == 0) ? -1 : (f == 1 ? 1 : 0), bdc = (f == 2) ? -1 : (f == 3 ? 1 : 0);
    const int bfr = min(max(rc.x + bdr, 0), Sb - 1), bfc = min(max(rc.y + bdc, 0), Sb - 1), bfr2 = min(max(rc.x + 2 * bdr, 0), Sb - 1);
    uint32_t wr0 = 0, wr1 = 0, wr2 = 0;
    uint32_t R[NRR], Rd[NRR], Ra[NRR];
    auto brd_hook = [&]() {
        if (BRD) {
            board_unpack<NRR>(bq, R);
            LDS_AS uint32_t* bl = (LDS_AS uint32_t*)(lds + a.off_ltab) + tid * (NRR + 4);
#pragma unroll
            for (int j = 0; j < NRR / 4; j++) *(LDS_AS u32x4*)(bl + 4 * j) = bq[j];
            wr0 = bl[min(max(rc.x, 0), Sb - 1)]; wr1 = bl[bfr]; wr2 = bl[bfr2];
#pragma unroll
            for (int k = 1; k < NRR; k++) {
                Rd[k] = __builtin_amdgcn_alignbit(R[k], R[k], (uint32_t)k);            // rotate right by k: bit j <- bit (j + k) mod 32
                Ra[k] = __builtin_amdgcn_alignbit(R[k], R[k], (uint32_t)(32 - k));     // rotate left by k:  bit j <- bit (j - k) mod 32
                PIN_V(Rd[k]); PIN_V(Ra[k]);
            }
            PIN_V(wr0); PIN_V(wr1); PIN_V(wr2);
        }
    };
    const uint32_t mapoff = (PLAIN ? bid * (uint32_t)(EPB * S2) : 0u) + tid * (uint32_t)S2;                     // this lane's map, likewise
    const LeanOut o = lean_body<STAGE, true, EXT, HW, TR>(U, X, e0, e1, e2, e3, e4, e5, live, valid, PLAIN ? Sb : a.S, K, mp, inv, bmap, binv, mapoff, rowoff,
                                                 rc.x, rc.y, f, sel, steps0, a.autoreset, a.horizon, brd_hook, hmap, hinv);
    uint32_t flags = o.flags;
    STAMP(4);
    // ---- the step's cell writes, repeated on the bit rows (write-through, like the cells themselves)
    uint32_t roww = 0;                                                             // the bit row of the row the agent stands in now
    if (BRD) {
        const uint32_t fbit = 1u << bfc;
        const uint32_t wr1n = o.wcell ? (o.cellv ? wr1 | fbit : wr1 & ~fbit) : wr1;
        if (o.wcell) stg<uint32_t>(bbrd, brow + 4u * (uint32_t)bfr, wr1n);
        roww = o.r == bfr ? wr1n : (o.r == rc.x ? wr0 : wr2);                      // (facing east / west all three are the agent's own row: wr1n is the current one)
        if (__any(o.grab != 0u)) {                                                 // grab_entities picked blocks up around the NEW position: up to three rows change
            uint32_t g[3];
#pragma unroll
            for (int dy = 0; dy < 3; dy++) g[dy] = ldg<uint32_t>(bbrd, brow + 4u * (uint32_t)min(max(o.r + dy - 1, 0), Sb - 1));
#pragma unroll
            for (int dy = 0; dy < 3; dy++) {
                const uint32_t m = ((o.grab >> (3 * dy)) & 7u) << (uint32_t)max(o.c - 1, 0);
                g[dy] &= ~m;
                if (m) stg<uint32_t>(bbrd, brow + 4u * (uint32_t)min(max(o.r + dy - 1, 0), Sb - 1), g[dy]);
            }
            if (o.grab) roww = g[1];
        }
    }
    STAMP(5);
    // (every state / output array is n_pad long: lanes beyond n write their own padding rows - zeros - instead of being masked off)
    if constexpr (PLAIN) {                                                         // (n_pad * 4 < 2^32: the block's share fits the lane offset)
        stg<int>(a.b.reward, bid * (uint32_t)(EPB * 4) + tid * 4u, o.reward);
        stg<uint8_t>(a.b.done, bid * (uint32_t)EPB + tid, (uint8_t)o.ended);
        stg<uint32_t>(a.b.info, bid * (uint32_t)(EPB * 4) + tid * 4u, o.info);
    } else {
        stg<int>(reinterpret_cast<char*>(a.b.reward) + (uint64_t)bid * (EPB * 4), tid * 4u, o.reward);
        stg<uint8_t>(reinterpret_cast<char*>(a.b.done) + (uint64_t)bid * EPB, tid, (uint8_t)o.ended);
        stg<uint32_t>(reinterpret_cast<char*>(a.b.info) + (uint64_t)bid * (EPB * 4), tid * 4u, o.info);
    }
    // Two tails, so that NO scalar of the hot path is live across the cold region (the register allocator otherwise parks half of
    // them in VGPR lanes from the prologue on: 50 v_writelane / 66 v_readlane in round 3's kernel, on a path bound by issue):
    //   * no lane resets (99 launches in 100 at H = 100): pose stores, epilogue, done;
    //   * some lane resets: everything from here on reads its uniform arguments from the HBM blob's copy of the launch block
    //     (NgwDevSpec::lp / lp_ns: scalar loads inside the cold region) - what crosses over is per-lane data in VGPRs, the spec
    //     pointer and the launch's sequence number.
    if (!__any(o.do_reset)) {
        // fused LidarInFront observation of the state this step produced (observation_wrappers.py:67-78): map and inventory row are in LDS
        stg<int2>(bloc, oloc, int2{o.r, o.c});
        stg<int>(bfac, ofac, o.f);
        stg<uint8_t>(bsel, osel, (uint8_t)o.sel);
        stg<int>(bstp, ostp, o.steps);
        if (HW) wire_outputs(W, bid, tid, live, o.r, o.c, o.f, o.sel, o.reward, o.ended, o.info);
        // (tried: the output and pose stores AFTER the epilogue, in case the epilogue's register re-use waited for their acknowledgement -
        //  no gain, 8.05 against 7.8 us per step; the stores stay where they overlap the epilogue)
        if (LIDAR && STAGE) lidar_epilogue(a, lds, (int)tid, live, mp + o.r * a.S + o.c, o.f, inv, true);   // (tile zeroed in the prologue; no cold path ran)
        if (BRD) {
            // the agent's column and diagonals out of the bit rows that came with the prologue; what this step changed on them is patched in:
            // a cell write sits in front of an agent that did not move (its column when it faces north / south; its row is `roww`), an entity
            // pick-up clears cells one step away on every line
            STAMP_SUB(a, 0);
            const int nr = live ? o.r : 1, nc = live ? o.c : 1;                    // (rows beyond n hold zeros: a pose inside the map keeps every read in bounds)
            BoardPatch pt = {0u, 0u, 0u, 0u};
            if (o.wcell && bfc == nc) { if (o.cellv) pt.col_set = 1u << bfr; else pt.col_clr = 1u << bfr; }
            if (o.grab) {
                const uint32_t up = 1u << (nr + 1), dn = 1u << (nr - 1), gm = o.grab;
                pt.col_clr |= (((gm >> 1) & 1u) ? dn : 0u) | (((gm >> 7) & 1u) ? up : 0u);
                pt.dg_clr = ((gm & 1u) ? dn : 0u) | (((gm >> 8) & 1u) ? up : 0u);
                pt.an_clr = (((gm >> 2) & 1u) ? dn : 0u) | (((gm >> 6) & 1u) ? up : 0u);
            }
            const uint32_t ring = 1u | (1u << (Sb - 1));
            wave_lds_sync();                                                       // (the tile was zeroed, the item tables written, by other lanes)
            lidar_boards_rows<NRR>(a, lds, (int)tid, R, Rd, Ra, roww | ring, pt, Sb, S2, nr, nc, o.f, bmap, mapoff, inv, lid0, lid1, bid, HW ? W.rows : nullptr);
        }
        if (MASK) {                                                                // the post-step state: pose in registers, map in LDS (staged) or
            const uint32_t mo = mapoff;                                            //   HBM (this lane's own writes), inventory row in LDS
            auto cell = [&](int q) -> int { return STAGE ? (int)mp[q] : (int)ldg<int8_t>(bmap, mo + (uint32_t)q); };
            const uint64_t m = lane_mask<EXT>(dspec, a.S, K, live ? o.r : 1, live ? o.c : 1, live ? o.f : 0, o.sel, inv, cell);
            uint64_t* const am = dspec->amask;
            if (am) stg<uint64_t>(reinterpret_cast<char*>(am) + (uint64_t)bid * (EPB * 8), tid * 8u, live ? m : 0ull);
        }
        if constexpr (VIEW) {                                                      // the post-step state: this wave's cell writes are in HBM behind view_sync
            view_sync();
            view_rows(a, PLAIN ? bmap + (uint64_t)bid * (uint32_t)(EPB * S2) : bmap, PLAIN ? Sb : a.S, S2, bid, tid, live, o.r, o.c);
        }
        if (HW) {
            step_signals(dspec, flags, 0u);
            wire_done(W, a.b.flags, a.seq, gridDim.x, tid);
        } else step_signals(dspec, flags, a.seq);
#ifdef NGW_STAMPS
        STAMP(6);
        __builtin_amdgcn_s_waitcnt(0);
        STAMP(7);
        STAMP_FLUSH(a);
#endif
        return;
    }
    {
        const NgwLaunch c = STAGE ? dspec->lp : dspec->lp_ns;                      // uniform: scalar loads (the fields used below)
        const uint32_t seq = a.seq;
        // A launch may cover a SLICE of the batch (ngw_step_host_packed pipelines its step through slices): the hot path above works on
        // base pointers the host shifted to the slice's first env, this region on the blob's own (unshifted) arrays - with the slice's
        // first block added to the block index
        const uint32_t gbid = bid + a.bid0;
        const int do_reset = o.do_reset ? 1 : 0;
        terminal_capture(dspec, c, do_reset, (int)tid, o.r, o.c, o.f, gbid);
        const uint32_t rr = STAGE ? lean_cold<MAPMODE, !LIDAR>(dspec, c, do_reset, gbid) : lean_cold_ns(dspec, c, do_reset, gbid);
        int ro = o.r, co = o.c, fo = o.f, so = o.sel, steps = o.steps;
        if (do_reset) {
            flags |= rr & 0xFFu;
            ro = (int)((rr >> 8) & 0xFFu); co = (int)((rr >> 16) & 0xFFu); fo = (int)(rr >> 24);
            so = 0; steps = 0;
        }
        stg<int2>(reinterpret_cast<char*>(c.b.loc) + (uint64_t)gbid * (EPB * 8), tid * 8u, int2{ro, co});
        stg<int>(reinterpret_cast<char*>(c.b.facing) + (uint64_t)gbid * (EPB * 4), tid * 4u, fo);
        stg<uint8_t>(reinterpret_cast<char*>(c.b.selected) + (uint64_t)gbid * EPB, tid, (uint8_t)so);
        stg<int>(reinterpret_cast<char*>(c.b.step_count) + (uint64_t)gbid * (EPB * 4), tid * 4u, steps);
        NgwWT Wc = {};
        if (HW) {                                                                  // (read again: nothing of the hot path's stays live across the cold region)
            Wc = load_wt(dspec);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");                 // the wave's own row copies are behind it
            wire_rows(Wc, c, do_reset, tid, gbid);
            wire_outputs(Wc, gbid, tid, live, ro, co, fo, so, o.reward, o.ended, o.info);
        }
        if (LIDAR && STAGE) lidar_epilogue(c, lds, (int)tid, live, mp + ro * c.S + co, fo, inv);   // (a reset has rewritten map and inventory row in LDS)
        if (BRD) {
            // the wave has rewritten map, inventory and bit rows of its resetting envs in HBM (lean_cold_ns): everything the rows are built
            // from is read again, for every lane (program order inside the wave = a workgroup-scope fence, as in terminal_capture)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            const int cS = c.S, cS2 = c.S2, cBS = c.BS, cK = c.K;
            char* const cbrd = reinterpret_cast<char*>(c.b.brd) + (uint64_t)gbid * (uint32_t)(EPB * 4 * cBS);
            char* const cmap = reinterpret_cast<char*>(c.b.map) + (uint64_t)gbid * (uint32_t)(EPB * cS2);
            char* const cinv = reinterpret_cast<char*>(c.b.inv) + (uint64_t)gbid * (uint32_t)(EPB * 4 * cK);
            const uint32_t crow = tid * 4u * (uint32_t)cBS;
            u32x4 cq[NRR / 4];
#pragma unroll
            for (int j = 0; j < NRR / 4; j++) cq[j] = ldgg<u32x4>(cbrd, crow + 16u * (uint32_t)min(j, cBS / 4 - 1));
            const int nr = live ? ro : 1, nc = live ? co : 1;
            const uint32_t rw = ldgg<uint32_t>(cbrd, crow + 4u * (uint32_t)nr);
            u32x4 iq2[IQ];                                                         // (a reset lane's inventory row changed in HBM only: the LDS row the tail reads follows)
#pragma unroll
            for (int j = 0; j < IQ; j++) iq2[j] = ldgg<u32x4>(cinv, tid * 4u * (uint32_t)cK + 4u * (uint32_t)min(4 * j, cK - 4));
#pragma unroll
            for (int j = 0; j < IQ; j++) {
                const int io = min(4 * j, cK - 4);
                inv[io] = (int)iq2[j].x; inv[io + 1] = (int)iq2[j].y; inv[io + 2] = (int)iq2[j].z; inv[io + 3] = (int)iq2[j].w;
            }
            uint32_t R2[NRR], Rd2[NRR], Ra2[NRR];
            board_unpack<NRR>(cq, R2);
            board_rotate<NRR>(R2, Rd2, Ra2);
            lidar_zero_tile(c, lds, (int)tid);                                     // (the cold path may have used the tile's LDS)
            wave_lds_sync();
            lidar_boards_rows<NRR>(c, lds, (int)tid, R2, Rd2, Ra2, rw | 1u | (1u << (cS - 1)), BoardPatch{0u, 0u, 0u, 0u}, cS, cS2, nr, nc, fo, cmap, tid * (uint32_t)cS2, inv, lid0, lid1, gbid, HW ? Wc.rows : nullptr);
        }
        if (MASK) {
            // the wave has rewritten the rows of its resetting envs in HBM (prepared-episode copies, inline placement, the staged chunk's
            // store-back): every lane reads its map and inventory row back from there (program order inside the wave = a workgroup-scope
            // fence, as in terminal_capture) and evaluates the state it leaves - the new episode's first state where it started one
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            const int cS = c.S, cS2 = c.S2, cK = c.K;
            char* const cmap = reinterpret_cast<char*>(c.b.map) + (uint64_t)gbid * (uint32_t)(EPB * cS2);
            char* const cinv = reinterpret_cast<char*>(c.b.inv) + (uint64_t)gbid * (uint32_t)(EPB * 4 * cK);
            for (int k = 0; k < cK; k++) inv[k] = ldgg<int>(cinv, tid * 4u * (uint32_t)cK + 4u * (uint32_t)k);
            const uint32_t mo = tid * (uint32_t)cS2;
            auto cell = [&](int q) -> int { return (int)ldgg<int8_t>(cmap, mo + (uint32_t)q); };
            const uint64_t m = lane_mask<EXT>(dspec, cS, cK, live ? ro : 1, live ? co : 1, live ? fo : 0, so, inv, cell);
            uint64_t* const am = dspec->amask;
            if (am) stgg<uint64_t>(reinterpret_cast<char*>(am) + (uint64_t)gbid * (EPB * 8), tid * 8u, live ? m : 0ull);
        }
        if constexpr (VIEW) {
            // the wave has rewritten the map rows of its resetting envs in HBM (prepared-episode copies or the inline placement): the windows are
            // built from there for every lane - the new episode's first state where the launch started one, the same state the pose stores above name
            view_sync();
            view_rows(a, reinterpret_cast<const char*>(c.b.map) + (uint64_t)gbid * (uint32_t)(EPB * c.S2), c.S, c.S2, gbid, tid, live, ro, co);
        }
        if (HW) {
            step_signals(dspec, flags, 0u);
            wire_done(Wc, c.b.flags, seq, gridDim.x, tid);
        } else step_signals(dspec, flags, seq);
#ifdef NGW_STAMPS
        STAMP(6);
        __builtin_amdgcn_s_waitcnt(0);
        STAMP(7);
        STAMP_FLUSH(a);
#endif
    }
}


template <int MAPMODE, bool STAGE, bool EXT, bool LIDAR, int NR = 0, bool HW = false, bool MASK = false, bool PLAIN = false, bool VIEW = false>
hipError_t launch_lean(const NgwDevSpec* dspec, const NgwLaunch* a, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    // the leading scalar arguments (see the kernel): the state slab's base and the offsets of its arrays in 16-byte units
    char* const base = reinterpret_cast<char*>(a->b.map);
    const void* const arr[5] = {a->b.inv, a->b.loc, a->b.facing, a->b.selected, a->b.step_count};
    uint32_t off[5];
    for (int i = 0; i < 5; i++) {
        const int64_t d = reinterpret_cast<const char*>(arr[i]) - base;
        if (d < 0 || (d & 15) || (d >> 4) > 0xFFFFFFFFll) return hipErrorInvalidValue;   // (not one slab: ngw_abi.cpp allocates them as one)
        off[i] = (uint32_t)(d >> 4);
    }
    if (a->S2 > 0xFFFF || a->K > 0xFF || a->S > 0xFF || a->n > 0xFFFFFFFFll) return hipErrorInvalidValue;
    uint32_t o_brd = 0;                                                            // the occupancy bit rows: part of the same slab (maps up to 32 x 32)
    if (a->b.brd) {
        const int64_t d = reinterpret_cast<const char*>(a->b.brd) - base;
        if (d < 0 || (d & 15) || (d >> 4) > 0xFFFFFFFFll) return hipErrorInvalidValue;
        o_brd = (uint32_t)(d >> 4);
    } else if (NR > 0) return hipErrorInvalidValue;
    if (NR > 0 && (a->BS > NR || a->BS < 4)) return hipErrorInvalidValue;
    const uint32_t s2k = (uint32_t)a->S2 | ((uint32_t)a->K << 16) | ((uint32_t)a->S << 24);
    if constexpr (PLAIN) {
        // the plain instantiation addresses everything as one base + 32 bits and reads the int32 row only: a launch that does not fit (a handle's
        // ngw_step_plain_class said so once; slices and other callers hand their own blocks) runs the general instantiation - never an error
        const uint64_t np = (uint64_t)a->n_pad, ends[6] = {np * (uint64_t)a->S2, 16ull * off[0] + np * 4u * (uint64_t)a->K, 16ull * off[1] + np * 8u,
                                                             16ull * off[2] + np * 4u, 16ull * off[3] + np, 16ull * off[4] + np * 4u};
        uint64_t span = 0;
        for (uint64_t e : ends) span = e > span ? e : span;
        if (!ngw_step_plain_class(a->K, 0, 0, 0, 0, span, np * 4u) || a->use_action0 != 0)
            return launch_lean<MAPMODE, STAGE, EXT, LIDAR, NR, HW, MASK, false, VIEW>(dspec, a, grid, lds_bytes, stream);
    }
    if constexpr (VIEW) {                                                          // (`a` is the NgwLaunchView the caller built: NGW_FEAT_VIEW says so)
        const NgwLaunchView& v = *static_cast<const NgwLaunchView*>(a);
        if (!v.view || v.V < 1 || v.V > NGW_VIEW_FUSE_MAX || a->bid0 != 0 || a->S2 != a->S * a->S) return hipErrorInvalidValue;
        return launch_kernel<ngw_step_lean<MAPMODE, STAGE, EXT, LIDAR, NR, HW, MASK, PLAIN, true>>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, base, a->actions, (uint32_t)a->n, o_brd,
                                                                                               dspec, off[0], off[1], off[2], off[3], off[4], s2k, v);
    } else
    return launch_kernel<ngw_step_lean<MAPMODE, STAGE, EXT, LIDAR, NR, HW, MASK, PLAIN>>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, base, a->actions, (uint32_t)a->n, o_brd, dspec,
                                                                                off[0], off[1], off[2], off[3], off[4], s2k, *a);
}

// ONE batched step(): ngw_step_lean.  The staged kernels of one map addressing mode (six each: plain and fused lidar, the plain ones also with
// fused action masks, all with and without the wrapper predicates) are a unit of their own.
template <int MM>
hipError_t step_staged(const NgwDevSpec* dspec, const NgwLaunch* a, int feat, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    const bool lidar = (feat & NGW_FEAT_LIDAR) != 0, ext = (feat & NGW_FEAT_EXT) != 0;
    if ((feat & NGW_FEAT_MASK) && !lidar)   // fused action masks
        return with_flag(ext, [&](auto E) { return launch_lean<MM, true, decltype(E)::value, false, 0, false, true>(dspec, a, grid, lds_bytes, stream); });
    return with_flag(lidar, [&](auto L) {
        return with_flag(ext, [&](auto E) { return launch_lean<MM, true, decltype(E)::value, decltype(L)::value>(dspec, a, grid, lds_bytes, stream); });
    });
}

// in-place step + the LidarInFront observation from the occupancy bit rows (ngw_boards.inc): NR = 12 / 20 / 32 register rows; HW: with the host write-through
template <bool HW>
hipError_t step_boards(const NgwDevSpec* dspec, const NgwLaunch* a, int feat, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    if (!a->l_boards) return hipErrorInvalidValue;
    return with_board_rows(a->BS, [&](auto R) {
        return with_flag((feat & NGW_FEAT_EXT) != 0, [&](auto E) {
            return launch_lean<NGW_MAP_STRAIGHT, false, decltype(E)::value, true, decltype(R)::value, HW>(dspec, a, grid, lds_bytes, stream);
        });
    });
}
