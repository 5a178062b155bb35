// ngw_mask.inc - action masks (included by ngw_lean.inc between the step body and the step kernel): lane_mask, which the fused form of the step
// kernel (ngw_step_lean<..., MASK = true>) calls at its end, and the standalone mask kernel.
//
// The mask of env i is a 64-bit word: bit a is 1 exactly when step(a) taken from env i's current state would report info['result'] == True
// under the handle's spec, with every novelty and wrapper on it; bits >= n_actions are 0.  Nothing here restates a game rule: every bit comes
// from the predicate lean_body uses (lean_cond_bits, lean_outcome, lean_break_ext, lean_result in ngw_lean_body.inc).
//
// One lane per env, 64 envs per wave, like the step kernels.  The lane reads its pose, the block in front, its 4-neighbourhood and (Jump) the
// cell two ahead ONCE, lands its inventory row in a private LDS row, then walks the n_actions micro-op entries.  The entries are wave-uniform:
// lane l holds entry l (the step kernels' table fetch) and the loop reads entry a out of lane a with v_readlane, so every entry field is a
// scalar.  The only per-action memory reads are the recipe-input and argument slots of the LDS row (and, with FenceRestriction, the fence
// cells of a Break - fetched once per wave that breaks anything breakable).

// ---- what the mask walk and the lookahead walk (ngw_lookahead.inc) share before their loops over the entries

// The micro-op table as the step kernels fetch it: lane l holds the six words of entry l (a walk reads entry a out of lane a).
struct LeanTable { uint32_t t0, t1, t2, t3, t4, t5; };
__device__ __forceinline__ LeanTable lean_fetch_table(const NgwDevSpec* __restrict__ dspec) {
    const uint2* ld = reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(dspec->act_lean) + min(threadIdx.x, (uint32_t)(NGW_MAX_ACTIONS - 1)) * (4u * NGW_LEAN_DW));
    const uint2 x0 = ld[0], x1 = ld[1], x2 = ld[2];
    return {x0.x, x0.y, x1.x, x1.y, x2.x, x2.y};
}

// The uniform parameters and (EXT) the wrapper predicates: scalar loads.
template <bool EXT>
__device__ __forceinline__ void lean_fetch_uniforms(const NgwDevSpec* __restrict__ dspec, NgwStepU& U, NgwExtU& X) {
    {
        const uint32_t* up = reinterpret_cast<const uint32_t*>(&dspec->u);
        uint32_t uw[16];
#pragma unroll
        for (int i = 0; i < 16; i++) uw[i] = up[i];
        __builtin_memcpy(&U, uw, sizeof(U));
    }
    X = {};
    if (EXT) {
        const uint32_t* xp = reinterpret_cast<const uint32_t*>(&dspec->x);
        uint32_t xw[9];
#pragma unroll
        for (int i = 0; i < 9; i++) xw[i] = xp[i];
        __builtin_memcpy(&X, xw, sizeof(X));
    }
}

// The cells every entry looks at (lean_body's L0 reads): the block in front, its 4-neighbourhood and (Jump) the cell two ahead.
struct LeanFront {
    int dcell, fr, fc, fcell, front;
    bool okN, okS, okW, okE;
    int nbN, nbS, nbW, nbE;
    int fr2, fc2;
    bool ok2;
    int front2;
};
template <class UT, class CELL>
__device__ __forceinline__ LeanFront lean_front_cells(const UT& U, int S, int r, int c, int f, const CELL& cell_at) {
    LeanFront q;
    const int dr = (f == 0) ? -1 : (f == 1 ? 1 : 0), dc = (f == 2) ? -1 : (f == 3 ? 1 : 0);
    q.fr = r + dr; q.fc = c + dc; q.dcell = dr * S + dc; q.fcell = r * S + c + q.dcell;
    q.front = cell_at(q.fcell);
    q.okN = q.fr > 0; q.okS = q.fr < S - 1; q.okW = q.fc > 0; q.okE = q.fc < S - 1;
    q.nbN = cell_at(q.okN ? q.fcell - S : q.fcell); q.nbS = cell_at(q.okS ? q.fcell + S : q.fcell);
    q.nbW = cell_at(q.okW ? q.fcell - 1 : q.fcell); q.nbE = cell_at(q.okE ? q.fcell + 1 : q.fcell);
    q.fr2 = q.fr + dr; q.fc2 = q.fc + dc;
    q.ok2 = q.fr2 >= 0 && q.fr2 <= S - 1 && q.fc2 >= 0 && q.fc2 <= S - 1;
    q.front2 = 1;
    if (U.feat & NGW_FEAT_JUMP) q.front2 = cell_at(q.ok2 ? q.fcell + q.dcell : q.fcell);
    return q;
}

// One lane's env as the standalone kernels read it from HBM: the pose (a padding lane gets a pose inside the map - its rows are zeros),
// the selected item, where its map starts, and its inventory row landed in the lane's private LDS row.
struct LeanLane {
    bool live;                                                                     // (every state array is n_pad long: lanes beyond n read padding rows)
    int r, c, f, sel;
    const char* bmap;
    uint32_t mapoff;
    int32_t* inv;
};
__device__ __forceinline__ LeanLane lean_load_lane(const NgwBufs& b, uint32_t n32, int S, int K, int32_t* inv_lds) {
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    const int S2 = S * S, KP = K | 1;
    const int nlive = (int)min((int64_t)EPB, (int64_t)n32 - (int64_t)bid * EPB);
    LeanLane l;
    l.live = (int)tid < nlive;
    l.bmap = reinterpret_cast<const char*>(b.map) + (uint64_t)bid * (uint32_t)(EPB * S2);
    const char* const binv = reinterpret_cast<const char*>(b.inv) + (uint64_t)bid * (uint32_t)(EPB * 4 * K);
    const int2 rc = ldg<int2>(reinterpret_cast<const char*>(b.loc) + (uint64_t)bid * (EPB * 8), tid * 8u);
    const int f0 = ldg<int>(reinterpret_cast<const char*>(b.facing) + (uint64_t)bid * (EPB * 4), tid * 4u);
    l.sel = ldg<uint8_t>(reinterpret_cast<const char*>(b.selected) + (uint64_t)bid * EPB, tid);
    l.inv = inv_lds + tid * KP;
    for (int k = 0; k < K; k++) l.inv[k] = ldg<int>(binv, tid * 4u * (uint32_t)K + 4u * (uint32_t)k);
    l.r = l.live ? rc.x : 1; l.c = l.live ? rc.y : 1; l.f = l.live ? (f0 & 3) : 0;
    l.mapoff = tid * (uint32_t)S2;
    return l;
}

// lean_load_lane, gathered: pose, selected item and map base come from row `row` of the set, the inventory row goes into the lane's private LDS row
// (the slot masks of ngw_slot_observe.inc and the weighted choice of ngw_sample.inc).
__device__ __forceinline__ LeanLane lean_gather_lane(const NgwSnapRows& s, int row, bool live, int S, int K, int32_t* inv_lds) {
    const uint32_t tid = threadIdx.x;
    const int KP = K | 1;
    LeanLane l;
    l.live = live;
    l.bmap = reinterpret_cast<const char*>(s.map) + (size_t)row * (size_t)(S * S);
    l.mapoff = 0u;
    const int2 rc = reinterpret_cast<const int2*>(s.loc)[row];
    const int f0 = s.facing[row];
    l.sel = s.selected[row];
    l.inv = inv_lds + tid * KP;
    const int32_t* const ginv = s.inv + (size_t)row * (size_t)K;
    for (int k = 0; k < K; k++) l.inv[k] = ginv[k];
    l.r = rc.x; l.c = rc.y; l.f = f0 & 3;
    return l;
}

// The walk over the entries: the mask of one lane's state from its pose and selected item, its inventory row (a lane-private LDS row) and its map
// (cell_at: a cell index -> the item there), fed the table (lane l holds entry l), the uniform parameters and the wrapper predicates the caller
// holds; A = the number of entries to walk.  All lanes of the wave must be active (the loop is wave-uniform).
template <bool EXT, class UT, class CELL>
__device__ __forceinline__ uint64_t lean_mask_walk(const LeanTable& t, const UT& U, const NgwExtU& X, int A, int S, int K, int r, int c, int f, int sel,
                                                   const int32_t* inv, const CELL& cell_at) {
    const LeanFront q = lean_front_cells(U, S, r, c, f, cell_at);
    const int inv_place = inv[U.place_item], inv_axe = inv[U.axe_item];
    uint64_t mask = 0;
    for (int a = 0; a < A; a++) {
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)t.t0, a), e1 = (uint32_t)__builtin_amdgcn_readlane((int)t.t1, a);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_readlane((int)t.t2, a), e4 = (uint32_t)__builtin_amdgcn_readlane((int)t.t4, a);
        const int aarg = (e0 >> 8) & 255;
        const int inv_arg = inv[min(aarg, K - 1)];
        const int iv0 = inv[e1 & 255], iv1 = inv[(e1 >> 8) & 255], iv2 = inv[(e1 >> 16) & 255], iv3 = inv[e1 >> 24];
        bool axe_ok;
        uint32_t missing;
        const uint32_t cb = lean_cond_bits(U, e0, e2, q.front, q.front2, q.ok2, q.okN, q.okS, q.okW, q.okE, q.nbN, q.nbS, q.nbW, q.nbE, inv_place,
                                           inv_axe, inv_arg, iv0, iv1, iv2, iv3, sel, axe_ok, missing);
        const uint32_t s = lean_outcome(cb, e4);
        LeanBreakX xb = {false, false, false};
        if (EXT) xb = lean_break_ext(U, X, lean_is_break(e0), q.front, S, r, c, f, q.fr, q.fc, q.fcell, cell_at);
        mask |= (uint64_t)(lean_result(s, xb) ? 1u : 0u) << a;
    }
    return mask;
}

// The mask of one lane's env: fetches the table, the uniform parameters and the wrapper predicates itself, so that a caller has nothing of
// them live across its own work, and walks the spec's entries.
template <bool EXT, class CELL>
__device__ __forceinline__ uint64_t lane_mask(const NgwDevSpec* __restrict__ dspec, int S, int K, int r, int c, int f, int sel, const int32_t* inv,
                                              const CELL& cell_at) {
    const LeanTable t = lean_fetch_table(dspec);
    NgwStepU U;
    NgwExtU X;
    lean_fetch_uniforms<EXT>(dspec, U, X);
    return lean_mask_walk<EXT>(t, U, X, min(U.n_actions, NGW_MAX_ACTIONS), S, K, r, c, f, sel, inv, cell_at);
}

// The standalone form: the masks of the state held in HBM, [n_pad] words at `out` (padding rows 0).
template <bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_mask_kernel(const NgwDevSpec* __restrict__ dspec, const NgwBufs b, uint32_t n32, int S, int K,
                                                           uint64_t* __restrict__ out) {
    __shared__ int32_t inv_lds[NGW_EPB * (NGW_MAX_ITEMS | 1)];
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    const LeanLane l = lean_load_lane(b, n32, S, K, inv_lds);
    auto cell_at = [&](int cell) -> int { return (int)ldg<int8_t>(l.bmap, l.mapoff + (uint32_t)cell); };
    const uint64_t mask = lane_mask<EXT>(dspec, S, K, l.r, l.c, l.f, l.sel, l.inv, cell_at);
    stg<uint64_t>(reinterpret_cast<char*>(out) + (uint64_t)bid * (EPB * 8), tid * 8u, l.live ? mask : 0ull);
}
