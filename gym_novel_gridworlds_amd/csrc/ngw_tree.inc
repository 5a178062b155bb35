// ngw_tree.inc - tree-search runs: the glue of one MCTS iteration between a guided playout and the key table's insert, on the device (a unit of
// its own; host side: ngw_abi_tree.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// The loop README's "Guided playouts" describes is a playout, then torch: nonzero over `where`, two index_add_ into N and Q, the insert of the
// new leaves, and the recomputation of the [buckets, A] weight rows.  Here that glue is four kernels (NgwTree in ngw_device.h says what each
// stores; the contract is include/ngw.h's ngw_tree_run, tree.py states it in numpy), so that a driver on the host can enqueue whole iterations
// without a torch operation in between.
//
// All four give one pair - or one list entry - to a lane: consecutive lanes read and write consecutive words of the step-major recorded arrays,
// no LDS, vector memory operations only.  The statistics are INTEGERS - visits int32, returns int64 - and are added with returnless global
// atomics: integer addition is associative, so the bytes do not depend on the order the device runs the adds in, nor on how the backup combines
// them inside a wave first.  What is counted over the pairs is reduced inside the wave - a ballot - and reaches memory as at most one atomic
// per wave and quantity, as in ngw_search.inc.  The one place with floats is the reweight: every operation there is a single rounded binary32
// operation through the explicit round-to-nearest intrinsics (as ngw_sample.inc's), so no multiply is ever contracted into an add.

__device__ __forceinline__ uint32_t tree_wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__device__ __forceinline__ bool tree_wave_leader() { return (threadIdx.x & (EPB - 1)) == 0; }

__global__ void __launch_bounds__(NGW_TREE_BLOCK) ngw_tree_leaf_kernel(const NgwTree x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TREE_BLOCK + threadIdx.x;
    uint64_t key = 0, mask = 0;
    int32_t d = 0;
    bool alive = false;
    if (j < x.count) {
        d = x.depth[j];
        const int32_t len = x.length[j];
        alive = len >= 1;
        if (d >= 1 && d < len && d < x.n) {                                        // (d - 1 and d are rows of the recorded arrays: n of them)
            key = x.keys[(int64_t)(d - 1) * x.stride + j];
            mask = x.masks[(int64_t)d * x.stride + j];
        }
        x.leaf_keys[j] = key;
        x.leaf_masks[j] = mask;
    }
    if (!x.row) return;
    if (j == 0)
        for (int c = 0; c < NGW_TREE_COLS; c++) x.next_row[c] = 0u;                // (the next iteration's row: nothing of this iteration counts into it)
    uint32_t deepest = alive && d > 0 ? (uint32_t)d : 0u;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)deepest, off);
        deepest = other > deepest ? other : deepest;
    }
    const uint32_t count = tree_wave_count(alive);
    if (tree_wave_leader()) {
        if (count) atomicAdd(x.row + NGW_TREE_ALIVE, count);
        if (deepest) atomicMax(x.row + NGW_TREE_DEPTH, deepest);
    }
}

__global__ void __launch_bounds__(NGW_TREE_BLOCK) ngw_tree_grow_kernel(const NgwTree x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TREE_BLOCK + threadIdx.x;
    bool grown = false, refused = false;
    if (j < x.count) {
        const int32_t w = x.where_leaf[j];
        const uint64_t mask = x.leaf_masks[j];
        if (w >= 0 && (int64_t)w < x.buckets) {
            if (mask) x.mask_words[w] = mask;                                      // (a scattered 8-byte store; equal states store equal words)
        } else {
            refused = x.leaf_keys[j] != 0;
        }
        grown = x.fresh[j] != 0;
    }
    if (!x.row) return;
    const uint32_t n_grown = tree_wave_count(grown), n_refused = tree_wave_count(refused);
    if (tree_wave_leader()) {
        if (n_grown) atomicAdd(x.row + NGW_TREE_GROWN, n_grown);
        if (n_refused) atomicAdd(x.row + NGW_TREE_REFUSED, n_refused);
    }
}

// The every-visit backup.  One lane per pair walks its steps from the last down to 0 with the return-to-go G in a register; row t of rewards /
// where / actions is read by the wave as consecutive words.  Many pairs share a root: at t = 0 a whole wave often adds to ONE (bucket, action).
// With `combine` the wave first settles the destination of its first adding lane: the lanes that share it (a compare against the broadcast
// index, a ballot) are counted and their G summed across the wave, and one lane adds both once; the other lanes add on their own.  That is the
// wave-uniform case and the majority case where the first lane belongs to it; destinations shared by fewer lanes elsewhere in the wave still
// meet in the memory system.  The sums are integers: any combining gives the same bytes.
// One body, two kernels.  DISCOUNT (ngw_tree_set_rule, g < 65536): G_t = r_t + ((g * G_{t+1}) >> 16) over the EXECUTED steps t < len - the int64 product
// wraps, the shift is arithmetic (floor) -; the steps behind them add their (zero) rewards and discount nothing.  Without it the instantiation is the
// undiscounted kernel, instruction for instruction (make asm: its body in tree.s is the parent's), so a default tree pays nothing.  The sums are
// formed in unsigned arithmetic: they wrap as the contract says, where a signed overflow would be undefined.
template <bool DISCOUNT>
__device__ __forceinline__ void tree_backup(const NgwTree& x, const int32_t g) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TREE_BLOCK + threadIdx.x;
    const bool in = j < x.count, own = j < x.cap;
    const int lane = (int)(threadIdx.x & (EPB - 1));
    int32_t d = 0, top = -1, leaf = -1, executed = 0;
    long long G = 0;
    if (in) {
        d = x.depth[j];
        int32_t len = x.length[j];
        len = len < 0 ? 0 : (len > x.n ? x.n : len);
        if (DISCOUNT) executed = len;
        if (d >= 1) top = (d < len - 1 ? d : len - 1);                             // (d = 0: the root is not in the table - nothing is backed up)
        if (x.where_leaf) leaf = x.where_leaf[j];
        if (x.bootstrap) G = (long long)x.bootstrap[j];
    }
    uint32_t steps = 0;                                                            // wave-uniform
    for (int32_t t = x.T - 1; t >= 0; t--) {
        int32_t e = -1, a = -1;
        if (in && t < x.n) {
            const int64_t at = (int64_t)t * x.stride + j;
            const unsigned long long r = (unsigned long long)(long long)x.rewards[at];
            if (DISCOUNT && t < executed) G = (long long)(r + (unsigned long long)((long long)((unsigned long long)(long long)g * (unsigned long long)G) >> 16));
            else G = (long long)((unsigned long long)G + r);
            if (t <= top) {
                e = t < d ? x.where[at] : leaf;
                a = x.actions[at];
            }
        }
        const bool add = e >= 0 && (int64_t)e < x.buckets && a >= 0 && a < x.A;
        if (own) x.touched[(int64_t)t * x.cap + j] = add ? e : -1;
        const uint64_t adding = __ballot(add);
        if (!adding) continue;
        steps += (uint32_t)__popcll(adding);
        const int32_t at = add ? e * x.A + a : -1;                                 // (buckets * A <= 2^31 - 1: checked where the tree is made)
        bool mine = add;
        if (x.combine) {
            const int first = (int)__ffsll((unsigned long long)adding) - 1;
            const int32_t shared = __shfl(at, first);
            const bool with = add && at == shared;
            const uint32_t n = tree_wave_count(with);
            if (n > 1) {                                                           // wave-uniform
                long long sum = with ? G : 0;
#pragma unroll
                for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
                if (lane == first) {
                    atomicAdd(x.visits + shared, (int32_t)n);
                    atomicAdd(x.returns + shared, (unsigned long long)sum);
                }
                mine = add && !with;
            }
        }
        if (mine) {
            atomicAdd(x.visits + at, 1);
            atomicAdd(x.returns + at, (unsigned long long)G);
        }
    }
    if (x.row && steps && lane == 0) atomicAdd(x.row + NGW_TREE_BACKED, steps);
}

__global__ void __launch_bounds__(NGW_TREE_BLOCK) ngw_tree_backup_kernel(const NgwTree x) { tree_backup<false>(x, 65536); }

__global__ void __launch_bounds__(NGW_TREE_BLOCK) ngw_tree_backup_discount_kernel(const NgwTree x, const NgwTreeRule rule) { tree_backup<true>(x, rule.g); }

// The PUCT row of one bucket: 1.0f at the valid action of the largest q + u, lowest id on ties, 0.0f elsewhere; an all-zero row for mask 0.  One
// lane per list entry walks its row three times with a scalar bound - the visit sum, the choice, the stores; an entry that names the bucket of
// the lane before it (the root, at t = 0, in every lane of a wave) is skipped: the lane before it writes the same row.
__global__ void __launch_bounds__(NGW_TREE_BLOCK) ngw_tree_reweight_kernel(const NgwTree x) {
    constexpr float LO = 0x1p-64f, HI = 0x1p64f;
    const int64_t q = (int64_t)blockIdx.x * NGW_TREE_BLOCK + threadIdx.x;
    const int32_t e = q < x.n_list ? x.list[q] : -1;
    const int32_t before = __shfl_up(e, 1);
    const bool work = e >= 0 && (int64_t)e < x.buckets && !((threadIdx.x & (EPB - 1)) != 0 && before == e);
    if (!work) return;
    const int A = min(x.A, NGW_MAX_ACTIONS);
    const int64_t base = (int64_t)e * A;
    const uint64_t m = x.mask_words[e];
    long long total = 0;
    for (int a = 0; a < A; a++) total += (long long)x.visits[base + a];
    const float root = __fsqrt_rn(__ll2float_rn(total + 1));
    int pick = -1;
    float best = 0.0f;
    bool bad = false;
    for (int a = 0; a < A; a++) {
        const int32_t v = x.visits[base + a];
        const long long r = (long long)x.returns[base + a];
        float p = 1.0f;
        if (x.priors) {
            const float w = x.priors[base + a];
            bad |= !(w >= 0.0f && w <= HI);                                        // (NaN fails both compares; -0.0 passes: it is zero)
            p = (w >= LO && w <= HI) ? w : 0.0f;
        }
        const float mean = v > 0 ? __fdiv_rn(__ll2float_rn(r), __int2float_rn(v)) : x.q_init;
        const float bonus = __fdiv_rn(__fmul_rn(__fmul_rn(x.c, p), root), __ll2float_rn(1ll + (long long)v));
        const float score = __fadd_rn(mean, bonus);
        const bool valid = ((m >> a) & 1ull) != 0;
        if (valid && (pick < 0 || score > best)) { pick = a; best = score; }
    }
    for (int a = 0; a < A; a++) x.rows[base + a] = a == pick ? 1.0f : 0.0f;
    if (bad) atomicOr(x.flags, NGW_F_BAD_WEIGHT);
}

// The 16-lane form of the reweight, and the spread rule (include/ngw.h, rule 5 with spread = S): the row of a bucket is the allotment k[a] that S
// successive PUCT choices with virtual visits make.  One list entry per DPP row of 16 lanes - 16 entries per work-group of 256 -; lane l holds the
// actions l, l + 16 and l + 32 (A <= NGW_MAX_ACTIONS = 48): their visits, returns and priors are loaded once, and q, c * p and k stay in
// registers across the S rounds.  The visit sum and every round's pick are reduced inside the row by row rotations (DPP row_ror 8, 4, 2, 1: an
// all-reduce, every lane ends with the row's answer), no LDS.  The pick of a round is the ordered walk's: the candidates are ordered by (score
// descending, id ascending), which is a total order once no score is NaN - and the walk's answer under NaN is reproduced exactly: a NaN score never
// wins `score > best`, so it is no candidate, EXCEPT at the first valid action, which the walk takes unconditionally and then never leaves (nothing is
// > NaN): there the candidate's score is +inf, and no valid id is lower than the first, so it wins every tie.  An entry equal to the entry before it
// in the list is skipped (that row writes the same bytes); divergence is by whole DPP rows only, so a rotation never reads a disabled lane.
template <int CTRL>
__device__ __forceinline__ int tree_row_ror(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }

template <int CTRL>
__device__ __forceinline__ void tree_row_best(float& s, int& id) {
    const float os = __int_as_float(tree_row_ror<CTRL>(__float_as_int(s)));
    const int oid = tree_row_ror<CTRL>(id);
    if (os > s || (os == s && oid < id)) { s = os; id = oid; }
}

template <int CTRL>
__device__ __forceinline__ long long tree_row_sum(long long v) {
    const uint32_t lo = (uint32_t)tree_row_ror<CTRL>((int)(uint32_t)(unsigned long long)v), hi = (uint32_t)tree_row_ror<CTRL>((int)(uint32_t)((unsigned long long)v >> 32));
    return v + (long long)(((unsigned long long)hi << 32) | lo);
}

constexpr int TREE_ROW = 16, TREE_SLOTS = NGW_MAX_ACTIONS / TREE_ROW, TREE_NO_ACTION = 64;
constexpr int TREE_ROR8 = 0x128, TREE_ROR4 = 0x124, TREE_ROR2 = 0x122, TREE_ROR1 = 0x121;   // DPP row_ror:n = 0x120 + n
static_assert(TREE_SLOTS * TREE_ROW == NGW_MAX_ACTIONS && NGW_TREE_BLOCK % TREE_ROW == 0, "a row of 16 lanes holds every action in three slots");

__global__ void __launch_bounds__(NGW_TREE_BLOCK) ngw_tree_reweight16_kernel(const NgwTree x, const NgwTreeRule rule) {
    constexpr float LO = 0x1p-64f, HI = 0x1p64f;
    const int l = (int)(threadIdx.x & (TREE_ROW - 1));
    const int64_t q = (int64_t)blockIdx.x * (NGW_TREE_BLOCK / TREE_ROW) + (threadIdx.x / TREE_ROW);
    const int32_t e = q < x.n_list ? x.list[q] : -1;
    const int32_t before = q > 0 && q < x.n_list ? x.list[q - 1] : -1;
    if (!(e >= 0 && (int64_t)e < x.buckets && before != e)) return;               // (uniform over the 16 lanes of the row)
    const int A = min(x.A, NGW_MAX_ACTIONS);
    const int S = min(max(rule.spread, 1), 64);
    const int64_t base = (int64_t)e * A;
    const uint64_t m = x.mask_words[e] & (~0ull >> (64 - A));
    const int first = m ? (int)__ffsll((unsigned long long)m) - 1 : -1;
    float mean[TREE_SLOTS], cp[TREE_SLOTS];
    int32_t v[TREE_SLOTS], k[TREE_SLOTS];
    long long total = 0;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < TREE_SLOTS; s++) {
        const int a = l + s * TREE_ROW;
        v[s] = 0; k[s] = 0; mean[s] = x.q_init; cp[s] = 0.0f;
        if (a < A) {
            v[s] = x.visits[base + a];
            const long long r = (long long)x.returns[base + a];
            float p = 1.0f;
            if (x.priors) {
                const float w = x.priors[base + a];
                bad |= !(w >= 0.0f && w <= HI);
                p = (w >= LO && w <= HI) ? w : 0.0f;
            }
            if (v[s] > 0) mean[s] = __fdiv_rn(__ll2float_rn(r), __int2float_rn(v[s]));
            cp[s] = __fmul_rn(x.c, p);
            total += (long long)v[s];
        }
    }
    total = tree_row_sum<TREE_ROR8>(total);
    total = tree_row_sum<TREE_ROR4>(total);
    total = tree_row_sum<TREE_ROR2>(total);
    total = tree_row_sum<TREE_ROR1>(total);
    if (m) {
        for (int i = 0; i < S; i++) {
            const float root = __fsqrt_rn(__ll2float_rn(total + 1 + i));
            float best = -__builtin_inff();
            int pick = TREE_NO_ACTION;
#pragma unroll
            for (int s = 0; s < TREE_SLOTS; s++) {
                const int a = l + s * TREE_ROW;
                const float bonus = __fdiv_rn(__fmul_rn(cp[s], root), __ll2float_rn(1ll + (long long)v[s] + (long long)k[s]));
                float score = __fadd_rn(mean[s], bonus);
                bool valid = ((m >> a) & 1ull) != 0;                               // (a < 48; bits at and above A are cleared)
                if (score != score) {                                              // NaN: the walk's first valid action keeps it, no later one takes it
                    valid = valid && a == first;
                    score = __builtin_inff();
                }
                if (valid && (pick == TREE_NO_ACTION || score > best)) { pick = a; best = score; }   // (ids ascend with s: a tie keeps the lower)
            }
            tree_row_best<TREE_ROR8>(best, pick);
            tree_row_best<TREE_ROR4>(best, pick);
            tree_row_best<TREE_ROR2>(best, pick);
            tree_row_best<TREE_ROR1>(best, pick);
#pragma unroll
            for (int s = 0; s < TREE_SLOTS; s++) k[s] += (pick == l + s * TREE_ROW) ? 1 : 0;
        }
    }
#pragma unroll
    for (int s = 0; s < TREE_SLOTS; s++) {
        const int a = l + s * TREE_ROW;
        if (a < A) x.rows[base + a] = __int2float_rn(k[s]);
    }
    if (bad) atomicOr(x.flags, NGW_F_BAD_WEIGHT);
}

}  // namespace
