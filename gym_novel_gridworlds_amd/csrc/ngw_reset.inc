// ngw_reset.inc — the dedicated new-episode kernel.
#pragma once
#include "ngw_common.inc"
#include "ngw_newepisode.inc"      // the Philox stream, the prepared rows, the signals towards the host

namespace {
//
// reset() of the plain configurations, of AddItem / Crate (pogostick_v1_env.py:86-181, novelty_wrappers.py:1013-1034, :1071)
// and of ReplaceItem / FireWall of the wall ring (:1129-1160), for explicit resets (ngw_reset) and for preparing next
// episodes (NGW_MODE_REFILL); same per-(env, episode) Philox4x32-10 stream and same draws as reset_lane / the oracle's
// Philox mode, bit for bit.  One lane per env and NO byte map anywhere but in the output:
//   * a fresh map is the wall ring + the <= 12 placed items (+ the cells a subset pass fills), so the placement loop's "cell
//     and its four neighbours are air" test is one bit of a `blocked` mask over the candidate grid (set around every placed
//     item) instead of five map reads;
//   * the subset pass (include/ngw.h, ngw_spec.n_passes: a uniformly random cnt-subset of the air / ring cells, which is all
//     that numpy's shuffle + prefix amounts to) works on ONE BIT PER CELL: a per-lane column of LDS words, candidate cell
//     indices cut four at a time from one Philox block (bit fields: no multiply, no mapping), their four words read together,
//     accepted in order in registers, set with fire-and-forget ds_or - no index array, no shuffle, min(cnt, len - cnt)
//     accepted draws instead of len;
//   * the map leaves the kernel ONCE, composed per env from the ring template, the bit column and the placed list
//     into an LDS tile and stored from there with consecutive lanes on consecutive bytes of one env: no template store
//     followed by scattered byte stores (round 2: ~270 partial-line writes per env at 32 x 32, 11x the payload in HBM
//     write traffic), and no lane-per-row stores either (measured: 64 partial lines per instruction, 1 300 cycles each);
//   * random words for the placement loop come from a per-lane LDS ring that the WAVE tops up (one Philox block for every
//     lane with room whenever any lane runs dry), and every loop consumes at most one word per lane and iteration: the
//     10-round block is executed max-over-lanes(words) / 4 times per wave, not once per draw.
// Configurations with other reset passes (Fence, ReplaceItem of an interior item, stacks, the v0 tree tap) or the fused lidar
// epilogue keep the general kernel.

constexpr int RING_W = 16;                                                         // words per lane in the ring

struct WaveRing {
    uint32_t k0, k1, c0, c1, c2, c3;
    LDS_AS uint32_t* ring;                                                         // word slot s of this lane at ring[s * EPB]
    uint32_t rd, wr, cur;                                                          // consumed / produced; cur = word rd (valid iff rd < wr)

    __device__ __forceinline__ void init(uint64_t seed, uint64_t env, uint32_t episode, LDS_AS uint32_t* ring_) {
        k0 = (uint32_t)seed; k1 = (uint32_t)(seed >> 32);
        c0 = 0; c1 = episode; c2 = (uint32_t)env; c3 = (uint32_t)(env >> 32);
        ring = ring_; rd = wr = 0; cur = 0;
    }
    // Wave-level: call where EVERY lane of the wave arrives together.  `want` = this lane may take a word before the next call.
    __device__ __forceinline__ void top_up(bool want) {
        if (__any(want && rd == wr)) {
            if (want && wr - rd <= (uint32_t)(RING_W - 4)) {
                uint32_t w0, w1, w2, w3;
                philox_block(c0, c1, c2, c3, k0, k1, w0, w1, w2, w3);
                c0++;
                const uint32_t s = wr & (RING_W - 1);                              // wr is a multiple of 4: no wrap inside a block
                ring[s * EPB] = w0; ring[(s + 1) * EPB] = w1; ring[(s + 2) * EPB] = w2; ring[(s + 3) * EPB] = w3;
                if (rd == wr) cur = w0;
                wr += 4;
            }
        }
    }
    __device__ __forceinline__ uint32_t take() {                                   // requires rd < wr (top_up(true) since the last take)
        const uint32_t w = cur;
        rd++;
        cur = ring[(rd & (RING_W - 1)) * EPB];                                     // next word, requested one draw ahead
        return w;
    }
    // Branch-free form for lock-step loops: the current word; the lane consumes it iff `on` (an idle lane re-reads its slot).
    __device__ __forceinline__ uint32_t take_if(bool on) {
        const uint32_t w = cur;
        rd += on ? 1u : 0u;
        cur = ring[(rd & (RING_W - 1)) * EPB];
        return w;
    }
};

__device__ __forceinline__ uint32_t smear_mask(uint32_t max) { return 0xFFFFFFFFu >> __clz((int)(max | 1u)); }

// Bit masks over the candidate grid ((S-4)^2 cells, row-major): NW words per lane, in registers (dynamic word access by
// unrolled selects) up to 8 words = 16 x 16 candidates (S <= 20), in LDS columns beyond.
template <int NW>
struct RegMask {
    uint32_t w[NW];
    __device__ __forceinline__ void fill(int nbits) {
#pragma unroll
        for (int k = 0; k < NW; k++) { const int left = nbits - 32 * k; w[k] = left >= 32 ? 0xFFFFFFFFu : (left > 0 ? ((1u << left) - 1u) : 0u); }
    }
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] = 0;
    }
    __device__ __forceinline__ uint32_t word(int i) const {                        // 0 beyond the mask
        uint32_t x = 0;
#pragma unroll
        for (int k = 0; k < NW; k++) x = i == k ? w[k] : x;
        return x;
    }
    __device__ __forceinline__ bool test(int pos) const { return (word(pos >> 5) >> (pos & 31)) & 1u; }
    __device__ __forceinline__ void set(int pos, bool on) {
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] |= (on && (pos >> 5) == k) ? 1u << (pos & 31) : 0u;
    }
    __device__ __forceinline__ void reset_bit(int pos) {
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] &= (pos >> 5) == k ? ~(1u << (pos & 31)) : 0xFFFFFFFFu;
    }
    __device__ __forceinline__ int select(int idx) const {                         // position of the idx-th (0-based) set bit
        int base = 0, rem = idx;
        uint32_t x = w[0];
        bool found = false;
#pragma unroll
        for (int k = 0; k < NW; k++) {
            const int pc = __popc(w[k]);
            const bool here = !found && rem < pc;
            x = here ? w[k] : x; base = here ? 32 * k : base;
            found |= here;
            rem -= (!found) ? pc : 0;
        }
        return base + nth_set_bit(x, rem);
    }
};

// Fire-and-forget LDS read-modify-write (ds_or_b32, no return value): nothing of it sits in a dependency chain; a lane with
// nothing to set ORs a zero instead of being masked off.  LDS operations of a wave execute in order, so a later read of the
// same word sees it.
__device__ __forceinline__ void lds_or(LDS_AS uint32_t* p, uint32_t val) {
    asm volatile("ds_or_b32 %0, %1" ::"v"((uint32_t)(size_t)p), "v"(val) : "memory");
}
__device__ __forceinline__ void lds_and(LDS_AS uint32_t* p, uint32_t val) {
    asm volatile("ds_and_b32 %0, %1" ::"v"((uint32_t)(size_t)p), "v"(val) : "memory");
}

// The same masks as LDS columns (word k of this lane at p[k * EPB]) for candidate grids beyond 16 x 16.  Updates are
// fire-and-forget read-modify-writes (ds_or / ds_and: nothing of them sits in the try's dependency chain), and the candidate
// mask keeps the number of set bits of every group of eight words in registers, so "the idx-th remaining candidate" is one
// compare chain over <= 8 counters + ONE round trip for the eight words of the group it falls into (it used to walk the
// whole column, eight words per round trip: 3-4 dependent round trips per try at 28 x 28 candidates).
struct LdsMask {
    LDS_AS uint32_t* p;
    int nw, gsh;                                                                   // words; log2 of the words per group (3, or 4 beyond 64 words: maps up to 64 x 64)
    uint32_t gc[8];                                                                // set bits per group (candidate mask only)
    __device__ __forceinline__ void fill(int nbits) {
        for (int k = 0; k < nw; k++) { const int left = nbits - 32 * k; p[k * EPB] = left >= 32 ? 0xFFFFFFFFu : (left > 0 ? ((1u << left) - 1u) : 0u); }
        const int gbits = 32 << gsh;
#pragma unroll
        for (int g = 0; g < 8; g++) gc[g] = (uint32_t)min(max(nbits - gbits * g, 0), gbits);
    }
    __device__ __forceinline__ void clear() { for (int k = 0; k < nw; k++) p[k * EPB] = 0; }
    __device__ __forceinline__ bool test(int pos) const { return (p[(pos >> 5) * EPB] >> (pos & 31)) & 1u; }
    __device__ __forceinline__ void set(int pos, bool on) { lds_or(p + (on ? pos >> 5 : 0) * EPB, on ? 1u << (pos & 31) : 0u); }
    __device__ __forceinline__ void reset_bit(int pos) {                           // (pos is a set bit of the candidate mask)
        lds_and(p + (pos >> 5) * EPB, ~(1u << (pos & 31)));
        const int grp = pos >> (5 + gsh);
#pragma unroll
        for (int g = 0; g < 8; g++) gc[g] -= grp == g ? 1u : 0u;
    }
    __device__ __forceinline__ int select(int idx) const {                         // position of the idx-th (0-based) set bit
        int rem = idx, grp = 0;
        bool found = false;
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const bool here = !found && rem < (int)gc[g];
            grp = here ? g : grp;
            found |= here;
            rem -= found ? 0 : (int)gc[g];
        }
        const int w0 = grp << gsh, gw = 1 << gsh;
        int base = 0;
        uint32_t x = 0;
        found = false;
        for (int h = 0; h < gw; h += 8) {                                          // (uniform: one trip, two beyond 64 words)
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = p[min(w0 + h + j, nw - 1) * EPB];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int pc = w0 + h + j < nw ? __popc(v[j]) : 0;
                const bool here = !found && rem < pc;
                x = here ? v[j] : x; base = here ? 32 * (w0 + h + j) : base;
                found |= here;
                rem -= found ? 0 : pc;
            }
        }
        return base + nth_set_bit(x, rem);
    }
};



constexpr int PLR = 12;                                                            // placed items per reset this kernel handles (the host checks n_place)

template <int NW /* mask words in registers, 0 = LDS */, bool SUBSET /* one subset pass over the air of the interior / the wall ring */>
__global__ void __launch_bounds__(NGW_EPB) ngw_reset_fast(const NgwDevSpec* __restrict__ dspec, const NgwResetFast a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    STAMP_DECL;
    STAMP(0);
    const int tid = threadIdx.x;
    const uint32_t bid = blockIdx.x;
    const int64_t env0 = (int64_t)bid * EPB;
    const bool live = env0 + tid < a.n;
    const bool refill = a.mode == NGW_MODE_REFILL;
    // what the host reads, without a sync, before a later refill: the stale-row resets so far and the number of this refill -
    // counted on the device, so that a replayed graph reports increasing numbers too
    if (refill && bid == 0 && tid == 0 && a.nx.slow_host) { a.nx.slow_host[0] = a.nx.slow[0]; a.nx.slow_host[1] = atomicAdd(a.nx.slow + 1, 1u) + 1u; }
    const int S = a.S, S2 = a.S2, K = a.K, W = S - 4, ncand = W * W;
    const int MW = (S2 + 31) >> 5;                                                 // words of a bit column that cover the map
    const int NBW = SUBSET ? (1 << a.sub_nb) >> 5 : 0;                             // words of the column the candidates index (2^nb bits)
    const bool wallpass = SUBSET && a.pass_wall != 0;                              // ReplaceItem / FireWall of the wall item: the source cells are the ring
    const uint32_t main_ep = live ? a.main.episode[env0 + tid] : 0u;
    // Prepared episodes are kept `depth` deep (a power of two): the row of episode E of env e lives in slot E & (depth - 1),
    // at row index slot * nx.stride + e of every shadow array.  A refill visits the slots one after the other; an explicit
    // reset builds (or copies) the one episode main + 1.
    const uint32_t dmask = (uint32_t)a.nx.dmask;
    const int nslots = refill ? (int)dmask + 1 : 1;
    // A refill of a DEEPER set compacts: the wave's stale (env, slot) pairs - up to 64 x depth of them, typically a fraction of
    // one wave's worth per slot when episodes end fast - are listed first, and every pass of the loop below builds 64 of them,
    // lane j the j-th pair of the list, whatever env and slot it belongs to.  A pass per slot ran the whole placement chain
    // for a handful of lanes each time (FireWall hard, four episodes deep: 88 us per refill of 65 536 envs for ~0.5 rows per env).
    const bool compact = refill && nslots > 1;
    LDS_AS uint32_t* const crow = (LDS_AS uint32_t*)(lds + a.off_ctab);            // [64] destination row of this pass's lanes
    LDS_AS uint16_t* const ctab = (LDS_AS uint16_t*)(crow + EPB);                  // [64 * depth] slot << 8 | lane of the wave
    int npass = nslots, npairs = 0;
    if (compact) {
        for (int s = 0; s < nslots; s++) {
            const uint32_t ep_s = main_ep + 1u + (((uint32_t)s - main_ep - 1u) & dmask);
            const bool stale = live && a.nx.episode[(int64_t)s * a.nx.stride + env0 + tid] != ep_s;
            const uint64_t b = __ballot(stale);
            if (stale) ctab[npairs + __popcll(b & ((1ull << tid) - 1ull))] = (uint16_t)(((uint32_t)s << 8) | (uint32_t)tid);
            npairs += __popcll(b);
        }
        npass = (npairs + EPB - 1) / EPB;
        __syncthreads();
    }
    bool lds_ready = false;
  for (int pass = 0; pass < npass; pass++) {
    // ---- which lanes build an episode, of which env, for which slot
    int slot = pass;
    int64_t e = env0 + tid;
    uint32_t episode = main_ep + 1u;
    bool todo0 = false;
    if (compact) {
        const int j = pass * EPB + tid;
        todo0 = j < npairs;
        const uint32_t ent = ctab[min(j, npairs - 1)];
        slot = (int)(ent >> 8);
        const int lane = (int)(ent & 255u);
        e = env0 + lane;
        const uint32_t mep = (uint32_t)__shfl((int)main_ep, lane);
        episode = mep + 1u + (((uint32_t)slot - mep - 1u) & dmask);
    } else if (live) {
        if (refill) {                                                              // the episode of (main, main + depth] that belongs into this slot
            episode = main_ep + 1u + (((uint32_t)slot - main_ep - 1u) & dmask);
            todo0 = a.nx.episode[(int64_t)slot * a.nx.stride + e] != episode;      // stale unless prepared for exactly that episode
        } else todo0 = a.reset_mask ? a.reset_mask[e] != 0 : true;
    }
    if (!__any(todo0)) continue;
    // ---- an explicit reset with the episode already prepared (the refill that followed the last reset built it): copy the
    //      row - the same bytes the loops below would produce.  A whole wave of prepared rows in ONE slot moves as coalesced
    //      16-byte pieces (the 64 rows are contiguous in both buffer sets), a lone lane walks its own row.
    bool prep = false;
    if (!refill && a.nx.episode) {
        const uint32_t sl = episode & dmask;
        const int64_t se = (int64_t)sl * a.nx.stride + e;
        prep = todo0 && a.nx.episode[se] == episode;
        if (__any(prep)) {
            const uint32_t sl0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sl);
            if (env0 + EPB <= a.n && __all(prep && sl == sl0)) {
                const int64_t s0 = (int64_t)sl0 * a.nx.stride + env0;
                const int npieces = 4 * S2;
                const u32x4* s4 = reinterpret_cast<const u32x4*>(a.nx.map + s0 * S2);
                u32x4* d4 = reinterpret_cast<u32x4*>(a.main.map + env0 * S2);
                for (int p = tid; p < npieces; p += EPB) d4[p] = s4[p];
                const u32x4* si4 = reinterpret_cast<const u32x4*>(a.nx.inv + s0 * K);
                u32x4* di4 = reinterpret_cast<u32x4*>(a.main.inv + env0 * K);
                for (int p = tid; p < 16 * K; p += EPB) di4[p] = si4[p];
                if (a.boards) {                                                    // boards mode: the prepared maps' occupancy bit rows
                    const u32x4* sb4 = reinterpret_cast<const u32x4*>(a.nx.brd + s0 * a.BS);
                    u32x4* db4 = reinterpret_cast<u32x4*>(a.main.brd + env0 * a.BS);
                    for (int p = tid; p < 16 * a.BS; p += EPB) db4[p] = sb4[p];
                }
            } else if (prep) {
                const int8_t* src = a.nx.map + se * S2;
                int8_t* dst = a.main.map + e * S2;
                if ((S2 & 3) == 0) {
                    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
                    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
                    for (int i = 0; i < (S2 >> 2); i++) d32[i] = s32[i];
                } else {
                    for (int i = 0; i < S2; i++) dst[i] = src[i];
                }
                for (int k = 0; k < K; k++) a.main.inv[e * K + k] = a.nx.inv[se * K + k];
                if (a.boards) for (int k = 0; k < a.BS; k++) a.main.brd[e * a.BS + k] = a.nx.brd[se * a.BS + k];
            }
            if (prep) {
                reinterpret_cast<int2*>(a.main.loc)[e] = reinterpret_cast<const int2*>(a.nx.loc)[se];
                a.main.facing[e] = a.nx.facing[se];
                a.main.selected[e] = 0;
                a.main.step_count[e] = 0;
                a.main.episode[e] = episode;
            }
        }
    }
    const bool todo = todo0 && !prep;
    if (!__any(todo)) continue;
    const int64_t drow = (refill ? (int64_t)slot * a.nx.stride : 0) + e;           // this lane's row of the destination arrays
    int8_t* const dmap = refill ? a.nx.map : a.main.map;
    int32_t* const dloc = refill ? a.nx.loc : a.main.loc;
    int32_t* const dfac = refill ? a.nx.facing : a.main.facing;
    int32_t* const dinv = refill ? a.nx.inv : a.main.inv;
    uint32_t* const dtag = refill ? a.nx.episode : nullptr;
    crow[tid] = (uint32_t)drow;                                                    // (row numbers fit 32 bits: the arrays exist in memory)

    // ---- one map of ring + air in LDS (16 spare bytes behind it), the placement sequence, and - for the subset pass - the
    //      cells that match the pass on an empty map, one bit per cell (air pass: the interior; wall pass: the ring), the same
    //      for every env of the wave.  64 cells per trip: every lane decides its cell, a ballot makes the two words.
    if (!lds_ready) {
        lds_ready = true;
        uint8_t* t = reinterpret_cast<uint8_t*>(lds + a.off_tmpl);
        const int ncell = SUBSET ? max(S2 + 16, NBW * 32) : S2 + 16;
        for (int i0 = 0; i0 < ncell; i0 += EPB) {
            const int i = i0 + tid;
            const int r = (int)__umulhi((uint32_t)i, a.magicS), c = i - r * S;
            const bool ring = i < S2 && (r == 0 || c == 0 || r == S - 1 || c == S - 1);
            if (i < S2 + 16) t[i] = ring ? (uint8_t)a.wall_item : (uint8_t)0;
            if (SUBSET) {
                const uint64_t b = __ballot(i < S2 && ring == wallpass);
                if (tid == 0 && (i0 >> 5) < NBW) lds[a.off_dom + (i0 >> 5)] = (uint32_t)b;
                if (tid == 0 && (i0 >> 5) + 1 < NBW) lds[a.off_dom + (i0 >> 5) + 1] = (uint32_t)(b >> 32);
            }
        }
        uint8_t* ps = t + S2 + 16;
        if (tid < NGW_MAX_PLACE) ps[tid] = dspec->place_seq[tid];
    }
    // inventory rows: zeros + the start inventory (AxeEasy.reset :33, AxetoBreakHard.reset :667-670) - the same row for every env
    if (todo) {
        uint32_t* row = reinterpret_cast<uint32_t*>(dinv) + (uint64_t)drow * (uint32_t)K;
        for (int k = 0; k < K; k++) {
            uint32_t v = 0;
            for (int j = 0; j < a.n_inv_start; j++) v = (int)((a.inv_start_items >> (8 * j)) & 255u) == k ? (a.inv_start_qtys >> (8 * j)) & 255u : v;
            row[k] = v;
        }
    }
    __syncthreads();

    STAMP(1);
    // ---- per-lane reset (pogostick_v1_env.py:86-157 + add_item_to_map :159-181)
    WaveRing px;
    px.init(a.seed, (uint64_t)(a.env_base + e), episode, (LDS_AS uint32_t*)(lds + a.off_ring + tid));
    const uint32_t magicW = a.magicW;
    LDS_AS uint32_t* placed = (LDS_AS uint32_t*)(lds + a.off_placed + tid);          // placement n: cell << 8 | item at placed[n * EPB]
    const LDS_AS uint8_t* place_seq = (const LDS_AS uint8_t*)(lds + a.off_tmpl) + S2 + 16;
    // candidate / blocked masks over the candidate grid
    RegMask<(NW > 0 ? NW : 1)> rc, rb;
    LdsMask lc, lb;
    if (NW > 0) { rc.fill(ncand); rb.clear(); }
    else {
        lc.p = (LDS_AS uint32_t*)(lds + a.off_masks + tid); lc.nw = a.CW; lc.gsh = a.CW <= 64 ? 3 : 4;
        lb.p = lc.p + a.CW * EPB; lb.nw = a.CW; lb.gsh = lc.gsh;
        lc.fill(ncand); lb.clear();
    }
    uint32_t flags = 0;
    int phase = todo ? 0 : 3;                                                      // 0 agent cell, 1 facing, 2 placements, 3 done
    int apos = 0, agent = 0, r_out = 1, c_out = 1, f_out = 0, len = ncand, n = 0;
    const int total = a.n_place;
    if (todo && ncand < 1) { flags |= NGW_F_PLACEMENT; phase = 3; }
    while (__any(phase < 3)) {
        PIN_V(phase); PIN_V(len);                                                  // (opaque per iteration: keeps LLVM from threading the rejection path into an inner divergent loop)
        // the draw this lane is waiting for: np.random.choice(len(list)) / choice(4) -> bounded(max)
        const uint32_t max = phase == 0 ? (uint32_t)ncand - 1u : (phase == 1 ? 3u : (uint32_t)len - 1u);
        const bool active = phase < 3;
        const bool needs_word = active && max != 0;                                // max == 0 consumes no word (numpy)
        px.top_up(needs_word);
        if (active) {
            uint32_t v = 0;
            if (needs_word) v = px.take() & smear_mask(max);
            if (v <= max) {
                if (phase == 0) {                                                  // :141 (the agent stays in the list)
                    apos = (int)v;
                    const int arow = (int)__umulhi((uint32_t)apos, magicW), acol = apos - arow * W;
                    r_out = 2 + arow; c_out = 2 + acol; agent = r_out * S + c_out;
                    phase = 1;
                } else if (phase == 1) {                                           // :145
                    f_out = (int)v;
                    phase = total > 0 ? 2 : 3;
                } else {                                                           // :169 idx-th remaining candidate, row-major; list.pop(idx)
                    const int pos = NW > 0 ? rc.select((int)v) : lc.select((int)v);
                    if (NW > 0) rc.reset_bit(pos); else lc.reset_bit(pos);
                    len--;
                    const bool blocked = NW > 0 ? rb.test(pos) : lb.test(pos);
                    if (pos != apos && !blocked) {                                 // :172-178: not the agent, cell and 4 neighbours are air
                        const int prow = (int)__umulhi((uint32_t)pos, magicW), pcol = pos - prow * W;
                        const int cell = (2 + prow) * S + 2 + pcol, item = place_seq[n];
                        placed[n * EPB] = ((uint32_t)cell << 8) | (uint32_t)item;
                        if (NW > 0) {
                            rb.set(pos, true); rb.set(pos - 1, pcol > 0); rb.set(pos + 1, pcol < W - 1);
                            rb.set(pos - W, prow > 0); rb.set(pos + W, prow < W - 1);
                        } else {
                            lb.set(pos, true); lb.set(pos - 1, pcol > 0); lb.set(pos + 1, pcol < W - 1);
                            lb.set(pos - W, prow > 0); lb.set(pos + W, prow < W - 1);
                        }
                        n++;
                    }
                    if (n >= total) phase = 3;
                    else if (len < 1) { flags |= NGW_F_PLACEMENT; phase = 3; }     // :167
                }
            }
        }
    }
    STAMP(2);
    // ---- the placed items, cell << 8 | item, in 12 registers (nothing beyond n)
    uint32_t pl[PLR];
#pragma unroll
    for (int j = 0; j < PLR; j++) pl[j] = (todo && j < n) ? placed[j * EPB] : 0x7FFFFFFFu;
    // ---- the subset pass on one bit per cell (AddItem.reset novelty_wrappers.py:1017-1028, Crate.reset :1071, ReplaceItem.reset
    //      :1131-1144 of the wall item, FireWall.reset :1160); bit c of the lane's column = cell c is taken
    LDS_AS uint32_t* mcol = (LDS_AS uint32_t*)(lds + (SUBSET ? a.off_mcol : 0u) + tid);
    if (SUBSET) {
        const bool run = todo && !flags;
        // the column starts as "cannot be drawn": everything but the matching cells (cells beyond the map included)
        for (int w = 0; w < NBW; w++) mcol[w * EPB] = ~lds[a.off_dom + w];
        if (!wallpass)                                                             // an item's cell is not air
#pragma unroll
            for (int j = 0; j < PLR; j++)
                if (j < total) { const uint32_t cell = pl[j] >> 8; if (run && j < n) mcol[(cell >> 5) * EPB] |= 1u << (cell & 31u); }
        const int plen = run ? (wallpass ? 4 * S - 4 : (S - 2) * (S - 2) - n) : 0; // what np.where(map == 0) / (map == wall) finds
        int pct = -1;                                                              // randint(lo, hi) FIRST; a span of 1 draws nothing
        const uint32_t pmax = (uint32_t)a.additem_span - 1u;
        if (!run || pmax == 0) pct = 0;
        while (__any(pct < 0)) {
            PIN_V(pct);
            const bool act = pct < 0;
            px.top_up(act);
            if (act) { const uint32_t v = px.take() & smear_mask(pmax); if (v <= pmax) pct = (int)v; }
        }
        const int cnt = run ? (int)ceil((double)plen * a.pctq[pct]) : 0;           // int(np.ceil(len * (pct / 100)))
        const bool comp = 2 * cnt > plen;                                          // the complement is the smaller set: draw what is NOT taken
        const int need = comp ? plen - cnt : cnt;
        STAMP(3);
        // Candidates four at a time: field j of the four words of one Philox block (blocks from the next block boundary on)
        // = four cell indices, their four column words read together, accepted IN ORDER in registers (a cell taken earlier
        // in the same group counts as taken), four fire-and-forget ds_or - one LDS round trip per group sits in the loop's
        // dependency chain.  Written without per-lane branches (lanes that are done keep drawing and accept nothing).
        {
            const int nb = a.sub_nb, F = a.sub_fields;
            const uint32_t fm = (1u << nb) - 1u;
            uint32_t c0 = (px.rd + 3u) >> 2;
            int got = 0;
            while (__any(got < need)) {
                PIN_V(got);
                uint32_t w[4];
                philox_block(c0, px.c1, px.c2, px.c3, px.k0, px.k1, w[0], w[1], w[2], w[3]);
                c0++;
                for (int j = 0; j < F; j++) {                                      // (uniform)
                    const int sh = j * nb;
                    uint32_t cell[4], bit[4], wd[4];
                    LDS_AS uint32_t* at[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        cell[k] = (w[k] >> sh) & fm;
                        at[k] = mcol + (cell[k] >> 5) * EPB; bit[k] = 1u << (cell[k] & 31u);
                        wd[k] = *at[k];
                    }
                    bool acc[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        bool dup = false;
#pragma unroll
                        for (int i = 0; i < k; i++) dup |= acc[i] && cell[i] == cell[k];
                        acc[k] = !(wd[k] & bit[k]) && !dup && got < need;
                        got += acc[k] ? 1 : 0;
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) lds_or(at[k], acc[k] ? bit[k] : 0u);
                }
            }
        }
        STAMP(4);
        // what gets the item: the cells taken, or - complement - the matching cells NOT taken (the column's zeros); never an
        // item's cell, never the agent's (:1026 / :1142)
        for (int w = 0; w < MW; w++) { const uint32_t m = mcol[w * EPB], d = lds[a.off_dom + w]; mcol[w * EPB] = comp ? ~m : (m & d); }
        if (!wallpass)
#pragma unroll
            for (int j = 0; j < PLR; j++)
                if (j < total) { const uint32_t cell = pl[j] >> 8; if (run && j < n) mcol[(cell >> 5) * EPB] &= ~(1u << (cell & 31u)); }
        if (run) mcol[(agent >> 5) * EPB] &= ~(1u << (agent & 31));
    }
    STAMP(5);
    // ---- the map, composed per env and stored once.  A lane composes its own row, 128 bytes at a time, into its row of an
    //      LDS tile - template ^ (taken ? wall-or-air ^ item : 0) from the bit column, then one byte per placed item that
    //      falls into the window (no walk, no per-cell test) - and the wave stores the 64 windows with consecutive lanes on
    //      consecutive units of one env (16-byte units where rows are 16-byte aligned, dwords / bytes otherwise): full lines
    //      per env instead of one partial line per lane and instruction.
    {
        // Rows up to 512 bytes (maps up to 22 x 22): the tile is the exact IMAGE of the wave's 64 rows (row stride S*S) and goes
        // out after the last window as one run of coalesced 16-byte pieces over the whole chunk - full lines except at the chunk's
        // edges, whatever the row size is (a piece that straddles two envs of which only one is being built goes by bytes).
        constexpr int CH = 128;                                                    // window bytes per env
        const bool img = a.img != 0;
        const int TS = img ? S2 : 144;                                             // tile row stride
        const uint64_t todo_mask = __ballot(todo);
        // (one slot per pass: the wave's 64 rows are contiguous, `chunk`; a compacting refill stores row by row through `crow`)
        uint8_t* chunk = reinterpret_cast<uint8_t*>(dmap) + ((uint64_t)(refill && !compact ? (int64_t)slot * a.nx.stride : 0) + (uint64_t)env0) * (uint32_t)S2;
        uint8_t* const dmap8 = reinterpret_cast<uint8_t*>(dmap);
        LDS_AS uint8_t* tile = (LDS_AS uint8_t*)(lds + a.off_tile);
        LDS_AS uint8_t* trow0 = tile + tid * TS;
        const LDS_AS uint8_t* tb = (const LDS_AS uint8_t*)(lds + a.off_tmpl);
        const uint32_t xor4 = SUBSET ? (uint32_t)((wallpass ? a.wall_item : 0) ^ a.additem_item) * 0x01010101u : 0u;
        auto expand = [&](uint32_t tmpl, uint32_t bits4) -> uint32_t {             // 4 bits -> 4 bytes of 0 / xor value over the template
            const uint32_t x01 = __umul24(bits4, 0x00204081u) & 0x01010101u;
            return tmpl ^ (((x01 << 8) - x01) & xor4);
        };
        const int ush = (S2 & 15) == 0 ? 4 : ((S2 & 3) == 0 ? 2 : 0);             // log2 of the store unit (uniform)
        for (int cw = 0; cw < S2; cw += CH) {
            const int chlen = min(CH, S2 - cw);
            LDS_AS uint8_t* trow = trow0 + (img ? cw : 0);                          // where this window of the lane's row goes
            if (ush == 4 && chlen == CH) {                                         // a full window: every LDS read issued before the first use
                uint32_t m[4];
                u32x4 t[8];
#pragma unroll
                for (int w = 0; w < 4; w++) m[w] = SUBSET ? mcol[((cw >> 5) + w) * EPB] : 0u;
#pragma unroll
                for (int p = 0; p < 8; p++) t[p] = *(const LDS_AS u32x4*)(tb + cw + 16 * p);
#pragma unroll
                for (int p = 0; p < 8; p++) {
                    u32x4 v = t[p];
                    if (SUBSET) {
                        const uint32_t b = m[p >> 1] >> (16 * (p & 1));
                        v.x = expand(v.x, b & 15u); v.y = expand(v.y, (b >> 4) & 15u); v.z = expand(v.z, (b >> 8) & 15u); v.w = expand(v.w, (b >> 12) & 15u);
                    }
                    *(LDS_AS u32x4*)(trow + 16 * p) = v;
                }
            } else if (ush == 4) {
                for (int o = 0; o < chlen; o += 32) {                              // one word of the bit column = two 16-byte units
                    const uint32_t m = SUBSET ? mcol[((cw + o) >> 5) * EPB] : 0u;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int p = o + 16 * h;
                        if (p < chlen) {                                           // (uniform)
                            const u32x4 t4 = *(const LDS_AS u32x4*)(tb + cw + p);
                            u32x4 v = t4;
                            if (SUBSET) {
                                v.x = expand(t4.x, (m >> (16 * h)) & 15u); v.y = expand(t4.y, (m >> (16 * h + 4)) & 15u);
                                v.z = expand(t4.z, (m >> (16 * h + 8)) & 15u); v.w = expand(t4.w, (m >> (16 * h + 12)) & 15u);
                            }
                            *(LDS_AS u32x4*)(trow + p) = v;
                        }
                    }
                }
            } else if (ush == 2) {
#pragma unroll 5
                for (int o = 0; o < chlen; o += 4) {
                    const int cell = cw + o;
                    const uint32_t t1 = *(const LDS_AS uint32_t*)(tb + cell);
                    const uint32_t m = SUBSET ? mcol[(cell >> 5) * EPB] : 0u;
                    *(LDS_AS uint32_t*)(trow + o) = SUBSET ? expand(t1, (m >> (cell & 31)) & 15u) : t1;
                }
            } else {                                                               // odd S: rows are byte-aligned
                for (int o = 0; o < chlen; o++) {
                    const int cell = cw + o;
                    const uint32_t m = SUBSET ? mcol[(cell >> 5) * EPB] : 0u;
                    trow[o] = (uint8_t)(tb[cell] ^ (((m >> (cell & 31)) & 1u) ? (xor4 & 255u) : 0u));
                }
            }
#pragma unroll
            for (int j = 0; j < PLR; j++)
                if (j < total) {                                                   // (uniform)
                    const uint32_t off = (pl[j] >> 8) - (uint32_t)cw;
                    if (off < (uint32_t)chlen) trow[off] = (uint8_t)pl[j];
                }
            if (img) continue;                                                     // (uniform) the whole chunk goes out below
            __syncthreads();
            const int nu = (chlen + (1 << ush) - 1) >> ush;                        // units per env in this window
            if (ush == 4 && chlen == CH) {                                         // 8 units per env: 8 trips, reads first
                u32x4 r[8];
#pragma unroll
                for (int it = 0; it < 8; it++) { const int q = tid + EPB * it; r[it] = *(const LDS_AS u32x4*)(tile + (q >> 3) * TS + ((q & 7) << 4)); }
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    const int q = tid + EPB * it, env = q >> 3;
                    if ((todo_mask >> env) & 1ull) {
                        uint8_t* const rowp = compact ? dmap8 + (uint64_t)crow[env] * (uint32_t)S2 : chunk + (uint32_t)env * (uint32_t)S2;
                        *reinterpret_cast<u32x4*>(rowp + (uint32_t)(cw + ((q & 7) << 4))) = r[it];
                    }
                }
            } else {
                const bool full = chlen == CH;
#pragma unroll 4
                for (int q = tid; q < EPB * nu; q += EPB) {
                    int env, u;
                    if (full) { env = q >> (7 - ush); u = q & ((1 << (7 - ush)) - 1); }
                    else if (nu == 1) { env = q; u = 0; }
                    else { env = (int)__umulhi((uint32_t)q, a.magic_tail); u = q - env * nu; }
                    if ((todo_mask >> env) & 1ull) {
                        const LDS_AS uint8_t* src = tile + env * TS + (u << ush);
                        uint8_t* dst = (compact ? dmap8 + (uint64_t)crow[env] * (uint32_t)S2 : chunk + (uint32_t)env * (uint32_t)S2) + (uint32_t)(cw + (u << ush));
                        if (ush == 4) *reinterpret_cast<u32x4*>(dst) = *(const LDS_AS u32x4*)src;
                        else if (ush == 2) *reinterpret_cast<uint32_t*>(dst) = *(const LDS_AS uint32_t*)src;
                        else *dst = *src;
                    }
                }
            }
            __syncthreads();
        }
        if (img) {
            __syncthreads();
            const int npc = 4 * S2;                                                // 16-byte pieces of the chunk
            const u32x4 LDS_AS* t16 = (const u32x4 LDS_AS*)tile;
            u32x4* c16 = reinterpret_cast<u32x4*>(chunk);
            if (compact) {                                                         // rows of different envs and slots: dword by dword (bytes for odd S), row by row
                if ((S2 & 3) == 0) {
                    const int nd = S2 >> 2, tot = nd * min(EPB, npairs - pass * EPB);
                    const uint32_t LDS_AS* t32 = (const uint32_t LDS_AS*)tile;
                    for (int q = tid; q < tot; q += EPB) {
                        const int j = (int)__umulhi((uint32_t)(4 * q), a.magicS2), d = q - j * nd;
                        *reinterpret_cast<uint32_t*>(dmap8 + (uint64_t)crow[j] * (uint32_t)S2 + 4u * (uint32_t)d) = t32[q];
                    }
                } else {
                    const int tot = S2 * min(EPB, npairs - pass * EPB);
                    for (int q = tid; q < tot; q += EPB) {
                        const int j = (int)__umulhi((uint32_t)q, a.magicS2);
                        dmap8[(uint64_t)crow[j] * (uint32_t)S2 + (uint32_t)(q - j * S2)] = tile[q];
                    }
                }
            } else if (todo_mask == ~0ull) {                                       // (uniform) every env of the wave is being built: a plain copy
                for (int base = 0; base < npc; base += EPB * PB) {
                    u32x4 r[PB];
#pragma unroll
                    for (int k = 0; k < PB; k++) r[k] = t16[min(base + tid + EPB * k, npc - 1)];
#pragma unroll
                    for (int k = 0; k < PB; k++)
                        if (base + tid + EPB * k < npc) c16[base + tid + EPB * k] = r[k];
                }
            } else {
                // env and cell of a piece's first byte, carried from piece to piece (p += 64 -> 1 024 bytes further)
                uint32_t g = 16u * (uint32_t)tid;
                uint32_t e0 = __umulhi(g, a.magicS2), o0 = g - e0 * (uint32_t)S2;
                const uint32_t de = __umulhi(1024u, a.magicS2), dq = 1024u - de * (uint32_t)S2;
                for (int p = tid; p < npc; p += EPB) {
                    const uint32_t e1 = e0 + (o0 + 15u >= (uint32_t)S2 ? 1u : 0u);
                    const bool t0 = (todo_mask >> e0) & 1ull, t1 = (todo_mask >> (e1 & 63u)) & 1ull;
                    if (t0 || t1) {
                        const u32x4 v = t16[p];
                        if (t0 && t1) c16[p] = v;
                        else {
                            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                            for (uint32_t b = 0; b < 16u; b++)
                                if ((o0 + b < (uint32_t)S2) ? t0 : t1) chunk[g + b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
                        }
                    }
                    g += 1024u; o0 += dq; e0 += de;
                    if (o0 >= (uint32_t)S2) { o0 -= (uint32_t)S2; e0++; }
                }
            }
        }
    }
    // ---- boards mode (the O(1) lidar reads occupancy bit rows, ngw_boards.inc): the rows of the maps just composed, from what this kernel
    //      already holds as bits - the ring, the placed items, the cells the subset pass filled (a wall pass changes no cell's occupancy) -
    //      written into the (now free) tile as [64][BS + 1] words and stored like the maps: the chunk's image, or row by row when compacting
    if (a.boards) {                                                                // (uniform)
        const int BS = a.BS;
        __syncthreads();
        LDS_AS uint32_t* bt = (LDS_AS uint32_t*)(lds + a.off_tile) + tid * (BS + 1);
        if (todo) {
            const uint32_t full = S >= 32 ? 0xFFFFFFFFu : ((1u << S) - 1u), edge = 1u | (1u << (S - 1));
            for (int r = 0; r < BS; r++) {
                uint32_t w = r >= S ? 0u : ((r == 0 || r == S - 1) ? full : edge);
                if (SUBSET && !wallpass && r < S) {
                    const int c0 = r * S, w0 = c0 >> 5, o = c0 & 31;
                    const uint32_t lo = mcol[w0 * EPB], hi = mcol[min(w0 + 1, MW - 1) * EPB];
                    w |= (uint32_t)((((uint64_t)hi << 32) | lo) >> o) & full;
                }
                bt[r] = w;
            }
#pragma unroll
            for (int j = 0; j < PLR; j++)
                if (j < n) {
                    const uint32_t cell = pl[j] >> 8, r = __umulhi(cell, a.magicS);
                    bt[r] |= 1u << (cell - r * (uint32_t)S);
                }
        }
        __syncthreads();
        uint32_t* const dbrd = refill ? a.nx.brd : a.main.brd;
        const LDS_AS uint32_t* t0 = (const LDS_AS uint32_t*)(lds + a.off_tile);
        const int q4 = BS >> 2;                                                    // 16-byte pieces per row
        const uint64_t tm = __ballot(todo);
        if (compact) {
            const int rows = min(EPB, npairs - pass * EPB);
            for (int q = tid; q < rows * q4; q += EPB) {
                const int j = q / q4, part = q - j * q4;
                const LDS_AS uint32_t* sp = t0 + j * (BS + 1) + 4 * part;
                *reinterpret_cast<u32x4*>(dbrd + (uint64_t)crow[j] * (uint32_t)BS + 4u * (uint32_t)part) = u32x4{sp[0], sp[1], sp[2], sp[3]};
            }
        } else {
            u32x4* c16 = reinterpret_cast<u32x4*>(dbrd + ((uint64_t)(refill ? (int64_t)slot * a.nx.stride : 0) + (uint64_t)env0) * (uint32_t)BS);
            for (int q = tid; q < EPB * q4; q += EPB) {
                const int j = q / q4, part = q - j * q4;
                if ((tm >> j) & 1ull) {
                    const LDS_AS uint32_t* sp = t0 + j * (BS + 1) + 4 * part;
                    c16[q] = u32x4{sp[0], sp[1], sp[2], sp[3]};
                }
            }
        }
    }
    STAMP(6);
    // ---- outputs
    if (todo) {
        if (refill) {
            if (!flags) {                                                          // a failed placement leaves the row stale: the real reset raises the flag
                reinterpret_cast<int2*>(dloc)[drow] = int2{r_out, c_out};
                dfac[drow] = f_out;
                dtag[drow] = episode;
            }
        } else {
            reinterpret_cast<int2*>(dloc)[e] = int2{r_out, c_out};
            dfac[e] = f_out;
            a.main.selected[e] = 0;
            a.main.step_count[e] = 0;
            a.main.episode[e] = episode;
            if (flags) atomicOr(a.flags, flags);
        }
    }
    if (!refill) raise_host_flags(a.main.flags_host, (todo && !refill) ? flags : 0u);
    __syncthreads();                                                               // (the next slot reuses the LDS columns)
  }
    if (!refill && a.seq) mirror_wave(dspec, a.main, a.S2, a.K, a.n);              // one-wavefront handles reset by ngw_reset_host: host mirror, then
    if (!refill) signal_host_seq(a.main.flags_host, a.seq);                        // the word the host polls
#ifdef NGW_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    STAMP(7);
    STAMP_FLUSH(a);
#endif
}

}  // namespace
