// ngw_lidar_march.inc - the LidarInFront observation MARCHED over a map in LDS: row formats and the observation tile,
// the constant-offset march of the reference's default 8 beams on 10 x 10, the world-frame and the per-lane-table marches of every other beam count.  (The default 8 beams on
// maps up to 32 x 32 no longer march: ngw_boards.inc finds the first hits on occupancy bit rows.)
#pragma once
#include "ngw_common.inc"

namespace {

// ---------------------------------------------------------------- LidarInFront observation (shared by every kernel that produces it)
// observation_wrappers.py:32-78 on the LDS map.  The wave's 64 rows are built in an LDS tile that is the exact HBM image of
// those rows in the chosen format (NGW_LFMT_*: int32, int16, or uint8 beam entries + an int16 inventory tail) and leave as one
// contiguous run of 16-byte pieces.  Two marches:
//   * WORLD FRAME (num_beams a multiple of 4 - the reference's default 8, and 12, 16; ngw_lidar_configure verifies it entry by
//     entry): the four facings shoot the same rays, numbered from a different start, so the cell offsets of a ray are the same
//     for EVERY lane of the wave - they arrive through scalar loads (no per-lane table reads, no unpacking) and a cell costs
//     one address add and one byte read; all eight rays advance four ranges per round (32 reads in flight) and the wave stops
//     when no lane has an open ray left;
//   * per-lane table (any other beam count): flat int16 offsets [facing][beam][range-1] staged into LDS by the epilogue itself.
// A ray cannot leave the map before it hits the wall ring; cells read beyond the hit are ignored (the LDS layout keeps a
// guard on both sides of the maps for them), and beyond max_range a table repeats the last in-range cell, so a padded entry
// can never be the FIRST non-zero one.
#define CONST_AS __attribute__((address_space(4)))

// A wave alone on its SIMD issues one instruction every ~6 cycles whatever the instruction is (stamped: 1 150 instructions of march in
// 7 100 cycles, with either march), so what the march costs is its INSTRUCTION COUNT.  Per cell: an address add, a byte read and
// three quarters of a pack; per ray and round, three instructions that remember the first non-zero word; the hit itself is resolved
// once per ray, after the rounds.
//
// Four cells of one ray as one dword, bytes in range order: four byte reads and three shift-ors.  (The d16 forms of the byte read -
// two reads filling the halves of one register, one shift-or per four cells - are no use on this part: with SRAM ECC on, a d16 load
// ZEROES the other half of its destination instead of preserving it, which is why the compiler never emits them here; tried through
// inline asm, every observation came out wrong.)
__device__ __forceinline__ uint32_t lidar_cells4(const LDS_AS uint8_t* ag, int o0, int o1, int o2, int o3) {
    const uint32_t c0 = ag[o0], c1 = ag[o1], c2 = ag[o2], c3 = ag[o3];
    return (c0 | (c1 << 8)) | ((c2 | (c3 << 8)) << 16);
}

// Eight rays, one round of four ranges each (k0 + 1 .. k0 + 4): `first` keeps a ray's first non-zero word, `kc` the round it came
// from.  Returns whether any of the eight is still open in this lane.
__device__ __forceinline__ bool lidar_round(const uint32_t (&word)[8], int k0, uint32_t (&first)[8], int (&kc)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const bool take = first[i] == 0;
        first[i] = take ? word[i] : first[i];
        kc[i] = take ? k0 : kc[i];
    }
    const uint32_t m = min(min(min(first[0], first[1]), min(first[2], first[3])), min(min(first[4], first[5]), min(first[6], first[7])));
    return m == 0;
}

// The hits of up to eight rays (observation_wrappers.py:59-64: the first non-air block = the lowest non-zero byte of the ray's first
// non-zero word) go into the row: the channel look-ups go out together (a ray without a hit looks up item 0 = air = no channel), a
// beam entry is a range <= 64, so ONE byte store at the entry's place serves every row format (the tile was zeroed, rows are
// little-endian; `sh` = log2 of the entry size), and a ray that reports nothing stores into the lane's dump byte behind the tile -
// no branch per ray.
__device__ __forceinline__ void lidar_hits(const uint32_t (&first)[8], const int (&kc)[8], int pos0 /* row entry of ray slot 0's beam: beam * NC */,
                                           int nb, int R, int NC, int wrap /* num_beams * NC */, int sh, const LDS_AS uint8_t* chan_of_item,
                                           LDS_AS uint8_t* rowp, int dump) {
    int hk[8], ch[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int q = (__ffs((int)(first[i] | 0x80000000u)) - 1) >> 3;
        hk[i] = kc[i] + q + 1;
        ch[i] = chan_of_item[(first[i] >> (8 * q)) & 255u];                        // (first == 0: item 0)
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int p = pos0 + i * NC;                                                     // consecutive ray slots are consecutive beams (mod num_beams)
        p -= p >= wrap ? wrap : 0;
        const bool hit = i < nb && ch[i] != 0 && hk[i] <= R;
        rowp[hit ? (p + ch[i] - 1) << sh : dump] = (uint8_t)hk[i];
    }
}

// The constant-offset march (NgwLaunch::l_world == 2): the reference's default 8 rays on an S x S map with S a compile-time
// constant.  What bounds a march is the LDS itself: every ray cell is a byte read at a per-lane address (the agents stand
// anywhere, so the 64 addresses of a read fall on the banks at random: ~3.5-way conflicts), and the four waves of a CU share one LDS
// pipe - stamped: ~25 cycles per read instruction, 104 of them in the table-driven marches = 2 600 of their 4 100 cycles, whatever
// the arithmetic around them looked like.  So this form issues FEWER reads:
//   * a diagonal ray advances by round(0.71 k) cells: ranges 1..11 visit the 8 diagonal cells d = 1..8, some twice; the first block
//     is the same either way, so rays are walked in GEOMETRIC steps d = 1..8 (8 cells per ray, not 11) and the range reported is the
//     first k that reaches d (a 4-bit-per-entry constant: 1 3 4 5 7 8 10 11); an axis ray cannot run further than S - 2 = 8 cells;
//   * every address is the agent's cell + an instruction immediate: no address arithmetic, no offset table, no loop.
// 64 byte reads per lane instead of 104.  (Tried: one 8-byte read for each of the two rays along the agent's row and one 4- / 8-byte
// read per neighbouring row for the three rays that cross it - 38 reads; the LDS takes unaligned wide reads, but at ~65 cycles
// apiece: 3 000 cycles for the 38.)  The reads are inline asm (the compiler folds the bias of the negative offsets back into adds and
// packs bytes through v_and / v_perm thickets); ngw_lidar_configure checks the host's ray table against ngw_lidar8_dr / _dc.
template <int OFF>
__device__ __forceinline__ uint32_t lds_u8_imm(const LDS_AS uint8_t* base) {
    static_assert(OFF >= 0 && OFF < 65536, "DS immediates are unsigned 16-bit");
    uint32_t v;
    asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(v) : "v"(base), "n"(OFF));
    return v;                                                                      // (zero-extended)
}
// byte 0 of a | byte 0 of b << 8 | byte 0 of c << 16 | byte 0 of d << 24 (the values are zero-extended bytes: three shift-ors)
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a | (b << 8)) | ((c | (d << 8)) << 16); }

template <int S, int DR, int DC>
__device__ __forceinline__ void lidar_ray8(const LDS_AS uint8_t* agb, uint32_t (&c)[8]) {
    constexpr int BIAS = 8 * (S + 1);
#define NGW_O(d) (BIAS + (d) * (DR * S + DC))
    c[0] = lds_u8_imm<NGW_O(1)>(agb); c[1] = lds_u8_imm<NGW_O(2)>(agb); c[2] = lds_u8_imm<NGW_O(3)>(agb); c[3] = lds_u8_imm<NGW_O(4)>(agb);
    c[4] = lds_u8_imm<NGW_O(5)>(agb); c[5] = lds_u8_imm<NGW_O(6)>(agb); c[6] = lds_u8_imm<NGW_O(7)>(agb); c[7] = lds_u8_imm<NGW_O(8)>(agb);
#undef NGW_O
}

template <int S>
__device__ __forceinline__ void lidar_march_const8(const NgwLaunch& a, const LDS_AS uint8_t* ag, int f, int NC, int sh, const LDS_AS uint8_t* chan_of_item,
                                                   LDS_AS uint8_t* rowp, int dump) {
    static_assert(S - 2 == 8, "eight geometric steps per ray: two words");
    static_assert(8 * (S + 1) <= 11 * (S + 1), "inside the LDS guard (11 * (S + 1) bytes on both sides of the maps)");
    const LDS_AS uint8_t* agb = ag - 8 * (S + 1);                                  // (immediates are unsigned)
    // world rays in table order: 0 (+d, 0)  1 (+d, +d)  2 (0, +d)  3 (-d, +d)  4 (-d, 0)  5 (-d, -d)  6 (0, -d)  7 (+d, -d)
    uint32_t c[8][8];
    lidar_ray8<S, 1, 0>(agb, c[0]); lidar_ray8<S, 1, 1>(agb, c[1]); lidar_ray8<S, 0, 1>(agb, c[2]); lidar_ray8<S, -1, 1>(agb, c[3]);
    lidar_ray8<S, -1, 0>(agb, c[4]); lidar_ray8<S, -1, -1>(agb, c[5]); lidar_ray8<S, 0, -1>(agb, c[6]); lidar_ray8<S, 1, -1>(agb, c[7]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                             // one wait for all 64 reads ...
#pragma unroll
    for (int w = 0; w < 8; w++)                                                    // ... and every value pinned behind it (no instruction; the compiler does not count asm reads)
        asm volatile("" : "+v"(c[w][0]), "+v"(c[w][1]), "+v"(c[w][2]), "+v"(c[w][3]), "+v"(c[w][4]), "+v"(c[w][5]), "+v"(c[w][6]), "+v"(c[w][7]));
    STAMP_SUB(a, 2);
    const int uf = f == 0 ? 4 : (f == 1 ? 0 : (f == 2 ? 6 : 2));                   // NORTH pi, SOUTH 0, WEST 3 pi / 2, EAST pi / 2 in units of pi / 4 (:38)
    int pos = ((4 - uf) & 7) * NC;                                                 // beam b = (world ray + rot) mod 8; its row entries start at b * NC
    const int wrap = 8 * NC;
    int hk[8], ch[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const uint32_t lo = pack4(c[w][0], c[w][1], c[w][2], c[w][3]), hi = pack4(c[w][4], c[w][5], c[w][6], c[w][7]);
        const uint32_t t = lo ? lo : hi;                                           // (the wall ring stops every ray within 8 cells: t != 0)
        const int q = (__ffs((int)(t | 0x80000000u)) - 1) >> 3;
        const int d = (lo ? 0 : 4) + q;                                            // geometric distance - 1
        hk[w] = (w & 1) ? (int)((0xBA875431u >> (4 * d)) & 15u) : d + 1;          // a diagonal reports the first range k with round(0.71 k) = d + 1
        ch[w] = chan_of_item[(t >> (8 * q)) & 255u];
    }
    STAMP_SUB(a, 6);
#pragma unroll
    for (int w = 0; w < 8; w++) {
        rowp[ch[w] ? (pos + ch[w] - 1) << sh : dump] = (uint8_t)hk[w];
        pos += NC;
        pos -= pos >= wrap ? wrap : 0;
    }
}

// One workgroup IS one wavefront here (NGW_EPB == 64), and a wave's LDS operations execute in program order: a lane reading what
// another lane of the same wave wrote earlier needs no hardware wait, only the compiler must not reorder the accesses.
// __syncthreads() would also drain every outstanding GLOBAL store of the wave (s_waitcnt vmcnt(0)): ~500 cycles after the step's
// output stores, three times per lidar epilogue.
__device__ __forceinline__ void wave_lds_sync() {
    static_assert(NGW_EPB == 64, "one wavefront per workgroup");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void lidar_march_world(const LDS_AS uint8_t* ag, int f, int B, int R, int NC, int sh, const NgwLidarDev* cfg,
                                                  const LDS_AS uint8_t* chan_of_item, LDS_AS uint8_t* rowp, int dump) {
    const CONST_AS int32_t* woff = (const CONST_AS int32_t*)(const void*)&cfg->woff[0][0];   // uniform addresses: scalar loads
    const int half = B >> 1, quarter = B >> 2;
    const int uf = f == 0 ? half : (f == 1 ? 0 : (f == 2 ? half + quarter : quarter));     // NORTH pi, SOUTH 0, WEST 3 pi / 2, EAST pi / 2 (:38)
    int rot = half - uf;                                                                  // beam b = (world ray + rot) mod B
    rot += rot < 0 ? B : 0;
    for (int w0 = 0; w0 < B; w0 += 8) {
        uint32_t first[8];
        int kc[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { first[i] = 0; kc[i] = 0; }
        // Scalar loads and LDS reads share one counter (lgkmcnt) and scalar loads return out of order, so a wait for offsets drains
        // the cell reads too.  Hence the order below: the cell reads of this round go out, THEN the offsets of the next round are
        // requested, and one wait covers both (left alone, the scheduler interleaved them: four full drains per round).
        int o[8][4];
#pragma unroll
        for (int i = 0; i < 8; i++) {                                                       // (a ray slot beyond B repeats ray B - 1)
            const CONST_AS int32_t* t = woff + min(w0 + i, B - 1) * NGW_LIDAR_MAX_RANGE;
            o[i][0] = t[0]; o[i][1] = t[1]; o[i][2] = t[2]; o[i][3] = t[3];
        }
        for (int k0 = 0; k0 < R; k0 += 4) {
            uint32_t c[8][4];
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) c[i][j] = ag[o[i][j]];
            __builtin_amdgcn_sched_barrier(0);
            const int kn = min(k0 + 4, NGW_LIDAR_MAX_RANGE - 4);                            // (the last round re-requests in-table entries nobody uses)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const CONST_AS int32_t* t = woff + min(w0 + i, B - 1) * NGW_LIDAR_MAX_RANGE + kn;
                o[i][0] = t[0]; o[i][1] = t[1]; o[i][2] = t[2]; o[i][3] = t[3];
            }
            __builtin_amdgcn_sched_barrier(0);
            uint32_t word[8];
#pragma unroll
            for (int i = 0; i < 8; i++) word[i] = (c[i][0] | (c[i][1] << 8)) | ((c[i][2] | (c[i][3] << 8)) << 16);
            if (!__any(lidar_round(word, k0, first, kc))) break;
        }
        int b0 = w0 + rot;
        b0 -= b0 >= B ? B : 0;
        lidar_hits(first, kc, b0 * NC, B - w0, R, NC, B * NC, sh, chan_of_item, rowp, dump);
    }
}

// Per-lane table form: flat int16 offsets [facing][beam][range-1] in LDS; eight rays advance four ranges per round (8 table
// reads of 4 offsets each, then 32 cell reads in flight).
__device__ __forceinline__ void lidar_march_table(const LDS_AS uint8_t* ag, int f, int B, int R, int NC, int sh, const LDS_AS int16_t* toff,
                                                  const LDS_AS uint8_t* chan_of_item, LDS_AS uint8_t* rowp, int dump) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    for (int b0 = 0; b0 < B; b0 += 8) {
        uint32_t first[8];
        int kc[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { first[i] = 0; kc[i] = 0; }
        for (int k0 = 0; k0 < R; k0 += 4) {
            u32x2 o[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                o[i] = *reinterpret_cast<const LDS_AS u32x2*>(toff + (f * NGW_LIDAR_MAX_BEAMS + min(b0 + i, B - 1)) * NGW_LIDAR_MAX_RANGE + k0);
            uint32_t word[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                word[i] = lidar_cells4(ag, (int16_t)(o[i].x & 0xFFFFu), (int16_t)(o[i].x >> 16), (int16_t)(o[i].y & 0xFFFFu), (int16_t)(o[i].y >> 16));
            if (!__any(lidar_round(word, k0, first, kc))) break;
        }
        lidar_hits(first, kc, b0 * NC, B - b0, R, NC, B * NC, sh, chan_of_item, rowp, dump);
    }
}

constexpr int LIDAR_TAB16 = 4 * NGW_LIDAR_MAX_BEAMS * NGW_LIDAR_MAX_RANGE * 2 / 16;     // per-lane ray table = 512 pieces of 16 B
constexpr int LIDAR_ITEM_DW = 2 * NGW_MAX_ITEMS / 4;                                    // chan_of_item | inv_item
static_assert(LIDAR_TAB16 == 8 * NGW_EPB, "ray table is 8 pieces per lane");
static_assert(offsetof(NgwLidarDev, chan_of_item) == 16 * LIDAR_TAB16 && offsetof(NgwLidarDev, inv_item) == 16 * LIDAR_TAB16 + NGW_MAX_ITEMS,
              "lidar tables are contiguous");

// The observation of the wave's 64 envs: `agent` = the lane's agent cell in its LDS map, `inv` = its inventory row in LDS; the two
// item tables are in LDS at a.off_litem (the caller's prologue put them there).  Whole-wave call (barriers inside).
// The observation tile starts as zeros.  A step kernel does this in its PROLOGUE, while its global loads are in flight (the wave has
// nothing else to do there for ~1 100 cycles); only a launch whose cold path used the tile's region for something else (the reset
// path's Philox ring shares it) zeroes it again in the epilogue.
__device__ __forceinline__ void lidar_zero_tile(const NgwLaunch& a, uint32_t* lds, int tid) {
    const int npc = 4 * a.l_rb;
    LDS_AS u32x4* t4 = (LDS_AS u32x4*)(lds + a.off_ltile);
    for (int base = 0; base < npc; base += EPB * 4) {                              // (a piece index beyond the tile zeroes the last piece again)
#pragma unroll
        for (int j = 0; j < 4; j++) t4[min(base + tid + EPB * j, npc - 1)] = u32x4{0u, 0u, 0u, 0u};
    }
}

// Inside a T-loop (the TRAJ forms of ngw_slot_rollout_kernel / ngw_playout_kernel: one call per step) two things differ, both defaulted so that
// every other caller compiles to what it always did: tab_staged = the caller staged the per-lane ray table ONCE with lidar_stage_table (the
// table does not change between the calls: T copies of 8 KiB saved), and tile_out = where THIS call's 64-row tile goes (nullptr: rows
// 64 * blockIdx.x .. of a.lout).
__device__ __forceinline__ void lidar_stage_table(const NgwLaunch& a, uint32_t* lds, int tid) {
    const u32x4* src = reinterpret_cast<const u32x4*>(a.lcfg->off);
    LDS_AS u32x4* dst = (LDS_AS u32x4*)(lds + a.off_ltab);
    u32x4 tb[8];
#pragma unroll
    for (int j = 0; j < 8; j++) tb[j] = src[tid + EPB * j];
#pragma unroll
    for (int j = 0; j < 8; j++) dst[tid + EPB * j] = tb[j];
}

__device__ __forceinline__ void lidar_epilogue(const NgwLaunch& a, uint32_t* lds, int tid, bool live, const int8_t* agent, int f, const int32_t* inv,
                                               bool zeroed = false, bool tab_staged = false, char* tile_out = nullptr) {
    const int B = a.l_beams, R = a.l_range, NC = a.l_chan, NI = a.l_inv, rb = a.l_rb, npc = 4 * rb;   // 64 rows = 4 * rb pieces of 16 B
    const int sh = a.l_fmt == NGW_LFMT_I32 ? 2 : (a.l_fmt == NGW_LFMT_I16 ? 1 : 0);                   // beam entry = 1 << sh bytes
    LDS_AS u32x4* t4 = (LDS_AS u32x4*)(lds + a.off_ltile);
    wave_lds_sync();
    STAMP_SUB(a, 0);
    if (!zeroed) lidar_zero_tile(a, lds, tid);
    if (!tab_staged && !a.l_world) lidar_stage_table(a, lds, tid);                 // (uniform) the per-lane ray table, staged now: 8 KiB
    wave_lds_sync();
    STAMP_SUB(a, 1);
    const LDS_AS uint8_t* chan_of_item = (const LDS_AS uint8_t*)(lds + a.off_litem);
    LDS_AS uint8_t* rowp = (LDS_AS uint8_t*)(lds + a.off_ltile) + tid * rb;
    if (live) {
        const LDS_AS uint8_t* ag = (const LDS_AS uint8_t*)agent;
        const int dump = EPB * rb - tid * rb + tid;                                // the 64 bytes behind the tile: one per lane
        if (a.l_world == 2) lidar_march_const8<NGW_LIDAR_CONST_S>(a, ag, f, NC, sh, chan_of_item, rowp, dump);     // (the host checked table and range: R = 11)
        else if (a.l_world) lidar_march_world(ag, f, B, R, NC, sh, a.lcfg, chan_of_item, rowp, dump);
        else lidar_march_table(ag, f, B, R, NC, sh, (const LDS_AS int16_t*)(lds + a.off_ltab), chan_of_item, rowp, dump);
    }
    STAMP_SUB(a, 3);
    if (live) {
        // the inventory tail (:74-75): the item ids sit in LDS behind the channel table (every lane reads the same six dwords: broadcast
        // reads), an entry is then one read of the lane's inventory row and one store; eight entries in flight
        const LDS_AS uint32_t* idw = (const LDS_AS uint32_t*)(chan_of_item + NGW_MAX_ITEMS);
        uint32_t iw[NGW_MAX_ITEMS / 4];
#pragma unroll
        for (int i = 0; i < NGW_MAX_ITEMS / 4; i++) iw[i] = idw[i];
        const LDS_AS int32_t* iv = (const LDS_AS int32_t*)inv;
        LDS_AS uint8_t* tail = rowp + a.l_invoff;
        const bool wide = a.l_fmt == NGW_LFMT_I32;
#pragma unroll
        for (int j0 = 0; j0 < NGW_MAX_ITEMS; j0 += 8) {
            if (j0 < NI) {                                                         // (uniform)
                int cnt[8];
#pragma unroll
                for (int i = 0; i < 8; i++) cnt[i] = iv[(iw[(j0 + i) >> 2] >> (8 * ((j0 + i) & 3))) & 255u];   // (entries beyond NI name item 0)
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if (j0 + i < NI) {
                        if (wide) *(LDS_AS int32_t*)(tail + 4 * (j0 + i)) = cnt[i];
                        else *(LDS_AS uint16_t*)(tail + 2 * (j0 + i)) = (uint16_t)min(cnt[i], 32767);
                    }
            }
        }
    }
    wave_lds_sync();
    STAMP_SUB(a, 4);
    GLOBAL_AS u32x4* g4 = (GLOBAL_AS u32x4*)(tile_out ? tile_out : reinterpret_cast<char*>(a.lout) + (uint64_t)blockIdx.x * (uint32_t)(EPB * rb));
    for (int base = 0; base < npc; base += EPB * 4) {                              // four pieces per lane in flight
        u32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = t4[min(base + tid + EPB * j, npc - 1)];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (base + tid + EPB * j < npc) g4[base + tid + EPB * j] = v[j];
    }
    STAMP_SUB(a, 5);
}

}  // namespace
