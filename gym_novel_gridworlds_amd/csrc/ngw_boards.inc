// ngw_boards.inc — the O(1) LidarInFront observation on occupancy bit rows (the in-place step kernel of ngw_lean.inc
// fuses lidar_boards_rows as its epilogue).
#pragma once
#include "ngw_common.inc"
#include "ngw_lidar_march.inc"     // the row formats and the observation tile

namespace {
//
// The reference's default LidarInFront (observation_wrappers.py:10-80, num_beams = 8) shoots the four axes and the four true
// diagonals: np.round(np.cos(pi / 4), 2) = 0.71 for BOTH coordinates and round(0.71 k) is the same number for the row and the
// column (:49-55), so a ray only ever visits cells of the agent's row, column, diagonal or anti-diagonal, in geometric order.  What a
// beam reports is the FIRST non-air block on its line and the first range k that reaches it: distance d itself on an axis, the first
// k with round(0.71 k) = d on a diagonal (ngw_lidar_configure compares the host's table with ngw_lidar8_dr / _dc for every range and
// this closed form for every distance: only an exact match switches this path on).
//
// So instead of marching over a map staged through LDS (64 - 336 scattered LDS byte reads per lane, S*S bytes per env through LDS:
// 7.3 us per batched step at 10 x 10, 15 at 20 x 20, 40 at 32 x 32 against 3.7 - 4.7 us for the plain in-place step), the state carries
// one OCCUPANCY BIT ROW per map row (NgwBufs::brd: bit c of word r = map[r][c] != 0; S words of S <= 32 bits per env):
//   * the lane's words arrive with the step kernel's prologue loads (their address does not depend on the pose);
//   * the agent's column, diagonal and anti-diagonal are cut out of them in registers: bit k of the line = one bit field of word k
//     (v_bfe_u32 + v_lshl_or_b32 per row: no memory, no LDS);
//   * a ray's first block is one shift / mask and one find-first-bit on its line (the wall ring stops every ray);
//   * ONE byte read per ray - the hit cell's item id, from the map row in HBM - names the channel.
// 8 byte reads per env instead of 64 - 336, nothing staged, the in-place step kernel stays, and the cost no longer depends on S*S.
// Other beam counts keep the marches of ngw_lidar_march.inc.

constexpr uint32_t LIDAR8_MAGIC71 = 60492498u;                                     // ceil(2^32 / 71): x / 71 == umulhi(x, .) for x < 2^15
// first range k with round(0.71 k) = d (d >= 1): floor((100 d + 20) / 71); checked against the host's table by ngw_lidar_configure
__device__ __forceinline__ int lidar8_first_range(int d) { return (int)__umulhi((uint32_t)(100 * d + 20), LIDAR8_MAGIC71); }

// distance to the first set bit above / below position p of a line word (the caller guarantees one exists: wall bits)
__device__ __forceinline__ int line_up(uint32_t w, int p) { return (int)__builtin_ctz((w >> (p + 1)) | 0x80000000u) + 1; }
__device__ __forceinline__ int line_dn(uint32_t w, int p) { return p - 31 + (int)__builtin_clz((w & ((1u << p) - 1u)) | 1u); }

// The agent's column, diagonal and anti-diagonal as line words indexed by ROW: bit k = occupancy of the line's cell in row k.
// R[k] = bit row k of the env (rows >= S are zero words).  A bit field whose column falls outside the map reads whatever bit
// (offset mod 32) holds: such cells lie beyond the wall ring on their line, and a ray stops at the ring (line_up / line_dn take the
// FIRST set bit from the agent outwards).  Bits 0 and S - 1 are the ring's rows: always occupied.
template <int NR>
__device__ __forceinline__ uint32_t board_col(const uint32_t (&R)[NR], int S, int nc) {
    uint32_t cw = 0;
#pragma unroll
    for (int k = 1; k < NR; k++) cw = (__builtin_amdgcn_ubfe(R[k], (uint32_t)nc, 1u) << k) | cw;
    return cw | 1u | (1u << (S - 1));
}
// Every row rotated by its own index - right (Rd[k] bit j = R[k] bit (j + k) mod 32) and left (Ra[k] bit j = R[k] bit (j - k) mod 32): the
// cell of the agent's diagonal in row k is column nc - nr + k, of its anti-diagonal nc + nr - k, i.e. bit (nc - nr) mod 32 of Rd[k] and bit
// (nc + nr) mod 32 of Ra[k] - ONE position for every row (two instructions per row and line instead of three).
template <int NR>
__device__ __forceinline__ void board_rotate(const uint32_t (&R)[NR], uint32_t (&Rd)[NR], uint32_t (&Ra)[NR]) {
#pragma unroll
    for (int k = 1; k < NR; k++) {
        Rd[k] = __builtin_amdgcn_alignbit(R[k], R[k], (uint32_t)k);
        Ra[k] = __builtin_amdgcn_alignbit(R[k], R[k], (uint32_t)(32 - k));
    }
}
template <int NR>
__device__ __forceinline__ void board_diags(const uint32_t (&Rd)[NR], const uint32_t (&Ra)[NR], int S, int nr, int nc, uint32_t& dgw, uint32_t& anw) {
    uint32_t dw = 0, aw = 0;
    const uint32_t sd = (uint32_t)(nc - nr) & 31u, sa = (uint32_t)(nc + nr) & 31u;
#pragma unroll
    for (int k = 1; k < NR; k++) {
        dw = (__builtin_amdgcn_ubfe(Rd[k], sd, 1u) << k) | dw;
        aw = (__builtin_amdgcn_ubfe(Ra[k], sa, 1u) << k) | aw;
    }
    const uint32_t ring = 1u | (1u << (S - 1));
    dgw = dw | ring; anw = aw | ring;
}

// What a step changed on the agent's lines AFTER the bit rows were loaded (the in-place step kernel's hot tail): bits to clear / set on the
// column, bits to clear on the two diagonals (a cell write sits on the agent's row or column; an entity pick-up clears cells one step away).
struct BoardPatch { uint32_t col_clr, col_set, dg_clr, an_clr; };

// Rows of the LidarInFront observation of the wave's 64 envs from the bit rows: lines cut, rays resolved, hit cells read from the map rows
// in HBM (`gmap` + `mapoff` = the lane's row, S2 bytes), beam entries and the inventory tail written into the wave's LDS tile (zeroed by
// the caller: lidar_zero_tile), the tile stored as the rows' HBM image.  `inv` = the lane's inventory row in LDS, `roww` = the bit row the
// agent stands in (with the ring's bits); the channel table is in LDS at a.off_litem; id0 / id1 = the first eight inventory-tail item ids
// (NgwLidarDev::inv_item, uniform: the caller fetched them with its prologue).  Whole-wave call.  Order of work = order of need: the
// inventory counts and the AXIS rays' hit cells are requested first (column line: 2 instructions per row), the diagonals are cut while those
// are in flight, everything that does not depend on a hit cell's item is computed before the first wait for one.
template <int NR>
__device__ __forceinline__ void lidar_boards_rows(const NgwLaunch& a, uint32_t* lds, int tid, const uint32_t (&R)[NR], const uint32_t (&Rd)[NR], const uint32_t (&Ra)[NR],
                                                  uint32_t roww, const BoardPatch pt,
                                                  int S, int S2, int nr, int nc, int nf, const char* gmap, uint32_t mapoff, const int32_t* inv,
                                                  uint32_t id0, uint32_t id1, uint32_t blk /* the wave's block among a.lout's rows */,
                                                  uint8_t* hrows = nullptr /* host write-through: the same rows into the caller's page-locked buffer too */) {
    const int NC = a.l_chan, NI = a.l_inv, rb = a.l_rb, npc = 4 * rb, Rmax = a.l_range;
    const int sh = a.l_fmt == NGW_LFMT_I32 ? 2 : (a.l_fmt == NGW_LFMT_I16 ? 1 : 0);
    const bool wide = a.l_fmt == NGW_LFMT_I32;
    LDS_AS uint8_t* rowp = (LDS_AS uint8_t*)(lds + a.off_ltile) + tid * rb;
    const int dump = EPB * rb - tid * rb + 4 * tid;                                // the 64 dwords behind the tile: one per lane (what reports nothing is stored there)
    const LDS_AS int32_t* iv = (const LDS_AS int32_t*)inv;
    // ---- the inventory tail's first eight counts (:74-75): requested now, stored below
    int cnt[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cnt[i] = iv[((i < 4 ? id0 : id1) >> (8 * (i & 3))) & 255u];           // (entries beyond NI name item 0)
    // ---- the eight rays in world order (ngw_lidar8_dr / _dc): 0 (+r, 0)  1 (+r, +c)  2 (0, +c)  3 (-r, +c)  4 (-r, 0)  5 (-r, -c)  6 (0, -c)  7 (+r, -c)
    const int ac = nr * S + nc;
    // (hit cells: scalar base + 32-bit lane offset; clamped - a map whose ring somebody opened with ngw_set_state must not send a read outside the row)
#ifdef NGW_EXP_NOHIT
    auto hit_item = [&](int d, int stride) -> uint32_t { return (uint32_t)((d + stride) & 7); };
#else
    auto hit_item = [&](int d, int stride) -> uint32_t {
        return (uint32_t)*(const GLOBAL_AS uint8_t*)((const GLOBAL_AS char*)gmap + (mapoff + min((uint32_t)(ac + d * stride), (uint32_t)(S2 - 1))));
    };
#endif
    int d[8];
    uint32_t item[8];
    const uint32_t colw = (board_col<NR>(R, S, nc) & ~pt.col_clr) | pt.col_set;
    d[0] = line_up(colw, nr); d[2] = line_up(roww, nc); d[4] = line_dn(colw, nr); d[6] = line_dn(roww, nc);
    item[0] = hit_item(d[0], S); item[2] = hit_item(d[2], 1); item[4] = hit_item(d[4], -S); item[6] = hit_item(d[6], -1);
    uint32_t dgw, anw;
    board_diags<NR>(Rd, Ra, S, nr, nc, dgw, anw);
    dgw &= ~pt.dg_clr; anw &= ~pt.an_clr;
    d[1] = line_up(dgw, nr); d[3] = line_dn(anw, nr); d[5] = line_dn(dgw, nr); d[7] = line_up(anw, nr);
    item[1] = hit_item(d[1], S + 1); item[3] = hit_item(d[3], 1 - S); item[5] = hit_item(d[5], -S - 1); item[7] = hit_item(d[7], S - 1);
    // ---- the inventory tail, branch-free: an entry beyond NI goes to the lane's dump dword
    {
        const int esz = wide ? 4 : 2, toff = a.l_invoff;
        if (wide) {
#pragma unroll
            for (int i = 0; i < 8; i++) *(LDS_AS int32_t*)(rowp + (i < NI ? toff + esz * i : dump)) = cnt[i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) *(LDS_AS uint16_t*)(rowp + (i < NI ? toff + esz * i : dump)) = (uint16_t)min(cnt[i], 32767);
        }
        if (NI > 8) {                                                              // (uniform) more than eight breakable items: the ids from the lidar config
            const CONST_AS uint32_t* idw = (const CONST_AS uint32_t*)(const void*)a.lcfg->inv_item;
            for (int j0 = 8; j0 < NI; j0 += 8) {
                const uint32_t iw0 = idw[j0 >> 2], iw1 = idw[(j0 >> 2) + 1];
                int c2[8];
#pragma unroll
                for (int i = 0; i < 8; i++) c2[i] = iv[((i < 4 ? iw0 : iw1) >> (8 * (i & 3))) & 255u];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int o = j0 + i < NI ? toff + esz * (j0 + i) : dump;
                    if (wide) *(LDS_AS int32_t*)(rowp + o) = c2[i]; else *(LDS_AS uint16_t*)(rowp + o) = (uint16_t)min(c2[i], 32767);
                }
            }
        }
    }
    // ---- what a hit writes and where, as far as it does not depend on the block's item: the range (:52-64) and the beam's row entries
    const int uf = nf == 0 ? 4 : (nf == 1 ? 0 : (nf == 2 ? 6 : 2));               // NORTH pi, SOUTH 0, WEST 3 pi / 2, EAST pi / 2 in units of pi / 4 (:38)
    int hk[8], base[8];
    {
        int pos = ((4 - uf) & 7) * NC;                                             // beam b = (world ray + rot) mod 8; its row entries start at b * NC
        const int wrap = 8 * NC;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            hk[w] = (w & 1) ? lidar8_first_range(d[w]) : d[w];
            base[w] = hk[w] <= Rmax ? pos - 1 : -0x10000;                           // beyond max_beam_range the reference's loop has ended (:52): reports nothing
            pos += NC;
            pos -= pos >= wrap ? wrap : 0;
        }
    }
    STAMP_SUB(a, 2);
    STAMP_SUBV(a, 6);
    // ---- hits: channel of the block (0 = not a lidar item: reports nothing), one byte store at the entry's place (rows are little-endian, the tile was zeroed)
    const LDS_AS uint8_t* chan_of_item = (const LDS_AS uint8_t*)(lds + a.off_litem);
    int ch[8];
#pragma unroll
    for (int w = 0; w < 8; w++) ch[w] = chan_of_item[min(item[w], (uint32_t)(NGW_MAX_ITEMS - 1))];
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const int e = base[w] + ch[w];
        rowp[(ch[w] != 0 && e >= 0) ? e << sh : dump] = (uint8_t)hk[w];
    }
    wave_lds_sync();
    STAMP_SUB(a, 3);
#ifdef NGW_EXP_NOROWS
    return;
#endif
    LDS_AS u32x4* t4 = (LDS_AS u32x4*)(lds + a.off_ltile);
    GLOBAL_AS u32x4* g4 = (GLOBAL_AS u32x4*)(reinterpret_cast<char*>(a.lout) + (uint64_t)blk * (uint32_t)(EPB * rb));
    for (int base4 = 0; base4 < npc; base4 += EPB * 4) {                           // four pieces per lane in flight
        u32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = t4[min(base4 + tid + EPB * j, npc - 1)];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (base4 + tid + EPB * j < npc) g4[base4 + tid + EPB * j] = v[j];
        if (hrows) {                                                               // (uniform)
            char* const hb = reinterpret_cast<char*>(hrows) + (uint64_t)blk * (uint32_t)(EPB * rb);   // (system-scope stores: ngw_lean.inc stgs16)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (base4 + tid + EPB * j < npc) stgs16(hb, 16u * (uint32_t)(base4 + tid + EPB * j), v[j]);
        }
    }
    STAMP_SUB(a, 5);
}

// The lane's NR bit rows out of NR / 4 loaded quads.
template <int NR>
__device__ __forceinline__ void board_unpack(const u32x4 (&bq)[NR / 4], uint32_t (&R)[NR]) {
#pragma unroll
    for (int j = 0; j < NR / 4; j++) { R[4 * j] = bq[j].x; R[4 * j + 1] = bq[j].y; R[4 * j + 2] = bq[j].z; R[4 * j + 3] = bq[j].w; }
}

// One env's bit rows from its byte map in GLOBAL memory, by the lane that owns it (the in-place step kernel's fallback: a reset that found
// no prepared episode ran the placement loop on the env's map row in HBM - slow, rare).
__device__ __forceinline__ void board_build_lane_global(const GLOBAL_AS int8_t* gm, GLOBAL_AS uint32_t* brow, int S, int BS) {
    for (int r = 0; r < BS; r++) {
        uint32_t w = 0;
        if (r < S)
            for (int c = 0; c < S; c++) w |= (gm[r * S + c] != 0 ? 1u : 0u) << c;
        brow[r] = w;
    }
}

// ---------------------------------------------------------------- bit rows of a whole buffer set from its maps
// ngw_boards_kernel: after every launch that rewrites maps wholesale while the boards mode is on (explicit resets, refills of the prepared
// episodes, fused rollouts, ngw_set_state) and when the mode is switched on.  Wave = 64 consecutive map rows of `map` ([rows][S2], rows a
// multiple of 64): staged through LDS with the usual coalesced pieces, every lane packs its own map (four cells per LDS dword read when
// rows are dword-aligned: item ids are < 128, so byte != 0 <=> bit 7 of byte + 0x7F, and one multiply gathers the four bits), the words go
// into an LDS tile and leave as the chunk's contiguous image.
template <int MAPMODE>
__global__ void __launch_bounds__(NGW_EPB) ngw_boards_kernel(const NgwLaunch a, const int8_t* __restrict__ map, uint32_t* __restrict__ brd) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    const int64_t env0 = (int64_t)blockIdx.x * EPB;
    const int S = a.S, S2 = a.S2, BS = a.BS, npieces = 4 * S2;
    uint32_t* lds_map = lds + a.off_map;
    u32x4 buf[PB];
    const u32x4* gin = reinterpret_cast<const u32x4*>(map + env0 * S2);
    for (int base = 0; base < npieces; base += EPB * PB) {
        pieces_load(buf, gin, base, npieces, tid);
        pieces_lds<true, MAPMODE>(buf, a, lds_map, base, npieces, tid);
    }
    __syncthreads();
    const LDS_AS uint8_t* mp = (const LDS_AS uint8_t*)(reinterpret_cast<int8_t*>(lds_map) + tid * a.MS);
    LDS_AS uint32_t* tile = (LDS_AS uint32_t*)(lds + a.off_ltile) + tid * (BS + 1);   // [64][BS + 1]: odd stride, conflict-free per-lane writes
    if ((S & 3) == 0) {
        const LDS_AS uint32_t* m4 = (const LDS_AS uint32_t*)mp;
        const int dpr = S >> 2;                                                    // dwords per row
        for (int r = 0; r < S; r++) {
            uint32_t w = 0;
            for (int q = 0; q < dpr; q++) {
                const uint32_t x = ((m4[r * dpr + q] + 0x7F7F7F7Fu) & 0x80808080u) >> 7;     // bits 0, 8, 16, 24: cell != 0
                w |= ((x * 0x10204080u) >> 28) << (4 * q);                         // gathered into four adjacent bits
            }
            tile[r] = w;
        }
    } else {
        for (int r = 0; r < S; r++) {
            uint32_t w = 0;
            for (int c = 0; c < S; c++) w |= (mp[r * S + c] != 0 ? 1u : 0u) << c;
            tile[r] = w;
        }
    }
    for (int r = S; r < BS; r++) tile[r] = 0u;
    __syncthreads();
    // the chunk's image: 64 * BS words = 16 * BS pieces of 16 bytes; piece p = words [4 p, 4 p + 4) of env 4 p / BS (BS is a multiple of 4)
    const LDS_AS uint32_t* t0 = (const LDS_AS uint32_t*)(lds + a.off_ltile);
    GLOBAL_AS u32x4* g4 = (GLOBAL_AS u32x4*)(brd + env0 * BS);
    const uint32_t magicB = a.magicK;                                              // (this launch: ceil(2^32 / BS))
    for (int p = tid; p < 16 * BS; p += EPB) {
        const uint32_t wd = 4u * (uint32_t)p, e = __umulhi(wd, magicB), o = wd - e * (uint32_t)BS;
        const LDS_AS uint32_t* s = t0 + e * (uint32_t)(BS + 1) + o;
        g4[p] = u32x4{s[0], s[1], s[2], s[3]};
    }
}

// ---------------------------------------------------------------- LidarInFront from the bit rows, stand-alone launch
// The observation of the CURRENT state (what an explicit reset is followed by in the boards mode; the step kernel fuses the same rows).
template <int NR>
__global__ void __launch_bounds__(NGW_EPB) ngw_lidar_boards_kernel(const NgwLaunch a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    const int S = a.S, S2 = a.S2, K = a.K, BS = a.BS;
    const int64_t env0 = (int64_t)bid * EPB;
    const int nlive = (int)min((int64_t)EPB, a.n - env0);
    const bool live = (int)tid < nlive;
    const char* const bmap = reinterpret_cast<const char*>(a.b.map) + (uint64_t)bid * (uint32_t)(EPB * S2);
    const char* const binv = reinterpret_cast<const char*>(a.b.inv) + (uint64_t)bid * (uint32_t)(EPB * 4 * K);
    const char* const bbrd = reinterpret_cast<const char*>(a.b.brd) + (uint64_t)bid * (uint32_t)(EPB * 4 * BS);
    int r = 1, c = 1, f = 0;
    {
        const GLOBAL_AS int* lp = (const GLOBAL_AS int*)((const GLOBAL_AS char*)a.b.loc + (uint64_t)bid * (EPB * 8) + tid * 8u);
        const int pr = lp[0], pc = lp[1];
        const int ff = *(const GLOBAL_AS int*)((const GLOBAL_AS char*)a.b.facing + (uint64_t)bid * (EPB * 4) + tid * 4u);
        if (live) { r = pr; c = pc; f = ff; }                                  // (rows beyond n hold zeros: a pose inside the map keeps every read in bounds)
    }
    u32x4 bq[NR / 4];
#pragma unroll
    for (int j = 0; j < NR / 4; j++) bq[j] = *(const GLOBAL_AS u32x4*)((const GLOBAL_AS char*)bbrd + tid * 4u * (uint32_t)BS + 16u * (uint32_t)min(j, BS / 4 - 1));
    u32x4 q[IQ];
    const uint32_t rowoff = tid * 4u * (uint32_t)K;
#pragma unroll
    for (int j = 0; j < IQ; j++) q[j] = *(const GLOBAL_AS u32x4*)((const GLOBAL_AS char*)binv + rowoff + 4u * (uint32_t)min(4 * j, K - 4));
    const uint32_t lit = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[min(tid, (uint32_t)(LIDAR_ITEM_DW - 1))];
    const uint32_t id0 = reinterpret_cast<const uint32_t*>(a.lcfg->inv_item)[0], id1 = reinterpret_cast<const uint32_t*>(a.lcfg->inv_item)[1];
    lidar_zero_tile(a, lds, (int)tid);
    int32_t* inv = reinterpret_cast<int32_t*>(lds + a.off_inv) + tid * a.KP;
#pragma unroll
    for (int j = 0; j < IQ; j++) {
        const int o = min(4 * j, K - 4);
        inv[o] = (int)q[j].x; inv[o + 1] = (int)q[j].y; inv[o + 2] = (int)q[j].z; inv[o + 3] = (int)q[j].w;
    }
    lds[a.off_litem + min(tid, (uint32_t)(LIDAR_ITEM_DW - 1))] = lit;
    uint32_t R[NR];
    board_unpack<NR>(bq, R);
    const uint32_t roww = *(const GLOBAL_AS uint32_t*)((const GLOBAL_AS char*)bbrd + tid * 4u * (uint32_t)BS + 4u * (uint32_t)r) | 1u | (1u << (S - 1));
    uint32_t Rd[NR], Ra[NR];
    board_rotate<NR>(R, Rd, Ra);
    wave_lds_sync();
    lidar_boards_rows<NR>(a, lds, (int)tid, R, Rd, Ra, roww, BoardPatch{0u, 0u, 0u, 0u}, S, S2, r, c, f, bmap, tid * (uint32_t)S2, inv, id0, id1, bid);
}

}  // namespace
