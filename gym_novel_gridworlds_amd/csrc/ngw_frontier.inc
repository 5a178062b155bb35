// ngw_frontier.inc - device-side frontiers: flags compacted into an index list of fixed capacity, and slots handed out for it (a unit of its own;
// host side: ngw_abi_frontier.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// A search turns a `fresh` / `where` / `length` tensor into the index lists of its next call.  The number of hits is known on the device only, so
// the list has a fixed CAPACITY and is padded with NGW_IDX_NONE, the pair that is not there, which every kernel that gathers by an index list skips.
// The contract is include/ngw.h's (ngw_frontier_compact, ngw_frontier_alloc); frontier.compact_reference states it in numpy.
//
// Compaction, two launches (count, scatter) over tiles of NGW_FRONTIER_TILE = 4096 flag bytes, one work-group of four waves per tile:
//   1. Lane l of the tile loads its 16 bytes in one piece (a flag array that does not start on 16 bytes, and a tile's ragged end, go byte by byte)
//      and folds them into a 16-bit mask: bit i = byte 16 * l + i is not zero - ANY non-zero byte counts.  Its count is a popcount.
//   2. Count launch: the counts are summed over the wave and the four waves (integer adds in a fixed order), tiles[b] = the tile's hits.
//   3. Scatter launch: every work-group sums tiles[0 .. b) and tiles[0 .. T) itself - at most 4096 dwords, 16 per lane, L2 hits - so no work-group
//      waits for another and no atomic orders the output: rank = hits in the tiles before + hits in the waves before (four words through LDS) + hits
//      in the lanes before (the five bits of the lane's count, each a ballot whose lower lanes v_mbcnt counts) + the set bits below in the lane's
//      own mask.  Position p with rank k < capacity stores first[k] = map[p / div] (or p / div) and second[k] = p % div: ascending and
//      deterministic, the row-major order fresh_pairs promises.
//   4. The tail [min(total, capacity), capacity) is filled with NGW_IDX_NONE by all work-groups in a grid stride; the first one stores count[0 .. 2)
//      and raises NGW_F_FRONTIER_FULL where total > capacity.
// No float, no host wait.  A position is never computed for a byte past n, and never stored at a rank past capacity.

constexpr int FR_BLOCK = NGW_FRONTIER_BLOCK, FR_WAVES = NGW_FRONTIER_BLOCK / NGW_EPB;
static_assert(NGW_EPB == 64 && FR_WAVES * NGW_EPB == FR_BLOCK && NGW_FRONTIER_TILE == 16 * FR_BLOCK, "four waves, 16 flag bytes per lane");

// bit i: byte p0 + i of the flags is not zero (a byte at or past n: 0)
template <bool VEC16>
__device__ __forceinline__ uint32_t frontier_lane_mask(const uint8_t* bytes, int64_t p0, int64_t n) {
    uint32_t m = 0;
    if (VEC16 && p0 + 16 <= n) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(bytes + p0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) m |= ((w[j] >> (8 * i)) & 255u) ? 1u << (4 * j + i) : 0u;
    } else {
        for (int i = 0; i < 16; i++)
            if (p0 + i < n && bytes[p0 + i]) m |= 1u << i;
    }
    return m;
}

// the sum of cnt (at most 16: five bits) over the lanes below this one, and over the wave: a ballot and an mbcnt per bit
__device__ __forceinline__ uint32_t frontier_wave_prefix(uint32_t cnt, uint32_t& total) {
    uint32_t pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const uint64_t b = __ballot((cnt >> k) & 1u);
        pre += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)) << k;
        total += (uint32_t)__popcll(b) << k;
    }
    return pre;
}

// the sum of v over the work-group, in every thread (part: FR_WAVES words of LDS; every thread calls it)
__device__ __forceinline__ int frontier_block_sum(int v, int* part) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & (EPB - 1)) == 0) part[threadIdx.x / EPB] = v;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < FR_WAVES; w++) r += part[w];
    __syncthreads();                                                               // (before `part` is written again)
    return r;
}

template <bool VEC16>
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_frontier_count_kernel(const NgwFrontier x) {
    __shared__ int part[FR_WAVES];
    const int64_t p0 = (int64_t)blockIdx.x * NGW_FRONTIER_TILE + (int64_t)threadIdx.x * 16;
    const uint32_t m = frontier_lane_mask<VEC16>(x.bytes, p0, x.n);
    const int hits = frontier_block_sum(__popc(m), part);
    if (threadIdx.x == 0) x.tiles[blockIdx.x] = hits;
}

// grid: at least n_tiles work-groups (those behind them only fill the tail), at least one
template <bool VEC16>
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_frontier_scatter_kernel(const NgwFrontier x) {
    __shared__ int part[FR_WAVES];
    const int b = (int)blockIdx.x, T = x.n_tiles, tid = (int)threadIdx.x;
    int before = 0, all = 0;
    for (int i = tid; i < T; i += FR_BLOCK) {
        const int c = x.tiles[i];
        all += c;
        if (i < b) before += c;
    }
    before = frontier_block_sum(before, part);
    all = frontier_block_sum(all, part);
    const int64_t cap = x.capacity;
    if (b < T) {                                                                   // (uniform: the barrier below is reached by the whole work-group)
        const int64_t p0 = (int64_t)b * NGW_FRONTIER_TILE + (int64_t)tid * 16;
        const uint32_t m = frontier_lane_mask<VEC16>(x.bytes, p0, x.n);
        uint32_t wave_hits;
        const uint32_t pre = frontier_wave_prefix((uint32_t)__popc(m), wave_hits);
        const int wave = tid / EPB;
        if ((tid & (EPB - 1)) == 0) part[wave] = (int)wave_hits;
        __syncthreads();
        int64_t k = (int64_t)before + (int64_t)pre;
        for (int w = 0; w < wave; w++) k += part[w];
        const int div = x.div;
        for (uint32_t bits = m; bits; bits &= bits - 1, k++) {
            if (k >= cap) break;                                                   // (the ranks only grow: nothing of this lane fits any more)
            const int32_t p = (int32_t)(p0 + __builtin_ctz(bits));                 // (p < n <= 2^24)
            const int32_t q = div == 1 ? p : p / div;
            x.first[k] = x.map ? x.map[q] : q;
            if (x.second) x.second[k] = p - q * div;
        }
    }
    const int64_t taken = min((int64_t)all, cap);
    for (int64_t k = taken + (int64_t)b * FR_BLOCK + tid; k < cap; k += (int64_t)gridDim.x * FR_BLOCK) {
        x.first[k] = NGW_IDX_NONE;
        if (x.second) x.second[k] = NGW_IDX_NONE;
    }
    if (b == 0 && tid == 0) {
        x.count[0] = (int32_t)taken;
        x.count[1] = all;
        if ((int64_t)all > cap) atomicOr(x.flags, NGW_F_FRONTIER_FULL);
    }
}

// Slot allocation, one launch.  Every thread reads the cursor and count[0] first; a work-group takes a ticket once all its threads have (the
// barrier), and the one that takes the last ticket - every work-group has read the cursor by then - stores the new cursor and puts the ticket back
// to 0 for the next call.  The slots are plain vector stores in a grid stride.
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_frontier_alloc_kernel(const NgwFrontierAlloc x) {
    const int32_t c = __hip_atomic_load(x.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t want = x.count[0];
    const int64_t m = max(min((int64_t)want, (int64_t)x.limit - (int64_t)c), (int64_t)0);
    for (int64_t k = (int64_t)blockIdx.x * FR_BLOCK + threadIdx.x; k < x.capacity; k += (int64_t)gridDim.x * FR_BLOCK)
        x.slots[k] = k < m ? (int32_t)((int64_t)c + k) : NGW_IDX_NONE;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t ticket = __hip_atomic_fetch_add(x.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == gridDim.x - 1u) {
            __hip_atomic_store(x.cursor, (int32_t)((int64_t)c + m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(x.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m < (int64_t)want) atomicOr(x.flags, NGW_F_FRONTIER_FULL);
        }
    }
}

}  // namespace
