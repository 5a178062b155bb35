// ngw_snapshot.inc - device-side snapshots: rows of the seven state arrays moved between the state slab and a snapshot buffer, in either
// direction, through index lists (NgwSnap in ngw_device.h; a unit of its own; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// A row is small and oddly sized (S*S map bytes + 4*K inventory bytes + 21 bytes of scalars: 188 B at 10 x 10 with K = 17), so one lane
// per env would issue 25 dword loads whose 64 addresses lie 100 B apart - most of every memory transaction unused.  Instead
// NGW_SNAP_GROUP = 16 lanes share one row: consecutive lanes move consecutive pieces of the row's map (16 B pieces where S*S is a multiple
// of 16, dwords where it is a multiple of 4), then the inventory dwords, and five lanes move one scalar each.  A wave handles four rows, a
// 256-thread workgroup sixteen.  Row indices are checked against the row counts of both sets: a bad one skips that row's copy and raises
// the sticky NGW_F_BAD_INDEX (one atomic OR per bad row), nothing is ever addressed with it.
//
// Odd map sizes (S*S % 4 != 0: 81 B at 9 x 9): rows start at any byte, and the source and destination row need not be aligned alike.
// When they are (always in the contiguous case, one permuted row in four otherwise) the group moves a byte head up to the next dword
// boundary, aligned dwords, and a byte tail; otherwise bytes all the way.
//
// Rows of one call never overlap (the host side's contract: distinct destination rows).  Source and destination are different allocations, or -
// a slot-to-slot copy inside one snapshot (ngw_snapshot_copy) - rows of one allocation of which no destination is also a source: the kernel
// addresses whole rows of either set by index and assumes nothing about which set is the state slab.

template <typename T>
__device__ __forceinline__ void snap_copy(void* dst, const void* src, int n, int g) {
    T* __restrict__ d = static_cast<T*>(dst);
    const T* __restrict__ s = static_cast<const T*>(src);
    for (int p = g; p < n; p += NGW_SNAP_GROUP) d[p] = s[p];
}

// VEC = bytes per map piece: 16 / 4 (S2 a multiple of it: every row of both sets is that aligned), 1 = odd S2
template <int VEC>
__global__ void __launch_bounds__(NGW_SNAP_BLOCK) ngw_snapshot_kernel(const NgwSnap a) {
    const int j = (int)(blockIdx.x * (NGW_SNAP_BLOCK / NGW_SNAP_GROUP) + threadIdx.x / NGW_SNAP_GROUP);
    const int g = (int)(threadIdx.x % NGW_SNAP_GROUP);
    if (j >= a.count) return;
    const int si = a.si ? a.si[j] : j, di = a.di ? a.di[j] : j;
    if ((uint32_t)si >= (uint32_t)a.src_rows || (uint32_t)di >= (uint32_t)a.dst_rows) {
        if (g == 0 && si != NGW_IDX_NONE && di != NGW_IDX_NONE) atomicOr(a.flags, NGW_F_BAD_INDEX);   // (NGW_IDX_NONE: a pair that is not there)
        return;
    }
    const int S2 = a.S2, K = a.K;
    const int8_t* ms = a.src.map + (size_t)si * (size_t)S2;
    int8_t* md = a.dst.map + (size_t)di * (size_t)S2;
    if (VEC == 16) {
        snap_copy<uint4>(md, ms, S2 >> 4, g);
    } else if (VEC == 4) {
        snap_copy<uint32_t>(md, ms, S2 >> 2, g);
    } else {
        const uint32_t sa = (uint32_t)(uintptr_t)ms & 3u, da = (uint32_t)(uintptr_t)md & 3u;
        if (sa == da) {
            const int head = min((int)((4u - sa) & 3u), S2), body = (S2 - head) >> 2, tail = S2 - head - 4 * body;
            if (g < head) md[g] = ms[g];
            snap_copy<uint32_t>(md + head, ms + head, body, g);
            if (g < tail) md[head + 4 * body + g] = ms[head + 4 * body + g];
        } else {
            snap_copy<int8_t>(md, ms, S2, g);
        }
    }
    snap_copy<int32_t>(a.dst.inv + (size_t)di * (size_t)K, a.src.inv + (size_t)si * (size_t)K, K, g);
    // the scalars, one lane each (the group's LAST lanes: at K <= 11 they are not the ones that moved an inventory dword)
    if (g == NGW_SNAP_GROUP - 1) reinterpret_cast<int2*>(a.dst.loc)[di] = reinterpret_cast<const int2*>(a.src.loc)[si];
    if (g == NGW_SNAP_GROUP - 2) a.dst.facing[di] = a.src.facing[si];
    if (g == NGW_SNAP_GROUP - 3) a.dst.step_count[di] = a.src.step_count[si];
    if (g == NGW_SNAP_GROUP - 4 && !a.keep_episode) a.dst.episode[di] = a.src.episode[si];
    if (g == NGW_SNAP_GROUP - 5) a.dst.selected[di] = a.src.selected[si];
}

}  // namespace
