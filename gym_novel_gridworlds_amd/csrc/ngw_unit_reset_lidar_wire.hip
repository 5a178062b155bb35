// ngw_unit_reset_lidar_wire.hip — the small kernels around the step: the dedicated new-episode kernel (ngw_reset.inc), the stand-alone
// LidarInFront kernel, the one-env resident loop (ngw_solo.inc), and the diff / wire / pack / agent-view kernels of the host step.
#include "ngw_common.inc"
#include "ngw_lidar_march.inc"     // lidar_epilogue
#include "ngw_solo.inc"
#include "ngw_reset.inc"

namespace {

// ---------------------------------------------------------------- LidarInFront observation kernel (stand-alone launch)
// observation_wrappers.py:32-80 of the CURRENT state.  Same wave = 64 envs decomposition and the same coalesced staging of the
// maps and inventory rows as the other kernels, then the shared row builder (lidar_epilogue).  `a` carries the launch's own LDS
// layout (ngw_lidar_configure: off_litem, off_ltab, off_ltile, off_map, off_inv).
template <int MAPMODE>
__global__ void __launch_bounds__(NGW_EPB) ngw_lidar_kernel(const NgwLaunch a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    const int64_t env0 = (int64_t)blockIdx.x * EPB;
    const int64_t e = env0 + tid;
    const bool live = e < a.n;
    const int S = a.S, K = a.K, npieces = 4 * a.S2;
    uint32_t* lds_map = lds + a.off_map;
    int32_t* lds_inv = reinterpret_cast<int32_t*>(lds + a.off_inv);
    uint32_t it = 0;
    if (tid < LIDAR_ITEM_DW) it = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[tid];
    u32x4 buf[PB];
    const u32x4* gin = reinterpret_cast<const u32x4*>(a.b.map + env0 * a.S2);
    pieces_load(buf, gin, 0, npieces, tid);
    int r = 1, c = 1, f = 0;
    if (live) {
        const int2 rc = reinterpret_cast<const int2*>(a.b.loc)[e];
        r = rc.x; c = rc.y;
        f = a.b.facing[e];
    }
    u32x4 iq[IQ];
    {
        const u32x4* gi = reinterpret_cast<const u32x4*>(a.b.inv + env0 * K);
#pragma unroll
        for (int j = 0; j < IQ; j++) iq[j] = (j * EPB < 16 * K) ? gi[min(tid + EPB * j, 16 * K - 1)] : u32x4{0u, 0u, 0u, 0u};
    }
    if (tid < LIDAR_ITEM_DW) lds[a.off_litem + tid] = it;
    pieces_lds<true, MAPMODE>(buf, a, lds_map, 0, npieces, tid);
    for (int base = EPB * PB; base < npieces; base += EPB * PB) {
        pieces_load(buf, gin, base, npieces, tid);
        pieces_lds<true, MAPMODE>(buf, a, lds_map, base, npieces, tid);
    }
    inv_lds<true>(iq, a, lds_inv, tid);
    const int8_t* mp = reinterpret_cast<const int8_t*>(lds_map) + tid * a.MS;
    lidar_epilogue(a, lds, tid, live, mp + r * S + c, f, lds_inv + tid * a.KP);     // (its first barrier makes the staging visible)
}

// Delta refresh of a host mirror (NgwDiff, ngw_step_host): region blockIdx.y is compared, 16 bytes at a time, with the shadow
// copy of what the host holds; only pieces that differ are stored - to the shadow, and straight into the host's page-locked
// mirror across PCIe (mapped memory).  A step changes a few bytes of an env's map / inventory, so this moves ~1 % of what a
// full copy moves.  Regions are 16-byte aligned on all three sides; a tail shorter than 16 bytes goes by bytes.
__global__ __launch_bounds__(256) void ngw_diff_kernel(const NgwDiff p) {
    const int r = blockIdx.y;
    const uint64_t nb = p.nbytes[r];
    const uint8_t* c = p.cur[r];
    uint8_t* s = p.shadow[r];
    uint8_t* h = p.host[r];
    const uint64_t stride = (uint64_t)gridDim.x * 256u, t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t n16 = nb >> 4;
    for (uint64_t i = t; i < n16; i += stride) {
        const u32x4 a = reinterpret_cast<const u32x4*>(c)[i], b = reinterpret_cast<const u32x4*>(s)[i];
        if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) {
            reinterpret_cast<u32x4*>(s)[i] = a;
            reinterpret_cast<u32x4*>(h)[i] = a;
        }
    }
    for (uint64_t i = (n16 << 4) + t; i < nb; i += stride)
        if (c[i] != s[i]) { s[i] = c[i]; h[i] = c[i]; }
}

// Narrow wire format of the host step (NgwWire, ngw_step_host_packed): one lane per env narrows pose / reward / done / info into
// four dense arrays of a staging payload (reads 22 B, writes 13 B per env; coalesced both ways).
__global__ __launch_bounds__(256) void ngw_wire_kernel(const NgwWire p) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) *p.flags_out = *p.flags;
    if (e >= p.n) return;
    const int r = p.loc[2 * e], c = p.loc[2 * e + 1], f = p.facing[e];
    const uint32_t sel = p.selected[e];
    p.pose[e] = (uint32_t)(r & 255) | ((uint32_t)(c & 255) << 8) | ((uint32_t)(f & 255) << 16) | (sel << 24);
    p.reward32[e] = p.reward[e];
    p.done8[e] = p.done[e];
    p.info32[e] = p.info[e];
}

// Delta refresh and narrowing in ONE launch (ngw_step_host_packed's steady state: the block is a mirror and takes direct stores): slices
// y < n_regions are ngw_diff_kernel's regions, the last slice narrows pose / reward / done / info with a grid-stride loop over the envs.
__global__ __launch_bounds__(256) void ngw_diff_wire_kernel(const NgwDiff p, const NgwWire w) {
    const int r = blockIdx.y;
    const uint64_t stride = (uint64_t)gridDim.x * 256u, t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r == p.n_regions) {
        if (t == 0) *w.flags_out = *w.flags;
        for (uint64_t e = t; e < (uint64_t)w.n; e += stride) {
            const int rr = w.loc[2 * e], c = w.loc[2 * e + 1], f = w.facing[e];
            const uint32_t sel = w.selected[e];
            w.pose[e] = (uint32_t)(rr & 255) | ((uint32_t)(c & 255) << 8) | ((uint32_t)(f & 255) << 16) | (sel << 24);
            w.reward32[e] = w.reward[e];
            w.done8[e] = w.done[e];
            w.info32[e] = w.info[e];
        }
        return;
    }
    const uint64_t nb = p.nbytes[r];
    const uint8_t* c = p.cur[r];
    uint8_t* s = p.shadow[r];
    uint8_t* h = p.host[r];
    const uint64_t n16 = nb >> 4;
    for (uint64_t i = t; i < n16; i += stride) {
        const u32x4 a = reinterpret_cast<const u32x4*>(c)[i], b = reinterpret_cast<const u32x4*>(s)[i];
        if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) {
            reinterpret_cast<u32x4*>(s)[i] = a;
            reinterpret_cast<u32x4*>(h)[i] = a;
        }
    }
    for (uint64_t i = (n16 << 4) + t; i < nb; i += stride)
        if (c[i] != s[i]) { s[i] = c[i]; h[i] = c[i]; }
}

// Region copies (NgwPack): region blockIdx.y, grid-stride over 16-byte pieces; tails and unaligned regions go by bytes.
// The destination may be host memory mapped into the GPU's address space (the stores then travel over PCIe).
__global__ __launch_bounds__(256) void ngw_pack_kernel(const NgwPack p) {
    const int r = blockIdx.y;
    const uint64_t nb = p.nbytes[r];
    const uint8_t* s = p.src[r];
    uint8_t* d = p.dst[r];
    const uint64_t stride = (uint64_t)gridDim.x * 256u, t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if ((((uintptr_t)s | (uintptr_t)d) & 15u) == 0) {
        const uint64_t n16 = nb >> 4;
        for (uint64_t i = t; i < n16; i += stride) reinterpret_cast<u32x4*>(d)[i] = reinterpret_cast<const u32x4*>(s)[i];
        for (uint64_t i = (n16 << 4) + t; i < nb; i += stride) d[i] = s[i];
    } else {
        for (uint64_t i = t; i < nb; i += stride) d[i] = s[i];
    }
}

// AgentMap (reference observation_wrappers.py:104-121): the (2V+1) x (2V+1) window of the map centred on the agent, 0 outside
// the map.  HBM-bound byte gather: one lane produces 4 consecutive output bytes (one coalesced dword store); the map reads
// hit each env's 100-B row image, which one wave covers with a handful of cache lines.
__global__ __launch_bounds__(256) void ngw_agent_view_kernel(const int8_t* __restrict__ map, const int32_t* __restrict__ loc,
                                                             uint32_t* __restrict__ out, uint32_t n_dwords, int S, int V,
                                                             uint32_t magicW) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_dwords) return;
    const uint32_t W = 2u * (uint32_t)V + 1u, WW = W * W;
    uint32_t idx = t * 4u;
    uint32_t e = idx / WW;                           // one full division per lane; the rest are small-operand magics
    uint32_t rem = idx - e * WW;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t r = __umulhi(rem, magicW), c = rem - r * W;
        const int mr = loc[2 * (size_t)e] + (int)r - V, mc = loc[2 * (size_t)e + 1] + (int)c - V;
        uint32_t v = 0;
        if ((unsigned)mr < (unsigned)S && (unsigned)mc < (unsigned)S) v = (uint8_t)map[(size_t)e * (S * S) + mr * S + mc];
        word |= v << (8 * j);
        if (++rem == WW) { rem = 0; ++e; }
    }
    out[t] = word;
}

}  // namespace

extern "C" hipError_t ngw_pack_launch(const NgwPack* p, hipStream_t stream) {
    if (p->n_regions < 1) return hipSuccess;
    uint64_t most = 0;
    for (int r = 0; r < p->n_regions; r++) most = p->nbytes[r] > most ? p->nbytes[r] : most;
    uint64_t blocks = (most / 16u + 255u) / 256u;                          // one 16-byte piece per thread, up to 2048 blocks per region
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    return launch_kernel<ngw_pack_kernel>(dim3((unsigned)blocks, (unsigned)p->n_regions), dim3(256), 0, stream, *p);
}

extern "C" hipError_t ngw_wire_launch(const NgwWire* p, hipStream_t stream) {
    return launch_kernel<ngw_wire_kernel>(dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, stream, *p);
}

extern "C" hipError_t ngw_diff_launch(const NgwDiff* p, hipStream_t stream) {
    if (p->n_regions < 1) return hipSuccess;
    uint64_t most = 0;
    for (int r = 0; r < p->n_regions; r++) most = p->nbytes[r] > most ? p->nbytes[r] : most;
    uint64_t blocks = (most / 16u + 255u) / 256u;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    return launch_kernel<ngw_diff_kernel>(dim3((unsigned)blocks, (unsigned)p->n_regions), dim3(256), 0, stream, *p);
}

extern "C" hipError_t ngw_diff_wire_launch(const NgwDiff* p, const NgwWire* w, hipStream_t stream) {
    uint64_t most = ((uint64_t)w->n + 15u) / 16u * 16u;                            // (the narrowing slice: one env per lane and round)
    for (int r = 0; r < p->n_regions; r++) most = p->nbytes[r] > most ? p->nbytes[r] : most;
    uint64_t blocks = (most / 16u + 255u) / 256u;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    return launch_kernel<ngw_diff_wire_kernel>(dim3((unsigned)blocks, (unsigned)p->n_regions + 1u), dim3(256), 0, stream, *p, *w);
}

extern "C" hipError_t ngw_agent_view_launch(const int8_t* map, const int32_t* loc, uint32_t* out, uint32_t n_dwords, int S, int V,
                                            hipStream_t stream) {
    const uint32_t W = 2u * (uint32_t)V + 1u;
    const uint32_t magicW = (uint32_t)((0x100000000ull + W - 1) / W);     // exact for operands < W * W
    return launch_kernel<ngw_agent_view_kernel>(dim3((n_dwords + 255u) / 256u), dim3(256), 0, stream, map, loc, out, n_dwords, S, V, magicW);
}

extern "C" hipError_t ngw_lidar_launch(const NgwLaunch* a, int map_mode, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    return with_map_mode(map_mode, [&](auto MM) { return launch_kernel<ngw_lidar_kernel<decltype(MM)::value>>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, *a); });
}

extern "C" hipError_t ngw_solo_launch(const NgwDevSpec* dspec, const NgwSolo* p, int ext, size_t lds_bytes, hipStream_t stream) {
    return with_flag(ext != 0, [&](auto E) { return launch_kernel<ngw_solo_kernel<decltype(E)::value>>(dim3(1), dim3(NGW_EPB), lds_bytes, stream, dspec, *p); });
}

// the dedicated new-episode kernel: nw = mask words in registers (2 / 8, 0 = LDS), subset = one subset pass
extern "C" hipError_t ngw_reset_fast_launch(const NgwDevSpec* dspec, const NgwResetFast* a, int nw, int subset, unsigned grid, size_t lds_bytes,
                                            hipStream_t stream) {
    auto go = [&](auto NW) {
        return with_flag(subset != 0, [&](auto SUB) {
            return launch_kernel<ngw_reset_fast<decltype(NW)::value, decltype(SUB)::value>>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, dspec, *a);
        });
    };
    switch (nw) {
    case 0: return go(std::integral_constant<int, 0>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 8: return go(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
    }
}
