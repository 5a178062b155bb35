// ngw_common.inc — what every compilation unit of the device code (ngw_unit_*.hip) and every kernel file (ngw_*.inc) starts from: the
// headers, the register / address-space / stamp macros, the staging of a wave's map and inventory rows between HBM and LDS, the stores
// into host memory, the launch helpers (ngw_launch.inc) and the functions the units call each other through.
//
// The kernels are CDNA4 (gfx950) kernels of the batched step()/reset() hot path.
// One 64-lane wavefront = one workgroup = 64 environments, ONE LANE PER ENV.  Per launch each wave
//   1. stages its 64 tile maps (64*S*S contiguous bytes) HBM -> LDS with coalesced 16-B loads, and the
//      per-env scalars / inventory rows into registers / LDS,
//   2. runs the table-driven step (and, for envs whose episode ended, the reset) per lane on LDS,
//   3. writes THROUGH to HBM only what the step changed - the broken / placed map cell, the touched inventory
//      slots, the agent pose - plus reward / done / packed info; a reset rewrites the wave's whole chunk with
//      coalesced 16-B stores.
// The observation buffers (map i8 [N,S,S], agent_location i32 [N,2], agent_facing_id i32 [N], inventory i32 [N,K])
// ARE the state and are updated in place, so a step reads S*S + 4*K + ~30 bytes per env and writes ~30
// (SURVEY.md §8(d) prices 2*S*S + 12*K + 45 for a read-pack-write design).  Integer/byte work only: no MFMA.
// Every global load of a phase is issued before its first consumer so a phase costs ONE memory round trip.
//
// Semantics follow the reference line by line (citations at each branch):
//   gym_novel_gridworlds/envs/pogostick_v1_env.py  reset :86-181, step :230-367, craft :413-474, grab :538-554
//   gym_novel_gridworlds/envs/bow_v1_env.py        Extract_string :293-304, craft :386-441
//   gym_novel_gridworlds/novelty_wrappers.py       AxeEasy :9-114, AxeMedium :117-213, AddItem :991-1034,
//                                                  AxetoBreak :439-625, AddChop :1267-1337, AddJump :1340-1412,
//                                                  BreakIncrease :1415-1488, ExtractIncDec :1491-1581
//   gym_novel_gridworlds/envs/pogostick_v0_env.py  tree_tap reset pass :156-178
//   gym_novel_gridworlds/observation_wrappers.py   LidarInFront :10-80 (ngw_lidar_kernel and the fused epilogue)
//
// The library's device code is one unit per ngw_unit_*.hip, compiled in parallel (Makefile); a unit holds the `extern "C"` launchers of
// its kernels and with them the kernel instantiations.  Every kernel file includes what it uses and keeps its contents in an unnamed
// namespace, so each unit has internal copies of what it shares with others and no two units clash.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ngw.h"
#include "ngw_device.h"
#include "ngw_launch.inc"

static_assert(NGW_MAX_PASSES == 4, "ResetArgs carries four pass words");
static_assert(sizeof(NgwDevSpec) % 4 == 0, "the spec blob is copied to LDS by dwords");

// The units call each other through these (feat: the NGW_FEAT_* bits, ngw_device.h); each is defined in the unit named after it
// (ngw_part_step: ngw_unit_step_straight.hip).
#define NGW_PART_FN(NAME) extern "C" hipError_t NAME(const NgwDevSpec* dspec, const NgwLaunch* a, int feat, unsigned grid, size_t lds_bytes, hipStream_t stream)
extern "C" hipError_t ngw_part_step(const NgwDevSpec* dspec, const NgwLaunch* a, int map_mode, int feat, unsigned grid, size_t lds_bytes, hipStream_t stream);
NGW_PART_FN(ngw_part_step_straight);
NGW_PART_FN(ngw_part_step_dword);
NGW_PART_FN(ngw_part_step_byte);
NGW_PART_FN(ngw_part_step_boards);
NGW_PART_FN(ngw_part_step_wire);
NGW_PART_FN(ngw_part_step_wire_boards);
NGW_PART_FN(ngw_part_step_mask_ns);
NGW_PART_FN(ngw_part_step_view);
NGW_PART_FN(ngw_part_rollout_straight);
NGW_PART_FN(ngw_part_rollout_dword);
NGW_PART_FN(ngw_part_rollout_byte);

namespace {

// Keep a value in a register across the step loop: the empty asm makes it opaque, so the compiler can neither
// re-load it from the kernarg segment / HBM with s_load inside the loop nor recompute it (worst case it parks it in
// a VGPR lane, one v_readlane to bring it back - no memory wait).
#define PIN_S(x) asm volatile("" : "+s"(x))
#define PIN_V(x) asm volatile("" : "+v"(x))
#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

constexpr int EPB = NGW_EPB;   // envs per block = wavefront width

// In-kernel timeline stamps (diagnostics build only: make stamps -> libngw_hip_stamps.so; tools/stamp_timeline.py).
// s_memrealtime = the chip-wide 100 MHz clock (aligns waves of different XCDs), s_memtime = shader cycles.
#ifdef NGW_STAMPS
#define STAMP_DECL uint64_t st_rt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_cy[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); st_rt[i] = __builtin_amdgcn_s_memrealtime(); st_cy[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_STRIDE 32        /* u64 per workgroup: [0, 8) chip clock, [8, 16) shader cycles of the kernel's stamps, [16, 32) shader cycles inside helpers (STAMP_SUB) */
#define STAMP_FLUSH(a) do { if ((a).stamps && threadIdx.x == 0) { for (int i_ = 0; i_ < 8; i_++) { (a).stamps[(size_t)blockIdx.x * STAMP_STRIDE + i_] = st_rt[i_]; (a).stamps[(size_t)blockIdx.x * STAMP_STRIDE + 8 + i_] = st_cy[i_]; } } } while (0)
#define STAMP_SUB(a, i) do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0xC07F) /* lgkmcnt(0): LDS work up to here is done */; const uint64_t c_ = __builtin_amdgcn_s_memtime(); if ((a).stamps && threadIdx.x == 0) (a).stamps[(size_t)blockIdx.x * STAMP_STRIDE + 16 + (i)] = c_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_SUBV(a, i) do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0) /* every counter: global loads have landed too */; const uint64_t c_ = __builtin_amdgcn_s_memtime(); if ((a).stamps && threadIdx.x == 0) (a).stamps[(size_t)blockIdx.x * STAMP_STRIDE + 16 + (i)] = c_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH(a)
#define STAMP_SUB(a, i)
#define STAMP_SUBV(a, i)
#endif

// ---------------------------------------------------------------- map staging HBM <-> LDS (coalesced 16-B pieces)
// The wave's 64 maps are one contiguous 64*S2-byte chunk in HBM = 4*S2 pieces of 16 B; lane l owns pieces
// l, l+64, ...  A round moves PB pieces per lane: ALL its global loads are issued before the first LDS write (and
// all LDS reads before the first global store), so a round costs one memory round trip, not PB.
// In LDS each env's map starts at e*MS bytes with MS/4 odd, so 64 lanes reading "their" cell hit distinct banks.
constexpr int PB = 8;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));                       // native vector: stays in VGPRs
typedef GLOBAL_AS u32x4 g_u32x4;
typedef GLOBAL_AS int2 g_int2;
typedef GLOBAL_AS int32_t g_i32;
typedef GLOBAL_AS uint32_t g_u32;
typedef GLOBAL_AS uint8_t g_u8;

// Loads are UNCONDITIONAL on a clamped index (a duplicate in-bounds load is harmless and keeps the values in plain
// registers); only stores and LDS writes are predicated.
__device__ __forceinline__ void pieces_load(u32x4 (&buf)[PB], const u32x4* g4, int base, int npieces, int tid) {
#pragma unroll
    for (int j = 0; j < PB; j++) buf[j] = g4[min(base + tid + EPB * j, npieces - 1)];
}

// LDS <-> register pieces.  TO_LDS: buf -> lds, else lds -> buf.
template <bool TO_LDS, int MAPMODE>
__device__ __forceinline__ void pieces_lds(u32x4 (&buf)[PB], const NgwLaunch& a, uint32_t* lds_map, int base, int npieces, int tid) {
    if (MAPMODE == NGW_MAP_STRAIGHT) {                                             // LDS image == HBM image
        u32x4* l4 = reinterpret_cast<u32x4*>(lds_map);
#pragma unroll
        for (int j = 0; j < PB; j++) {
            // (pieces_load clamps its addresses the same way: a slot beyond the chunk holds the LAST piece and stores it to the
            //  last piece's place again - no exec-mask bracket per piece)
            const int p = min(base + tid + EPB * j, npieces - 1);
            if (TO_LDS) l4[p] = buf[j]; else buf[j] = l4[p];
        }
    } else if (MAPMODE == NGW_MAP_DWORD) {                                         // dword granularity, padded stride
        const uint32_t S2dw = (uint32_t)a.S2 >> 2, MSdw = (uint32_t)a.MS >> 2;
#pragma unroll
        for (int j = 0; j < PB; j++) {
            const int p0 = base + tid + EPB * j;
            const int p = TO_LDS ? p0 : min(p0, npieces - 1);
            if (!TO_LDS || p0 < npieces) {
                const uint32_t d = (uint32_t)p * 4u;                               // dword offset inside the chunk
                uint32_t e = __umulhi(d, a.magic);                                 // d / S2dw (exact, see ngw_abi_create.cpp)
                uint32_t o = d - e * S2dw;
                uint32_t v[4] = {buf[j].x, buf[j].y, buf[j].z, buf[j].w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (o >= S2dw) { o = 0; e++; }
                    uint32_t* cell = lds_map + e * MSdw + o;
                    if (TO_LDS) *cell = v[q]; else v[q] = *cell;
                    o++;
                }
                if (!TO_LDS) buf[j] = u32x4{v[0], v[1], v[2], v[3]};
            }
        }
    } else {                                                                       // odd S: byte granularity
        uint8_t* lb = reinterpret_cast<uint8_t*>(lds_map);
#pragma unroll
        for (int j = 0; j < PB; j++) {
            const int p0 = base + tid + EPB * j;
            const int p = TO_LDS ? p0 : min(p0, npieces - 1);
            if (!TO_LDS || p0 < npieces) {
                const uint32_t g = (uint32_t)p * 16u;
                uint32_t e = __umulhi(g, a.magic);                                 // g / S2
                uint32_t o = g - e * (uint32_t)a.S2;
                uint32_t v[4] = {buf[j].x, buf[j].y, buf[j].z, buf[j].w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    uint32_t w = TO_LDS ? v[q] : 0u;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        if (o >= (uint32_t)a.S2) { o = 0; e++; }
                        uint8_t* cell = lb + e * (uint32_t)a.MS + o;
                        if (TO_LDS) *cell = (uint8_t)(w >> (8 * b)); else w |= (uint32_t)*cell << (8 * b);
                        o++;
                    }
                    v[q] = w;
                }
                if (!TO_LDS) buf[j] = u32x4{v[0], v[1], v[2], v[3]};
            }
        }
    }
}

// Inventory rows: the wave's 64 rows are one contiguous 64*K-dword chunk [e][K] = 16*K quads of 16 B; lane l owns
// quads l, l+64, ...  LDS layout [e][KP] with KP = K|1 (odd stride -> per-lane item reads are conflict-free).
constexpr int IQ = (NGW_MAX_ITEMS + 3) / 4;                                        // quads per lane, K <= 24

template <bool TO_LDS>
__device__ __forceinline__ void inv_lds(u32x4 (&q)[IQ], const NgwLaunch& a, int32_t* lds_inv, int tid) {
    const int nq = 16 * a.K;
    const int rounds = (nq + EPB - 1) / EPB;                                       // uniform: quads per lane actually used
    if (a.KP == a.K) {                                                             // K odd: LDS image == HBM image
        u32x4* l4 = reinterpret_cast<u32x4*>(lds_inv);
#pragma unroll
        for (int j = 0; j < IQ; j++) {
            if (j >= rounds) break;
            const int p = tid + EPB * j;
            if (TO_LDS) { if (p < nq) l4[p] = q[j]; } else q[j] = l4[min(p, nq - 1)];
        }
    } else {                                                                       // K even: one pad dword per env
#pragma unroll
        for (int j = 0; j < IQ; j++) {
            if (j >= rounds) break;
            const int p0 = tid + EPB * j;
            const int p = TO_LDS ? p0 : min(p0, nq - 1);
            if (!TO_LDS || p0 < nq) {
                const uint32_t d = (uint32_t)p * 4u;
                uint32_t e = __umulhi(d, a.magicK);                                // d / K
                uint32_t o = d - e * (uint32_t)a.K;
                uint32_t v[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (o >= (uint32_t)a.K) { o = 0; e++; }
                    int32_t* cell = lds_inv + e * (uint32_t)a.KP + o;
                    if (TO_LDS) *cell = (int32_t)v[i]; else v[i] = (uint32_t)*cell;
                    o++;
                }
                if (!TO_LDS) q[j] = u32x4{v[0], v[1], v[2], v[3]};
            }
        }
    }
}

// a store into the HOST's memory (the write-through targets, NgwWT): system scope - written through every cache level at once (global_store ... sc0 sc1),
// so that "the wave's stores are acknowledged" (s_waitcnt) means "the host can see them".  A plain store may sit dirty in this XCD's L2 until the
// kernel ends: wire_done's counter would then announce data that has not left the chip (seen with 2 MB of observation rows per launch).
template <class T> __device__ __forceinline__ void stgs(void* base, uint32_t off, T v) {
    __hip_atomic_store((GLOBAL_AS T*)((GLOBAL_AS char*)base + off), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ... 16 bytes of it (no 128-bit atomic store in the language: the instruction with the same cache bits)
__device__ __forceinline__ void stgs16(void* base, uint32_t off, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2 sc0 sc1" : : "v"(off), "v"(v), "s"(base) : "memory");
}

}  // namespace
