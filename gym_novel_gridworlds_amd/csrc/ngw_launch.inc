// ngw_launch.inc — how every kernel of the library is launched, and how a runtime flag picks a kernel instantiation (host code; part of
// ngw_common.inc).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "ngw_device.h"

namespace {

// The one launch: the opt-in to more than the default 64 KiB of dynamic LDS (CDNA4 has 160 KiB per CU), then the kernel, in the <<< >>> form
// (the arguments are converted to the kernel's parameter types in its own order).  The opt-in is per kernel and device and is repeated only
// when a request exceeds what this instantiation was last opted in to on the current device; two host threads that race on an entry make
// one redundant hipFuncSetAttribute call at worst.  A device index beyond the table opts in every time.
constexpr size_t LDS_DEFAULT_MAX = 64 * 1024;
constexpr int LDS_OPT_IN_DEVICES = 64;

template <auto Kernel, class... Args>
hipError_t launch_kernel(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
    if (lds_bytes > LDS_DEFAULT_MAX) {
        static std::atomic<size_t> opted_in[LDS_OPT_IN_DEVICES] = {};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::atomic<size_t>* const seen = dev >= 0 && dev < LDS_OPT_IN_DEVICES ? &opted_in[dev] : nullptr;
        if (!seen || lds_bytes > seen->load(std::memory_order_relaxed)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return e;
            if (seen) seen->store(lds_bytes, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
    return hipGetLastError();
}

// A runtime flag as a template argument: f is a generic lambda and receives the value as a std::integral_constant (`decltype(x)::value` is
// a constant expression inside it).  A nest of these instantiates EVERY combination it can reach, so a launcher dispatches only over the
// flags that are free where it stands and keeps the combinations that have no kernel as early returns or fixed arguments.
template <class F>
hipError_t with_flag(bool v, F&& f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}

// the map addressing mode (NGW_MAP_*: how a wave's map chunk lies in LDS)
template <class F>
hipError_t with_map_mode(int map_mode, F&& f) {
    switch (map_mode) {
    case NGW_MAP_STRAIGHT: return f(std::integral_constant<int, NGW_MAP_STRAIGHT>{});
    case NGW_MAP_DWORD: return f(std::integral_constant<int, NGW_MAP_DWORD>{});
    default: return f(std::integral_constant<int, NGW_MAP_BYTE>{});
    }
}

// the register rows NR of the bit-row lidar (ngw_boards.inc) that hold BS = NGW_BOARD_STRIDE(S) words per env
template <class F>
hipError_t with_board_rows(int BS, F&& f) {
    if (BS < 4 || BS > 32) return hipErrorInvalidValue;
    if (BS <= 12) return f(std::integral_constant<int, 12>{});
    if (BS <= 20) return f(std::integral_constant<int, 20>{});
    return f(std::integral_constant<int, 32>{});
}

// the bytes per map piece of the kernels that move single rows by index (ngw_expand.inc's expand_move_row: snapshot expand and snapshot
// rollout; ngw_keys.inc's row reads): 16 / 4 where S*S is a multiple of it - every row of every set is then that aligned -, 1 = odd S*S
template <class F>
hipError_t with_row_piece(int S2, F&& f) {
    if (S2 % 16 == 0) return f(std::integral_constant<int, 16>{});
    if (S2 % 4 == 0) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 1>{});
}

// the work-groups of a kernel that gives each of `count` items one lane: whole waves of NGW_EPB
constexpr int64_t blocks_for(int64_t count) { return (count + NGW_EPB - 1) / NGW_EPB; }

}  // namespace
