// fake_hip.cpp - the fake HIP runtime of the host-side sanitizer harness (see hip/hip_runtime.h).  What it guarantees:
//   * hipMalloc / hipHostMalloc are malloc() of EXACTLY the requested size, so AddressSanitizer's redzone starts at the first byte past it;
//     hipFree / hipHostFree are free(), so a pointer kept across a regrow is a use-after-free report.  hipHostGetDevicePointer answers with the
//     same address, and only for memory that hipHostMalloc handed out (the real runtime refuses pageable memory too).
//   * copies and fills do the real byte operation at once, through memcpy / memset, so both ends of every copy are bounds-checked.
//   * streams, events, graphs and graph-execs are small heap objects; capture and replay are bookkeeping (a launch made while a capture is open has
//     already run its stub); every synchronisation returns success.
//   * a ledger counts what is alive: fake_hip_live() / fake_hip_report().
// -DFAKE_HIP_SHORT=<bytes>: the harness's self-test.  Allocations are handed out that many bytes short (every one, or the one
// fake_hip_short_only() picks).  The zero-fill of exactly the requested size at the allocation's base - what ngwh::dev_alloc does right behind
// hipMalloc, and the memset behind ngw_host_alloc - is clamped to what was handed out, so that the report comes from the code that USES the
// allocation (a launch stub, a later copy), which is what the self-test asks about.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#ifndef FAKE_HIP_SHORT
#define FAKE_HIP_SHORT 0
#endif

struct fakeStream { int capturing; };
struct fakeEvent { int recorded; };
struct fakeGraph { int nodes; };
struct fakeGraphExec { int launches; };

namespace {

struct Alloc { size_t asked, given; };
std::map<void*, Alloc> g_dev, g_host;
long long g_streams, g_events, g_graphs, g_execs;
int g_short_countdown = -1;                       // -1: every allocation is short; >= 0: only the one that many calls ahead
bool g_short_picked = false;

size_t handed_out(size_t bytes) {
    if (!FAKE_HIP_SHORT) return bytes;
    bool cut = !g_short_picked;
    if (g_short_picked && g_short_countdown >= 0) cut = g_short_countdown-- == 0;
    if (!cut) return bytes;
    if (g_short_picked) fprintf(stderr, "fake_hip: the picked allocation: %zu bytes asked, %d fewer handed out\n", bytes, FAKE_HIP_SHORT);
    return bytes > (size_t)FAKE_HIP_SHORT ? bytes - (size_t)FAKE_HIP_SHORT : 0;
}

hipError_t alloc_into(std::map<void*, Alloc>& book, void** p, size_t bytes) {
    if (!p) return hipErrorInvalidValue;
    const size_t given = handed_out(bytes);
    void* q = malloc(given ? given : 1);
    if (!q) return hipErrorOutOfMemory;
    if (!given) { free(q); q = malloc(1); }       // (a one-byte block stands for the empty one: still a unique address)
    book[q] = Alloc{bytes, given};
    *p = q;
    return hipSuccess;
}

hipError_t free_from(std::map<void*, Alloc>& book, void* p, const char* what) {
    if (!p) return hipSuccess;
    auto it = book.find(p);
    if (it == book.end()) {
        fprintf(stderr, "fake_hip: %s(%p): not a live allocation of this kind (double free, or the wrong free)\n", what, p);
        abort();
    }
    book.erase(it);
    free(p);
    return hipSuccess;
}

// FAKE_HIP_SHORT: the fill of a whole fresh allocation (see the head of this file)
size_t clamp_whole_fill(void* dst, size_t bytes) {
    if (!FAKE_HIP_SHORT) return bytes;
    for (auto* book : {&g_dev, &g_host}) {
        auto it = book->find(dst);
        if (it != book->end() && it->second.asked == bytes) return it->second.given;
    }
    return bytes;
}

}  // namespace

extern "C" {

const char* hipGetErrorString(hipError_t e) {
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidResourceHandle: return "invalid resource handle";
    default: return "unknown error";
    }
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDeviceCount(int* count) { if (!count) return hipErrorInvalidValue; *count = 1; return hipSuccess; }
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidValue; }

hipError_t hipMalloc(void** p, size_t bytes) { return alloc_into(g_dev, p, bytes); }
hipError_t hipFree(void* p) { return free_from(g_dev, p, "hipFree"); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return alloc_into(g_host, p, bytes); }
hipError_t hipHostFree(void* p) { return free_from(g_host, p, "hipHostFree"); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) {
    if (!dev) return hipErrorInvalidValue;
    *dev = nullptr;
    auto it = g_host.upper_bound(host);            // the allocation that starts at or before `host`
    if (it == g_host.begin()) return hipErrorInvalidValue;
    --it;
    const char* base = static_cast<const char*>(it->first);
    if (static_cast<const char*>(host) >= base + (it->second.asked ? it->second.asked : 1)) return hipErrorInvalidValue;
    *dev = host;
    return hipSuccess;
}

hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    if (bytes) memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) { return hipMemcpy(dst, src, bytes, kind); }
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t) {
    if (width > dpitch || width > spitch) return hipErrorInvalidValue;
    for (size_t r = 0; r < height; r++)
        if (width) memmove(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, width);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    bytes = clamp_whole_fill(dst, bytes);
    if (bytes) memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipMemsetD32Async(hipDeviceptr_t dst, int value, size_t count, hipStream_t) {
    if (reinterpret_cast<uintptr_t>(dst) & 3u) return hipErrorInvalidValue;
    int32_t* p = static_cast<int32_t*>(dst);
    for (size_t i = 0; i < count; i++) p[i] = value;
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    if (!s) return hipErrorInvalidValue;
    *s = new fakeStream{0};
    g_streams++;
    return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s) { return hipStreamCreateWithFlags(s, 0); }
hipError_t hipStreamDestroy(hipStream_t s) {
    if (!s) return hipErrorInvalidResourceHandle;
    delete s;
    g_streams--;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned) { return e ? hipSuccess : hipErrorInvalidResourceHandle; }
hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode) {
    if (!s || s->capturing) return hipErrorInvalidValue;
    s->capturing = 1;
    return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t* graph) {
    if (!s || !s->capturing || !graph) return hipErrorInvalidValue;
    s->capturing = 0;
    *graph = new fakeGraph{0};
    g_graphs++;
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    if (!e) return hipErrorInvalidValue;
    *e = new fakeEvent{0};
    g_events++;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) {
    if (!e) return hipErrorInvalidResourceHandle;
    delete e;
    g_events--;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { if (!e) return hipErrorInvalidResourceHandle; e->recorded = 1; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { return e ? hipSuccess : hipErrorInvalidResourceHandle; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    if (!ms || !a || !b) return hipErrorInvalidValue;
    *ms = 0.0f;
    return hipSuccess;
}

hipError_t hipGraphInstantiate(hipGraphExec_t* exec, hipGraph_t graph, hipGraphNode_t*, char*, size_t) {
    if (!exec || !graph) return hipErrorInvalidValue;
    *exec = new fakeGraphExec{0};
    g_execs++;
    return hipSuccess;
}
hipError_t hipGraphUpload(hipGraphExec_t exec, hipStream_t) { return exec ? hipSuccess : hipErrorInvalidResourceHandle; }
hipError_t hipGraphLaunch(hipGraphExec_t exec, hipStream_t) { if (!exec) return hipErrorInvalidResourceHandle; exec->launches++; return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t exec) {
    if (!exec) return hipErrorInvalidResourceHandle;
    delete exec;
    g_execs--;
    return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t graph) {
    if (!graph) return hipErrorInvalidResourceHandle;
    delete graph;
    g_graphs--;
    return hipSuccess;
}

fake_hip_counts fake_hip_live(void) {
    return fake_hip_counts{(long long)g_dev.size(), (long long)g_host.size(), g_streams, g_events, g_graphs, g_execs};
}
int fake_hip_live_total(void) {
    const fake_hip_counts c = fake_hip_live();
    return (int)(c.allocs + c.host_allocs + c.streams + c.events + c.graphs + c.graph_execs);
}
void fake_hip_report(void) {
    const fake_hip_counts c = fake_hip_live();
    fprintf(stderr, "fake_hip ledger: %lld device allocations, %lld host allocations, %lld streams, %lld events, %lld graphs, %lld graph-execs alive\n", c.allocs,
            c.host_allocs, c.streams, c.events, c.graphs, c.graph_execs);
    for (const auto& a : g_dev) fprintf(stderr, "  device allocation %p: %zu bytes\n", a.first, a.second.asked);
    for (const auto& a : g_host) fprintf(stderr, "  host allocation %p: %zu bytes\n", a.first, a.second.asked);
}
void fake_hip_short_only(int nth) { g_short_picked = true; g_short_countdown = nth; }
int fake_hip_short_bytes(void) { return FAKE_HIP_SHORT; }

}  // extern "C"
