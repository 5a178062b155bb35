// A fake HIP runtime for the host-side sanitizer harness (tests/hostcheck): exactly the types, enums and functions that
// gym_novel_gridworlds_amd/csrc/ngw_abi_*.cpp and ngw_host.h use, declared with the real runtime's signatures.  "Device" memory is plain
// heap memory of exactly the requested size, copies and fills run at once on the host, streams / events / graphs are bookkeeping.  No kernel
// runs here: the *_launch functions of ngw_device.h are stubs (fake_kernels.cpp).  fake_hip.cpp says what each call guarantees.
#ifndef NGW_FAKE_HIP_RUNTIME_H
#define NGW_FAKE_HIP_RUNTIME_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue = 1,
    hipErrorOutOfMemory = 2,
    hipErrorInvalidResourceHandle = 400,
    hipErrorNotReady = 600
} hipError_t;

typedef struct fakeStream* hipStream_t;
typedef struct fakeEvent* hipEvent_t;
typedef struct fakeGraph* hipGraph_t;
typedef struct fakeGraphExec* hipGraphExec_t;
typedef struct fakeGraphNode* hipGraphNode_t;
typedef void* hipDeviceptr_t;

typedef enum hipMemcpyKind {
    hipMemcpyHostToHost = 0,
    hipMemcpyHostToDevice = 1,
    hipMemcpyDeviceToHost = 2,
    hipMemcpyDeviceToDevice = 3,
    hipMemcpyDefault = 4
} hipMemcpyKind;

typedef enum hipStreamCaptureMode {
    hipStreamCaptureModeGlobal = 0,
    hipStreamCaptureModeThreadLocal = 1,
    hipStreamCaptureModeRelaxed = 2
} hipStreamCaptureMode;

#define hipHostMallocDefault 0x0
#define hipHostMallocMapped 0x2
#define hipStreamNonBlocking 0x1
#define hipEventDisableTiming 0x2

const char* hipGetErrorString(hipError_t e);
hipError_t hipGetLastError(void);
hipError_t hipGetDeviceCount(int* count);
hipError_t hipSetDevice(int device);

hipError_t hipMalloc(void** p, size_t bytes);
hipError_t hipFree(void* p);
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags);
hipError_t hipHostFree(void* p);
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned flags);

hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream);
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind,
                            hipStream_t stream);
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream);
hipError_t hipMemsetD32Async(hipDeviceptr_t dst, int value, size_t count, hipStream_t stream);

hipError_t hipStreamCreate(hipStream_t* s);
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);
hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode mode);
hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t* graph);

hipError_t hipEventCreate(hipEvent_t* e);
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventSynchronize(hipEvent_t e);
hipError_t hipEventElapsedTime(float* ms, hipEvent_t start, hipEvent_t stop);

hipError_t hipGraphInstantiate(hipGraphExec_t* exec, hipGraph_t graph, hipGraphNode_t* error_node, char* log, size_t log_bytes);
hipError_t hipGraphUpload(hipGraphExec_t exec, hipStream_t s);
hipError_t hipGraphLaunch(hipGraphExec_t exec, hipStream_t s);
hipError_t hipGraphExecDestroy(hipGraphExec_t exec);
hipError_t hipGraphDestroy(hipGraph_t graph);

/* ---- the harness's own window into the fake (not HIP) */
typedef struct fake_hip_counts {
    long long allocs, host_allocs, streams, events, graphs, graph_execs;
} fake_hip_counts;
fake_hip_counts fake_hip_live(void);            /* what is alive now */
int fake_hip_live_total(void);                  /* the sum of the six */
void fake_hip_report(void);                     /* prints every live object to stderr, allocations with their sizes */
/* -DFAKE_HIP_SHORT=<bytes> builds only (a no-op otherwise): from now on ONLY the allocation `nth` calls of hipMalloc / hipHostMalloc ahead
 * (0 = the next one) is handed out short; without this call every allocation is. */
void fake_hip_short_only(int nth);
int fake_hip_short_bytes(void);                 /* FAKE_HIP_SHORT of this build, 0 in the ordinary one */

#ifdef __cplusplus
}
#endif
#endif
