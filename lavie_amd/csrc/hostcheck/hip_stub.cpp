// Stand-in for libamdhip64 used ONLY by `make asan` (host-side AddressSanitizer / UBSan build of the engine's planning,
// packing and argument code; SURVEY.md section 5 "ASan on the host C++ shim").  "Device" memory is host heap, copies are memcpy,
// kernel launches do nothing: what runs under the sanitizers is every line of HOST code in lavie_amd/csrc (parameter inventory,
// weight-arena carving, workspace dry run and bump allocation, split-K / tile planning, C-ABI argument checks), with every
// hipMemcpy* bounds-checked by ASan against the exact-size heap blocks behind it.  Never linked into liblavie_hip.so.
#include <hip/hip_runtime_api.h>

#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

extern "C" {

hipError_t hipMalloc(void** p, size_t n) {
    *p = malloc(n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memmove(d, s, n); return hipSuccess; }
static void trace_copy(size_t n, hipMemcpyKind kind);
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind kind, hipStream_t) {
    trace_copy(n, kind);
    memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
hipError_t hipMemcpyFromSymbol(void* d, const void*, size_t n, size_t, hipMemcpyKind) { memset(d, 0, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip stub"; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = nullptr; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) { *st = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* g) { *g = nullptr; return hipErrorNotSupported; }
hipError_t hipGraphInstantiate(hipGraphExec_t*, hipGraph_t, hipGraphNode_t*, char*, size_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

// kernel launch plumbing of clang's host stubs: configuration push / pop and a launch that does nothing
static thread_local struct { dim3 grid, block; size_t shmem; hipStream_t stream; } g_cfg;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    g_cfg.grid = grid; g_cfg.block = block; g_cfg.shmem = shmem; g_cfg.stream = stream;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    *grid = g_cfg.grid; *block = g_cfg.block; *shmem = g_cfg.shmem; *stream = g_cfg.stream;
    return hipSuccess;
}
// Launch trace: one line per launch (kernel, grid, block, dynamic LDS) to g_trace.  The driver's `trace` mode points it at a file;
// LAVIE_HOSTCHECK_TRACE=1 sends it to stderr.  Kernel names come from clang's registration calls.
static long g_launches = 0;
static unsigned g_last_grid_x = 0;     // of the latest launch (the driver's check of lavie_debug_rowfuse_grid)
static FILE* g_trace = getenv("LAVIE_HOSTCHECK_TRACE") ? stderr : nullptr;
// The driver's `trace` mode also records every asynchronous device-to-device copy, as "copy BYTES" (no addresses): the forward
// enqueues some, next to its launches.  Off elsewhere: to the readers of an operator trace every line is a launch.
static bool g_trace_copies = false;
static void trace_copy(size_t n, hipMemcpyKind kind) {
    if (g_trace && g_trace_copies && kind == hipMemcpyDeviceToDevice) fprintf(g_trace, "copy %zu\n", n);
}
static std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
static const char* kernel_name(const void* f) {
    auto it = kernel_names().find(f);
    return it == kernel_names().end() ? "?" : it->second.c_str();
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t shmem, hipStream_t) {
    // the launch geometry itself is host logic worth checking
    const char* bad = grid.x == 0 || grid.y == 0 || grid.z == 0          ? "empty grid"
                      : block.x * block.y * block.z == 0               ? "empty block"
                      : block.x * block.y * block.z > 1024             ? "more than 1024 threads per block"
                      : shmem > 160 * 1024                             ? "dynamic LDS above 160 KiB"
                                                                       : nullptr;
    if (bad) {
        fprintf(stderr, "hip_stub: launch of %s refused (%s): grid %u,%u,%u block %u,%u,%u lds %zu\n", kernel_name(f), bad, grid.x, grid.y,
                grid.z, block.x, block.y, block.z, shmem);
        abort();
    }
    ++g_launches;
    g_last_grid_x = grid.x;
    if (g_trace) fprintf(g_trace, "%s %u,%u,%u %u,%u,%u %zu\n", kernel_name(f), grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem);
    return hipSuccess;
}
hipError_t hipExtLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t shmem, hipStream_t s, hipEvent_t, hipEvent_t, int) {
    return hipLaunchKernel(f, grid, block, args, shmem, s);
}
long lavie_hostcheck_launches() { return g_launches; }
long lavie_hostcheck_last_grid_x() { return (long)g_last_grid_x; }
void lavie_hostcheck_trace_to(FILE* f) { g_trace = f; }
void lavie_hostcheck_trace_copies(int on) { g_trace_copies = on != 0; }
// every kernel name the registration calls have seen, sorted, one per line (the driver's `kernels` mode)
void lavie_hostcheck_kernel_names_to(FILE* f) {
    std::map<std::string, int> names;
    for (const auto& kv : kernel_names()) names[kv.second] = 1;
    for (const auto& kv : names) fprintf(f, "%s\n", kv.first.c_str());
}
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
// kernel names: the demangled name without namespace, return type and parameter list, e.g. igemm_kernel<2, 2, 4, 5, 2, true, 0>
void __hipRegisterFunction(void**, const void* f, char*, const char* mangled, unsigned, void*, void*, void*, void*, int*) {
    std::string m = mangled;                         // the demangler does not know _Float16 (DF16_): spell it as half (Dh)
    for (size_t i; (i = m.find("DF16_")) != std::string::npos;) m.replace(i, 5, "Dh");
    int st = 0;
    char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &st);
    std::string n = st == 0 && d ? d : mangled;
    free(d);
    if (n.compare(0, 5, "void ") == 0) n.erase(0, 5);
    if (n.compare(0, 7, "lavie::") == 0) n.erase(0, 7);
    int depth = 0;                                   // cut the parameter list: the first '(' outside template brackets
    for (size_t i = 0; i < n.size(); ++i) {
        if (n[i] == '<') ++depth;
        else if (n[i] == '>') --depth;
        else if (n[i] == '(' && depth == 0) { n.resize(i); break; }
    }
    kernel_names()[f] = n;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void*, void*, const char*, size_t, unsigned) {}
}
