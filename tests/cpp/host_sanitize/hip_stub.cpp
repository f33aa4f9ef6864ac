// hip_stub.cpp — TEST INFRASTRUCTURE: a stand-in for the HIP runtime on host memory, for the CPU-only sanitizer build of the PRODUCT's host code
// (tests/test_host_sanitizers.py).  The library's translation units are compiled host-only (`hipcc --cuda-host-only -fsanitize=address,undefined`)
// and linked against this file instead of libamdhip64: "device" memory is calloc'ed host memory (so AddressSanitizer sees every byte the host
// code uploads, every table it builds and every staging copy), copies are memcpy, kernel launches return success without running anything
// (the device code is not part of this build).  What runs for real is everything the host side does: geometry, planners (pyramid fusion /
// chains, FAST work items, quadtree key tables), workspace sizing, staging, the ingest ticket state machine, the vocabulary loaders.
// Nothing of this is linked into the product.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <map>
#include <mutex>

extern "C" {
typedef int hipError_t;                     // hipSuccess = 0
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;
struct dim3s { uint32_t x, y, z; };

static std::atomic<long> g_launches{0};
long hip_stub_launches() { return g_launches.load(); }
// what the host code asked of the runtime so far (host_sanitize.cpp prints it: two commits that claim the same behaviour print the same line).
// The launch digest is a SUM of per-launch hashes of (grid, block, dynamic LDS bytes), so it does not depend on the order of the launches.
enum { HS_C_LIVE_DEV, HS_C_LIVE_PIN, HS_C_MALLOC_CALLS, HS_C_MALLOC_BYTES, HS_C_PIN_CALLS, HS_C_PIN_BYTES, HS_C_H2D_CALLS, HS_C_H2D_BYTES,
       HS_C_D2H_CALLS, HS_C_D2H_BYTES, HS_C_MEMSET_CALLS, HS_C_MEMSET_BYTES, HS_C_LAUNCHES, HS_C_LAUNCH_DIGEST, HS_C_COUNT };
static std::atomic<unsigned long long> g_c[HS_C_COUNT];
void hip_stub_counters(unsigned long long* out /*[14]*/) { for (int i = 0; i < HS_C_COUNT; i++) out[i] = g_c[i].load(); out[HS_C_LAUNCHES] = (unsigned long long)g_launches.load(); }
static void count_copy(int kind, size_t bytes)       // hipMemcpyKind: 1 = host to device, 2 = device to host
{
    if (kind == 1) { g_c[HS_C_H2D_CALLS]++; g_c[HS_C_H2D_BYTES] += bytes; }
    if (kind == 2) { g_c[HS_C_D2H_CALLS]++; g_c[HS_C_D2H_BYTES] += bytes; }
}
static unsigned long long mix64(unsigned long long v) { v ^= v >> 33; v *= 0xff51afd7ed558ccdull; v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ull; return v ^ (v >> 33); }

hipError_t hipGetDeviceCount(int* n) { *n = 1; return 0; }
hipError_t hipSetDevice(int) { return 0; }
hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
hipError_t hipDeviceSynchronize() { return 0; }
hipError_t hipGetLastError() { return 0; }
const char* hipGetErrorString(hipError_t) { return "hip_stub"; }
// live "device" allocations, so that a test can put them back into the state a kernel-less run starts from (hip_stub_zero_device)
static std::mutex g_dev_mu;
// a block's owner is a number handed to each thread once and never again (a std::thread::id is reused after a join: a block that outlives its
// thread, a published frame for instance, would then pass for a later thread's)
static std::atomic<unsigned long long> g_next_owner{1};
static unsigned long long my_owner() { static thread_local const unsigned long long id = g_next_owner++; return id; }
struct DevBlock { size_t n; unsigned long long owner; };
static std::map<void*, DevBlock> g_dev;
hipError_t hipMalloc(void** p, size_t n)
{
    *p = calloc(n ? n : 1, 1);
    if (*p) { std::lock_guard<std::mutex> g(g_dev_mu); g_dev[*p] = DevBlock{ n, my_owner() }; g_c[HS_C_LIVE_DEV]++; g_c[HS_C_MALLOC_CALLS]++; g_c[HS_C_MALLOC_BYTES] += n; }
    return *p ? 0 : 2;
}
hipError_t hipFree(void* p) { { std::lock_guard<std::mutex> g(g_dev_mu); if (g_dev.erase(p)) g_c[HS_C_LIVE_DEV]--; } free(p); return 0; }
// no kernel writes the outputs here: a reused allocation would hand the host code the last call's uploads as "results" (indices, counts).  Zero
// everything instead, as a fresh allocation is — everything the CALLING THREAD allocated: another thread's handle may be in the middle of a call.
// (What other threads allocated and left behind, the frames the cache section's publisher threads published for instance, is therefore no longer
// zeroed by the main thread's later calls: the driver clears the cache at the end of that section.)
void hip_stub_zero_device() { std::lock_guard<std::mutex> g(g_dev_mu); const auto me = my_owner(); for (auto& a : g_dev) if (a.second.owner == me) memset(a.first, 0, a.second.n); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = calloc(n ? n : 1, 1); if (*p) { g_c[HS_C_LIVE_PIN]++; g_c[HS_C_PIN_CALLS]++; g_c[HS_C_PIN_BYTES] += n; } return *p ? 0 : 2; }
hipError_t hipHostFree(void* p) { if (p) g_c[HS_C_LIVE_PIN]--; free(p); return 0; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, int k) { count_copy(k, n); memcpy(d, s, n); return 0; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, int k, hipStream_t) { return hipMemcpy(d, s, n, k); }
hipError_t hipMemcpy2D(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, int k) { count_copy(k, w * h); for (size_t y = 0; y < h; y++) memcpy((char*)d + y * dp, (const char*)s + y * sp, w); return 0; }
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, int k, hipStream_t) { return hipMemcpy2D(d, dp, s, sp, w, h, k); }
hipError_t hipMemset(void* d, int v, size_t n) { g_c[HS_C_MEMSET_CALLS]++; g_c[HS_C_MEMSET_BYTES] += n; memset(d, v, n); return 0; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { return hipMemset(d, v, n); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)calloc(1, 8); return 0; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return 0; }
hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return 0; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)calloc(1, 8); return 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)calloc(1, 8); return 0; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return 0; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
hipError_t hipEventSynchronize(hipEvent_t) { return 0; }
hipError_t hipEventQuery(hipEvent_t) { return 0; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return 0; }
hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
hipError_t hipMemcpyFromSymbol(void*, const void*, size_t, size_t, int) { return 0; }
hipError_t hipMemcpyToSymbol(const void*, const void*, size_t, size_t, int) { return 0; }
hipError_t hipGetSymbolAddress(void** p, const void*) { static char z[4096]; *p = z; return 0; }
// kernel launches: the host-side stubs clang generates for __global__ functions call these three
// (push keeps what kernel<<<grid, block, lds, stream>>> was given, pop hands it to the generated stub, which passes it on to hipLaunchKernel)
static thread_local struct { dim3s g, b; size_t lds; hipStream_t s; } t_cfg;
hipError_t __hipPushCallConfiguration(dim3s g, dim3s b, size_t lds, hipStream_t s) { t_cfg = { g, b, lds, s }; return 0; }
hipError_t __hipPopCallConfiguration(dim3s* g, dim3s* b, size_t* lds, hipStream_t* s) { *g = t_cfg.g; *b = t_cfg.b; *lds = t_cfg.lds; *s = t_cfg.s; return 0; }
hipError_t hipLaunchKernel(const void*, dim3s g, dim3s b, void**, size_t lds, hipStream_t)
{
    g_launches++;
    unsigned long long hsh = 0;
    for (unsigned long long v : { (unsigned long long)g.x, (unsigned long long)g.y, (unsigned long long)g.z, (unsigned long long)b.x, (unsigned long long)b.y, (unsigned long long)b.z, (unsigned long long)lds }) hsh = mix64(hsh * 31 + v + 1);
    g_c[HS_C_LAUNCH_DIGEST] += hsh;
    return 0;
}
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void**, void*, void*, const char*, size_t, unsigned) {}
void __hipUnregisterFatBinary(void**) {}
}
