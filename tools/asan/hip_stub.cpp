// Stub HIP runtime for the sanitizer build of the host-side plan builders (`make -C deepsphere-cosmo-tf2_amd/csrc asan`).
// "Device" memory is host memory from malloc -- so AddressSanitizer sees every table the builders upload (hipMemcpy = memcpy,
// both ends bounds-checked) -- kernel launches are accepted and dropped (the two set-up passes the builders READ BACK run on the
// host instead: DSPH_HOST_EMU in cheb_struct.hip), streams and events are tokens.  Test infrastructure only: nothing here is
// part of libdsphere_hip.so, and no compute entry point produces results under it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include <hip/hip_runtime_api.h>

// DSPH_STUB_TRACE=<file>: one line per kernel launch, event record and event wait is appended to that file -- what a compute
// entry point submits, in order, without a GPU.  Streams and events are tokens that spell their index of creation, so a trace
// names them "side1" / "event2" (the null stream: "caller") and is the same from run to run.
static FILE* trace_file() {
  static FILE* f = getenv("DSPH_STUB_TRACE") ? fopen(getenv("DSPH_STUB_TRACE"), "a") : nullptr;
  return f;
}
static std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
static void* token(const char* kind) {
  static long long created = 0;
  char* t = (char*)malloc(24);
  snprintf(t, 24, "%s%lld", kind, ++created);
  return t;
}
static const char* name_of(const void* t) { return t ? (const char*)t : "caller"; }

extern "C" {

hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int) { memset(p, 0, sizeof(*p)); p->multiProcessorCount = 256; return hipSuccess; }
void dsph_stub_trace_note(const char* text) {  // the driver's own lines: which call the launches below belong to
  if (FILE* f = trace_file()) { fprintf(f, "# %s\n", text); fflush(f); }
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)token("side"); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)token("event"); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  if (FILE* f = trace_file()) { fprintf(f, "record %s on %s\n", name_of(e), name_of(s)); fflush(f); }
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  if (FILE* f = trace_file()) { fprintf(f, "wait %s on %s\n", name_of(e), name_of(s)); fflush(f); }
  return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* s) { *s = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipLaunchKernel(const void* fn, dim3 g, dim3 b, void**, size_t shm, hipStream_t s) {
  if (FILE* f = trace_file()) {
    auto it = kernel_names().find(fn);
    fprintf(f, "launch %s grid %u %u %u block %u %u %u lds %zu on %s\n", it == kernel_names().end() ? "?" : it->second.c_str(), g.x, g.y, g.z,
            b.x, b.y, b.z, shm, name_of(s));
    fflush(f);
  }
  return hipSuccess;
}

// what the host half of a HIP translation unit calls at load time and around a <<< >>> launch
static dim3 g_grid, g_block;
static size_t g_shm;
static hipStream_t g_stream;
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  kernel_names()[host_fn] = device_name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t s) { g_grid = g; g_block = b; g_shm = shm; g_stream = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* shm, hipStream_t* s) { *g = g_grid; *b = g_block; *shm = g_shm; *s = g_stream; return hipSuccess; }
}
