// Host-only stand-in for the HIP runtime entry points that libmixdq_hip's objects call.  It runs nothing: it keeps
// the kernel names that __hipRegisterFunction hands over and appends one line per event to an in-memory log, which
// tests/launch_trace.py reads back after every call:
//   launch <mangled kernel> <grid x,y,z> <block x[,y,z]> <dynamic LDS bytes>
//   attr <mangled kernel> <bytes>            (hipFuncSetAttribute: the > 64 KiB LDS opt-in)
//   sync | to_symbol <bytes> | from_symbol <bytes> | memcpy <bytes>
// Linked with g++ against mixdq_amd/_obj/*.o (never against libamdhip64); no pointer it is given is dereferenced.
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace {
struct dim3 { unsigned x, y, z; };
std::map<const void*, std::string>& names() { static std::map<const void*, std::string> m; return m; }
std::vector<std::string>& events() { static std::vector<std::string> v; return v; }
dim3 g_grid, g_block;
size_t g_lds;
void* g_stream;
int g_device = 0, g_capture_status = 0;
unsigned long long g_capture_id = 0;

std::string kernel_name(const void* f) {
  auto it = names().find(f);
  return it == names().end() ? "?" : it->second;
}
std::string dims(dim3 d, bool always3) {
  std::string s = std::to_string(d.x);
  if (always3 || d.y != 1 || d.z != 1) s += "," + std::to_string(d.y) + "," + std::to_string(d.z);
  return s;
}
}  // namespace

#define EXPORT extern "C" __attribute__((visibility("default")))

// ---- what hipcc's host code calls ---------------------------------------------------------------------------
EXPORT void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
EXPORT void __hipUnregisterFatBinary(void**) {}
EXPORT void __hipRegisterFunction(void**, const void* host, char*, const char* device, unsigned, void*, void*, void*,
                                  void*, int*) { names()[host] = device; }
EXPORT void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
EXPORT int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, void* stream) {
  g_grid = grid, g_block = block, g_lds = lds, g_stream = stream;
  return 0;
}
EXPORT int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, void** stream) {
  *grid = g_grid, *block = g_block, *lds = g_lds, *stream = g_stream;
  return 0;
}
EXPORT int hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, void*) {
  events().push_back("launch " + kernel_name(f) + " " + dims(grid, true) + " " + dims(block, false) + " " +
                     std::to_string(lds));
  return 0;
}
EXPORT int hipGetLastError() { return 0; }
EXPORT int hipGetDevice(int* device) { *device = g_device; return 0; }
EXPORT int hipFuncSetAttribute(const void* f, int, int value) {
  events().push_back("attr " + kernel_name(f) + " " + std::to_string(value));
  return 0;
}
EXPORT int hipStreamGetCaptureInfo(void*, int* status, unsigned long long* id) {
  if (status) *status = g_capture_status;
  if (id) *id = g_capture_id;
  return 0;
}
EXPORT int hipStreamSynchronize(void*) { events().push_back("sync"); return 0; }
EXPORT int hipMemcpyFromSymbolAsync(void*, const void*, size_t bytes, size_t, int, void*) {
  events().push_back("from_symbol " + std::to_string(bytes));
  return 0;
}
EXPORT int hipMemcpyToSymbol(const void*, const void*, size_t bytes, size_t, int) {
  events().push_back("to_symbol " + std::to_string(bytes));
  return 0;
}
EXPORT int hipMemcpyAsync(void*, const void*, size_t bytes, int, void*) {
  events().push_back("memcpy " + std::to_string(bytes));
  return 0;
}
EXPORT int hipDeviceGetAttribute(int* value, int, int) { *value = 256; return 0; }   // the multiprocessor count
EXPORT int hipOccupancyMaxActiveBlocksPerMultiprocessor(int* blocks, const void*, int, size_t) {
  *blocks = 1;
  return 0;
}

// ---- what the driver calls ----------------------------------------------------------------------------------
// The log so far, one event per line, and an empty log afterwards (the pointer is good until the next call).
EXPORT const char* launch_trace_take() {
  static std::string out;
  out.clear();
  for (const std::string& e : events()) out += e + "\n";
  events().clear();
  return out.c_str();
}
EXPORT void launch_trace_set_device(int device) { g_device = device; }
// status: 0 none, 1 active (hipStreamCaptureStatus); id: what hipStreamGetCaptureInfo reports with it
EXPORT void launch_trace_set_capture(int status, unsigned long long id) { g_capture_status = status, g_capture_id = id; }
// Every registered kernel, one mangled name per line.
EXPORT const char* launch_trace_kernels() {
  static std::string out;
  out.clear();
  for (const auto& kv : names()) out += kv.second + "\n";
  return out.c_str();
}
