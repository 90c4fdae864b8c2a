// Batched telemetry decode on the GPU (gfx950): the offload probe behind docs/DESIGN.md
// "Why there are no HIP kernels".
//
// The service decodes one ~50-byte protobuf per event on the CPU (ops/csrc/py_codec.cpp, the
// `decode` of index.js:63,129). This kernel decodes a whole batch of TelemetryProgress /
// TelemetryStatus messages (models/proto/api.proto: mediaId=1, status=2, progress=3, host=4)
// so scripts/gpu_offload_probe.py can price the alternative design: gather events into a
// pinned batch, copy it to HBM, decode, copy the fields back.
//
// Layout: `buf` holds the concatenated message bodies, `offs[n + 1]` their boundaries (checked
// on the host: offs[0] = 0, non-decreasing, offs[n] = bytes in buf). One lane per message: the
// work is a varint state machine with data-dependent branches, so a 64-wide wavefront decodes 64
// messages side by side and diverges where their layouts differ. Each lane emits one Row, 8 int32:
//   {id_off, id_len, status, progress, host_off, host_len, ok, seen}
// (offsets are absolute in buf; ok = OK_ERROR, 0, where the CPU codec raises DecodeError).
//
// The readers, their two dialects (protobufjs, the service's default, and upb) and the message
// types they know are in telemetry_readers.hpp, shared with telemetry_fold.hip. This kernel reads
// every message as a TelemetryProgress with the plain upb reader, as it always has.
#include "telemetry_readers.hpp"

namespace {

using namespace bh;

template <int DIALECT>
__global__ __launch_bounds__(256) void decode_telemetry(const uint8_t* __restrict__ buf,
                                                        const int32_t* __restrict__ offs, int n,
                                                        int4* __restrict__ out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const int start = offs[m];
  const int end = offs[m + 1];
  Row r;
  read_message<DIALECT, false>(buf, start, end, false, r);  // a TelemetryProgress, upb in its plain form
  out[2 * m] = make_int4(r.id_off, r.id_len, r.status, r.progress);
  out[2 * m + 1] = make_int4(r.host_off, r.host_len, r.ok, r.seen);
}

}  // namespace

// C ABI for ctypes (ops/gpu_decode.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t); `dialect` 0 = upb, 1 = protobufjs.
// Returns a hipError_t (hipErrorInvalidValue for an unknown dialect).
extern "C" __attribute__((visibility("default"))) int bh_decode_telemetry(const void* buf, const void* offs, int n,
                                                                         void* out, int dialect, void* stream) {
  if (n <= 0) return 0;
  if (dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) return static_cast<int>(hipErrorInvalidValue);
  const int block = 256;
  const int grid = (n + block - 1) / block;
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* t = static_cast<int4*>(out);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(decode_telemetry<DIALECT_PROTOBUFJS>, dim3(grid), dim3(block), 0,
                       static_cast<hipStream_t>(stream), b, o, n, t);
  else
    hipLaunchKernelGGL(decode_telemetry<DIALECT_UPB>, dim3(grid), dim3(block), 0, static_cast<hipStream_t>(stream),
                       b, o, n, t);
  return static_cast<int>(hipGetLastError());
}
