// The per-frame decision and key hash of the gfx950 coalesce kernels
// (beholder_amd/ops/hip/telemetry_coalesce.hpp), compiled for the host and run over a framed stream.
// Built by tests/test_hip_coalesce_host.py with -fsanitize=address,undefined: every frame is read from
// a heap block of exactly its own size, so a read one byte past a frame is a sanitizer report here,
// not a fault on a GPU.
//
//   coalesce_host_asan upb|protobufjs STREAM FLAGS
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); FLAGS is the decimal value of
// CoalesceParams::flags (ops/gpu_coalesce.py policy_flags). One line per frame goes to stdout:
// drop, keep, host where the device leaves the frame to the host, or for a keyed frame
//   key TOPIC STATUS ID_OFF ID_LEN HASH
// with ID_OFF counted from the start of the frame's body and HASH as 16 hex digits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_coalesce.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, const CoalesceParams&, CoalesceKey&);

int main(int argc, char** argv) {
  Classify classify_frame = nullptr;
  if (argc == 4 && std::string(argv[1]) == "upb") classify_frame = classify<DIALECT_UPB>;
  if (argc == 4 && std::string(argv[1]) == "protobufjs") classify_frame = classify<DIALECT_PROTOBUFJS>;
  if (!classify_frame) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM FLAGS\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[2], std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (data.size() >= (1u << 31)) {
    std::fprintf(stderr, "stream too large for int32 offsets\n");
    return 2;
  }
  const CoalesceParams params{~0ull, static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10)), 1};
  const size_t n = data.size();
  for (size_t i = 0; i < n;) {
    uint32_t L = 0;
    if (n - i >= 4) std::memcpy(&L, &data[i], 4);  // little-endian hosts only, as the kernels' are
    if (L == 0 || n - i - 4 < L) {
      std::fprintf(stderr, "truncated or empty frame at byte %zu\n", i);
      return 2;
    }
    const size_t size = 4 + size_t(L);
    const std::unique_ptr<uint8_t[]> exact(new uint8_t[size]);
    std::memcpy(exact.get(), &data[i], size);
    i += size;
    CoalesceKey key{0, 0, 0, 0, 0};
    switch (classify_frame(exact.get(), 0, int(size), params, key)) {
      case CL_DROP: std::puts("drop"); break;
      case CL_KEEP: std::puts("keep"); break;
      case CL_HOST: std::puts("host"); break;
      default:
        // an absent id has offset 0 and length 0: it is printed as offset 0 of the body
        std::printf("key %u %d %d %d %016llx\n", key.topic, key.status, key.id_len ? key.id_off - 5 : 0, key.id_len,
                    static_cast<unsigned long long>(key.hash));
    }
  }
  return 0;
}
