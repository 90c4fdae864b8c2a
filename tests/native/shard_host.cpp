// The per-frame decision of the gfx950 shard kernels (beholder_amd/ops/hip/telemetry_shard.hpp),
// compiled for the host and run over a framed stream. Built by tests/test_hip_shard_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   shard_host_asan upb|protobufjs STREAM SHARDS FLAGS
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); SHARDS and FLAGS are the
// decimal values of ShardParams (ops/gpu_shard.py shard_params). One line per frame goes to stdout:
// drop, host where the device leaves the frame to the host, or the shard number.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_shard.hpp"

using namespace bh;

using Route = int (*)(const uint8_t*, int, int, const ShardParams&);

int main(int argc, char** argv) {
  Route route_frame = nullptr;
  if (argc == 5 && std::string(argv[1]) == "upb") route_frame = route<DIALECT_UPB>;
  if (argc == 5 && std::string(argv[1]) == "protobufjs") route_frame = route<DIALECT_PROTOBUFJS>;
  if (!route_frame) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM SHARDS FLAGS\n", argv[0]);
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
  const ShardParams params{static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10)),
                           static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10))};
  if (params.shards < 1 || params.shards > MAX_SHARDS) {
    std::fprintf(stderr, "SHARDS is 1-%u\n", MAX_SHARDS);
    return 2;
  }
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
    const int r = route_frame(exact.get(), 0, int(size), params);
    if (r == ROUTE_DROP) std::puts("drop");
    else if (r == ROUTE_HOST) std::puts("host");
    else std::printf("%d\n", r);
  }
  return 0;
}
