// The telemetry readers of the gfx950 kernels (beholder_amd/ops/hip/telemetry_readers.hpp), compiled
// for the host and run over a framed stream. Built by tests/test_hip_readers_host.py with
// -fsanitize=address,undefined: every body is read from a heap block of exactly its own size, so a
// reader that steps one byte past its message is a sanitizer report here, not a fault on a GPU.
//
//   readers_host_asan upb|upb-strict|protobufjs STREAM
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py). For each frame of topic 1
// (read as a TelemetryStatus) or 2 (a TelemetryProgress) one line goes to stdout, the Row:
//   id_off id_len status progress host_off host_len ok seen
// with the offsets of the fields the message carried put back to positions in STREAM.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_readers.hpp"

using namespace bh;

using Reader = void (*)(const uint8_t*, const int&, const int&, bool, Row&);

static Reader reader_for(const std::string& mode) {
  if (mode == "upb") return read_message<DIALECT_UPB, false>;
  if (mode == "upb-strict") return read_message<DIALECT_UPB, true>;
  if (mode == "protobufjs") return read_message<DIALECT_PROTOBUFJS, false>;
  return nullptr;
}

int main(int argc, char** argv) {
  const Reader read = argc == 3 ? reader_for(argv[1]) : nullptr;
  if (!read) {
    std::fprintf(stderr, "usage: %s upb|upb-strict|protobufjs STREAM\n", argv[0]);
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
  const size_t n = data.size();
  for (size_t i = 0; i < n;) {
    uint32_t L = 0;
    if (n - i >= 4) std::memcpy(&L, &data[i], 4);  // little-endian hosts only, as the kernels' are
    if (L == 0 || n - i - 4 < L) {
      std::fprintf(stderr, "truncated or empty frame at byte %zu\n", i);
      return 2;
    }
    const int topic = data[i + 4];
    const size_t body = i + 5, size = L - 1;
    i += 4 + size_t(L);
    if (topic != 1 && topic != 2) continue;
    const std::unique_ptr<uint8_t[]> exact(new uint8_t[size]);
    if (size) std::memcpy(exact.get(), &data[body], size);
    Row r;
    read(exact.get(), 0, int(size), topic == 1, r);
    if (r.seen & SEEN_ID) r.id_off += int(body);
    if (r.seen & SEEN_HOST) r.host_off += int(body);
    std::printf("%d %d %d %d %d %d %d %d\n", r.id_off, r.id_len, r.status, r.progress, r.host_off, r.host_len, r.ok,
                r.seen);
  }
  return 0;
}
