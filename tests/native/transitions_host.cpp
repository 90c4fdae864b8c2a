// The per-frame code of the gfx950 transitions kernels (beholder_amd/ops/hip/telemetry_transitions.hpp),
// compiled for the host and run over a framed stream. Built by tests/test_hip_transitions_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   transitions_host_asan upb|protobufjs STREAM KNOWN_MASK
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); KNOWN_MASK is the decimal
// value of ops/gpu_fold.py known_mask. One line per frame goes to stdout: skip for a frame that is
// not read, error, host where the device leaves the frame to the host, or
// `event ID STATUS CLASS HASH` with the id's bytes in hex (`-` for an empty id) and the class as
// class_of gives it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_transitions.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, StatusEvent&);

int main(int argc, char** argv) {
  Classify classify_frame = nullptr;
  if (argc == 4 && std::string(argv[1]) == "upb") classify_frame = classify<DIALECT_UPB>;
  if (argc == 4 && std::string(argv[1]) == "protobufjs") classify_frame = classify<DIALECT_PROTOBUFJS>;
  if (!classify_frame) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM KNOWN_MASK\n", argv[0]);
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
  const uint64_t known_mask = std::strtoull(argv[3], nullptr, 10);
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
    StatusEvent ev;
    const int kind = classify_frame(exact.get(), 0, int(size), ev);
    if (kind != ev.kind) {
      std::fprintf(stderr, "classify returns %d and writes kind %d\n", kind, ev.kind);
      return 2;
    }
    if (kind == TR_SKIP) std::puts("skip");
    else if (kind == TR_ERROR) std::puts("error");
    else if (kind == TR_HOST) std::puts("host");
    else {
      if (ev.id_len < 0 || (ev.id_len > 0 && (ev.id_off < 5 || size_t(ev.id_off) + size_t(ev.id_len) > size))) {
        std::fprintf(stderr, "id span [%d, +%d) outside a frame of %zu bytes\n", ev.id_off, ev.id_len, size);
        return 2;
      }
      std::fputs("event ", stdout);
      if (ev.id_len == 0) std::fputs("-", stdout);
      for (int k = 0; k < ev.id_len; ++k) std::printf("%02x", exact[size_t(ev.id_off) + size_t(k)]);
      std::printf(" %d %u %llu\n", ev.status, class_of(ev.status, known_mask), static_cast<unsigned long long>(ev.hash));
    }
  }
  return 0;
}
