// The per-frame code of the gfx950 thin kernels (beholder_amd/ops/hip/telemetry_thin.hpp), compiled for
// the host and run over a framed stream. Built by tests/test_hip_thin_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   thin_host_asan upb|protobufjs STREAM STEP
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); STEP is the policy's step in
// decimal, 1 .. 2^31 - 1. One line per frame goes to stdout: skip for a frame that is not read, error,
// host where the device leaves the frame to the host, or `event ID STATUS BUCKET HASH` with the id's
// bytes in hex (`-` for an empty id) and status and bucket as the mark word holds them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_thin.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, int32_t, StatusEvent&, uint64_t&);

int main(int argc, char** argv) {
  Classify classify_frame = nullptr;
  if (argc == 4 && std::string(argv[1]) == "upb") classify_frame = thin_classify<DIALECT_UPB>;
  if (argc == 4 && std::string(argv[1]) == "protobufjs") classify_frame = thin_classify<DIALECT_PROTOBUFJS>;
  const long long step = classify_frame ? std::strtoll(argv[3], nullptr, 10) : 0;
  if (!classify_frame || step < 1 || step > 2147483647ll) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM STEP\n", argv[0]);
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
    const size_t size = 4 + size_t(L);
    const std::unique_ptr<uint8_t[]> exact(new uint8_t[size]);
    std::memcpy(exact.get(), &data[i], size);
    i += size;
    StatusEvent ev;
    uint64_t mark = 0;
    const int kind = classify_frame(exact.get(), 0, int(size), int32_t(step), ev, mark);
    if (kind != ev.kind) {
      std::fprintf(stderr, "thin_classify returns %d and writes kind %d\n", kind, ev.kind);
      return 2;
    }
    if (kind != TH_EVENT && mark != 0) {
      std::fprintf(stderr, "a frame that is no event has the mark word %llu\n", static_cast<unsigned long long>(mark));
      return 2;
    }
    if (kind == TH_SKIP) std::puts("skip");
    else if (kind == TH_ERROR) std::puts("error");
    else if (kind == TH_HOST) std::puts("host");
    else {
      if (ev.id_len < 0 || (ev.id_len > 0 && (ev.id_off < 5 || size_t(ev.id_off) + size_t(ev.id_len) > size))) {
        std::fprintf(stderr, "id span [%d, +%d) outside a frame of %zu bytes\n", ev.id_off, ev.id_len, size);
        return 2;
      }
      if (static_cast<int32_t>(mark >> 32) != ev.status) {
        std::fprintf(stderr, "the mark word's status differs from the row's\n");
        return 2;
      }
      std::fputs("event ", stdout);
      if (ev.id_len == 0) std::fputs("-", stdout);
      for (int k = 0; k < ev.id_len; ++k) std::printf("%02x", exact[size_t(ev.id_off) + size_t(k)]);
      std::printf(" %d %d %llu\n", static_cast<int32_t>(mark >> 32), static_cast<int32_t>(mark & 0xffffffffull),
                  static_cast<unsigned long long>(ev.hash));
    }
  }
  return 0;
}
