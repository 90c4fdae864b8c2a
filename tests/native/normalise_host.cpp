// The per-frame code of the gfx950 normalise kernels (beholder_amd/ops/hip/telemetry_normalise.hpp),
// compiled for the host and run over a framed stream. Built by tests/test_hip_normalise_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   normalise_host_asan upb|protobufjs STREAM keep|drop
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py). One line per frame goes to
// stdout: `drop`, `host`, or `copy|status|progress FRAME GROWTH` with the output frame in hex, put
// together from canon_byte for every rel < canon_len, and its length minus the input frame's. The
// program fails where canon_len and the plan's out_len differ, where a span leaves the frame, or where
// a frame grows by more than NM_GROWTH_MAX.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_normalise.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, bool, Plan&);

static bool inside(int off, int len, size_t size) {
  return len >= 0 && (len == 0 || (off >= 5 && size_t(off) + size_t(len) <= size));
}

int main(int argc, char** argv) {
  Classify classify_frame = nullptr;
  if (argc == 4 && std::string(argv[1]) == "upb") classify_frame = norm_classify<DIALECT_UPB>;
  if (argc == 4 && std::string(argv[1]) == "protobufjs") classify_frame = norm_classify<DIALECT_PROTOBUFJS>;
  const std::string undecoded = argc == 4 ? argv[3] : "";
  if (!classify_frame || (undecoded != "keep" && undecoded != "drop")) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM keep|drop\n", argv[0]);
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
    Plan plan;
    const int kind = classify_frame(exact.get(), 0, int(size), undecoded == "drop", plan);
    if (kind != plan.kind) {
      std::fprintf(stderr, "norm_classify returns %d and writes kind %d\n", kind, plan.kind);
      return 2;
    }
    const int length = canon_len(plan);
    if (length != plan.out_len) {
      std::fprintf(stderr, "canon_len is %d and the plan's out_len %d\n", length, plan.out_len);
      return 2;
    }
    if (kind == NM_DROP || kind == NM_HOST) {
      if (length != 0) {
        std::fprintf(stderr, "a frame the device does not write has the length %d\n", length);
        return 2;
      }
      std::puts(kind == NM_DROP ? "drop" : "host");
      continue;
    }
    if (kind != NM_COPY && kind != NM_STATUS && kind != NM_PROGRESS) {
      std::fprintf(stderr, "unknown kind %d\n", kind);
      return 2;
    }
    if (kind != NM_COPY && (!inside(plan.id_off, plan.id_len, size) || !inside(plan.host_off, plan.host_len, size))) {
      std::fprintf(stderr, "a span lies outside a frame of %zu bytes\n", size);
      return 2;
    }
    const long long growth = static_cast<long long>(length) - static_cast<long long>(size);
    if (length < 5 || growth > NM_GROWTH_MAX || (kind == NM_COPY && growth != 0)) {
      std::fprintf(stderr, "a frame of %zu bytes becomes one of %d: more than NM_GROWTH_MAX\n", size, length);
      return 2;
    }
    std::fputs(kind == NM_COPY ? "copy " : kind == NM_STATUS ? "status " : "progress ", stdout);
    for (int rel = 0; rel < length; ++rel) std::printf("%02x", canon_byte(exact.get(), plan, rel));
    std::printf(" %lld\n", growth);
  }
  return 0;
}
