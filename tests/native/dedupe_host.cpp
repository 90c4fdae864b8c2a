// The per-frame code of the gfx950 dedupe kernels (beholder_amd/ops/hip/telemetry_dedupe.hpp),
// compiled for the host and run over a framed stream. Built by tests/test_hip_dedupe_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   dedupe_host_asan wide|bytes STREAM T0 T1 T2 T3 [I:J ...]
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); T0-T3 are the decimal words
// of DedupeParams::topics (ops/gpu_dedupe.py dedupe_params). One line per frame goes to stdout:
// `keep`, `host`, or `row` and the content's hash in hex. Then, for every pair I:J of frame indices,
// one line `I:J 1` where the contents of the two frames are equal bytes (the kernel's test: length,
// then hash, then bytes) and `I:J 0` where they are not.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_dedupe.hpp"

using namespace bh;

struct Frame {
  std::unique_ptr<uint8_t[]> bytes;  // exactly the frame
  int size;
};

template <bool WIDE>
int run(const std::vector<Frame>& frames, const DedupeParams& params, int argc, char** argv) {
  std::vector<uint64_t> hashes(frames.size(), 0);
  for (size_t m = 0; m < frames.size(); ++m) {
    const Frame& f = frames[m];
    const int kind = dedupe_kind(f.bytes.get(), 0, f.size, params);
    if (kind == DK_KEEP) std::puts("keep");
    else if (kind == DK_HOST) std::puts("host");
    else {
      hashes[m] = content_hash<WIDE>(f.bytes.get() + 4, f.size - 4);
      std::printf("row %016" PRIx64 "\n", hashes[m]);
    }
  }
  for (int k = 7; k < argc; ++k) {
    char* colon = nullptr;
    const unsigned long i = std::strtoul(argv[k], &colon, 10);
    if (*colon != ':') return 2;
    const unsigned long j = std::strtoul(colon + 1, nullptr, 10);
    if (i >= frames.size() || j >= frames.size()) return 2;
    const Frame &a = frames[i], &b = frames[j];
    const bool equal = a.size == b.size && hashes[i] == hashes[j] &&
                       content_equal<WIDE>(a.bytes.get() + 4, b.bytes.get() + 4, a.size - 4);
    std::printf("%lu:%lu %d\n", i, j, equal ? 1 : 0);
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string method = argc >= 7 ? argv[1] : "";
  if (method != "wide" && method != "bytes") {
    std::fprintf(stderr, "usage: %s wide|bytes STREAM T0 T1 T2 T3 [I:J ...]\n", argv[0]);
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
  DedupeParams params{};
  for (int k = 0; k < 4; ++k) params.topics[k] = std::strtoull(argv[3 + k], nullptr, 10);
  std::vector<Frame> frames;
  const size_t n = data.size();
  for (size_t i = 0; i < n;) {
    uint32_t L = 0;
    if (n - i >= 4) std::memcpy(&L, &data[i], 4);  // little-endian hosts only, as the kernels' are
    if (L == 0 || n - i - 4 < L) {
      std::fprintf(stderr, "truncated or empty frame at byte %zu\n", i);
      return 2;
    }
    const size_t size = 4 + size_t(L);
    Frame f{std::unique_ptr<uint8_t[]>(new uint8_t[size]), int(size)};
    std::memcpy(f.bytes.get(), &data[i], size);
    frames.push_back(std::move(f));
    i += size;
  }
  const int rc = method == "wide" ? run<true>(frames, params, argc, argv) : run<false>(frames, params, argc, argv);
  if (rc) std::fprintf(stderr, "a pair is I:J with both below the frame count\n");
  return rc;
}
