// The per-frame code of the gfx950 stages kernels (beholder_amd/ops/hip/telemetry_stages.hpp), compiled
// for the host and run over a framed stream. Built by tests/test_hip_stages_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   stages_host_asan upb|protobufjs STREAM
//   stages_host_asan buckets
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py). One line per frame goes to
// stdout: skip for a frame that is not read, error, host where the device leaves the frame to the
// CPU, `status ID STATUS IDHASH` or `progress ID STATUS PROGRESS IDHASH` with the bytes of the id in
// hex (`-` for an empty one). `buckets` reads `COUNT LAST` pairs from stdin and prints bucket_of.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_stages.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, StatusEvent&, uint64_t&);

static bool inside(const StatusEvent& ev, size_t size) {
  return ev.id_len >= 0 && (ev.id_len == 0 || (ev.id_off >= 5 && size_t(ev.id_off) + size_t(ev.id_len) <= size));
}

static void hex(const uint8_t* frame, const StatusEvent& ev) {
  if (ev.id_len == 0) std::fputs("-", stdout);
  for (int k = 0; k < ev.id_len; ++k) std::printf("%02x", frame[size_t(ev.id_off) + size_t(k)]);
}

static int buckets() {
  long long count = 0, last = 0;
  while (std::scanf("%lld %lld", &count, &last) == 2) {
    if (count < 0 || count > 0xffffffffll || last < INT32_MIN || last > INT32_MAX) return 2;
    std::printf("%u\n", bucket_of(static_cast<uint32_t>(count), static_cast<int32_t>(last)));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "buckets") return buckets();
  Classify classify_frame = nullptr;
  if (argc == 3 && std::string(argv[1]) == "upb") classify_frame = stages_classify<DIALECT_UPB>;
  if (argc == 3 && std::string(argv[1]) == "protobufjs") classify_frame = stages_classify<DIALECT_PROTOBUFJS>;
  if (!classify_frame) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM | buckets\n", argv[0]);
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
    uint64_t aux = 0;
    const int kind = classify_frame(exact.get(), 0, int(size), ev, aux);
    if (kind != ev.kind) {
      std::fprintf(stderr, "stages_classify returns %d and writes kind %d\n", kind, ev.kind);
      return 2;
    }
    if (kind != ST_EVENT && (aux != 0 || ev.id_len != 0)) {
      std::fprintf(stderr, "a frame that is no event has a row\n");
      return 2;
    }
    if (kind == ST_SKIP) std::puts("skip");
    else if (kind == ST_ERROR) std::puts("error");
    else if (kind == ST_HOST) std::puts("host");
    else {
      if (!inside(ev, size) || (aux >> 33) != 0 || (aux_is_status(aux) && aux_progress(aux) != 0) ||
          aux_is_status(aux) != (exact[4] == 1)) {
        std::fprintf(stderr, "a span [%d, +%d) outside a frame of %zu bytes, or an aux word %llx of no event\n",
                     ev.id_off, ev.id_len, size, static_cast<unsigned long long>(aux));
        return 2;
      }
      std::fputs(aux_is_status(aux) ? "status " : "progress ", stdout);
      hex(exact.get(), ev);
      if (aux_is_status(aux)) std::printf(" %d %llu\n", ev.status, static_cast<unsigned long long>(ev.hash));
      else std::printf(" %d %d %llu\n", ev.status, aux_progress(aux), static_cast<unsigned long long>(ev.hash));
    }
  }
  return 0;
}
