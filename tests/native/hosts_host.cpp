// The per-frame code of the gfx950 hosts kernels (beholder_amd/ops/hip/telemetry_hosts.hpp), compiled
// for the host and run over a framed stream. Built by tests/test_hip_hosts_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size, so a
// read one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   hosts_host_asan upb|protobufjs STREAM
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py). One line per frame goes to
// stdout: skip for a frame that is not read, error, host where the device leaves the frame to the
// CPU, or `event ID WORKER STATUS PROGRESS IDHASH WORKERHASH` with the bytes of the id and of the
// worker string in hex (`-` for an empty one).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_hosts.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, StatusEvent&, StatusEvent&, int32_t&);

static bool inside(const StatusEvent& ev, size_t size) {
  return ev.id_len >= 0 && (ev.id_len == 0 || (ev.id_off >= 5 && size_t(ev.id_off) + size_t(ev.id_len) <= size));
}

static void hex(const uint8_t* frame, const StatusEvent& ev) {
  if (ev.id_len == 0) std::fputs("-", stdout);
  for (int k = 0; k < ev.id_len; ++k) std::printf("%02x", frame[size_t(ev.id_off) + size_t(k)]);
}

int main(int argc, char** argv) {
  Classify classify_frame = nullptr;
  if (argc == 3 && std::string(argv[1]) == "upb") classify_frame = hosts_classify<DIALECT_UPB>;
  if (argc == 3 && std::string(argv[1]) == "protobufjs") classify_frame = hosts_classify<DIALECT_PROTOBUFJS>;
  if (!classify_frame) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM\n", argv[0]);
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
    StatusEvent media, worker;
    int32_t progress = 0;
    const int kind = classify_frame(exact.get(), 0, int(size), media, worker, progress);
    if (kind != media.kind || kind != worker.kind) {
      std::fprintf(stderr, "hosts_classify returns %d and writes kinds %d and %d\n", kind, media.kind, worker.kind);
      return 2;
    }
    if (kind != HO_EVENT && (progress != 0 || media.hash != 0 || worker.hash != 0 || media.id_len != 0 || worker.id_len != 0)) {
      std::fprintf(stderr, "a frame that is no event has a row\n");
      return 2;
    }
    if (kind == HO_SKIP) std::puts("skip");
    else if (kind == HO_ERROR) std::puts("error");
    else if (kind == HO_HOST) std::puts("host");
    else {
      if (!inside(media, size) || !inside(worker, size)) {
        std::fprintf(stderr, "a span [%d, +%d) or [%d, +%d) outside a frame of %zu bytes\n", media.id_off, media.id_len,
                     worker.id_off, worker.id_len, size);
        return 2;
      }
      if (media.status != worker.status) {
        std::fprintf(stderr, "the two rows' statuses differ\n");
        return 2;
      }
      std::fputs("event ", stdout);
      hex(exact.get(), media);
      std::fputs(" ", stdout);
      hex(exact.get(), worker);
      std::printf(" %d %d %llu %llu\n", media.status, progress, static_cast<unsigned long long>(media.hash),
                  static_cast<unsigned long long>(worker.hash));
    }
  }
  return 0;
}
