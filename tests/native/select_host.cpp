// The predicate and media-table probe of the gfx950 select kernels
// (beholder_amd/ops/hip/telemetry_select.hpp), compiled for the host and run over a framed stream.
// Built by tests/test_hip_select_host.py with -fsanitize=address,undefined: every frame is read from a
// heap block of exactly its own size, and so are the table and its id bytes, so a read one byte past
// a frame, a table entry or an id is a sanitizer report here, not a fault on a GPU.
//
//   select_host_asan upb|protobufjs STREAM PARAMS TABLE BLOB
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); PARAMS the 72 bytes of a
// SelectParams; TABLE the MediaEntry array (params.slot_mask + 1 entries) and BLOB its id bytes, as
// ops/gpu_extract.py build_media_table lays them out. One line per frame goes to stdout:
// keep, drop, or host where the device leaves the frame to the host.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_select.hpp"

using namespace bh;

using Decide = int (*)(const uint8_t*, int, int, const SelectParams&, const MediaEntry*, const uint8_t*);

static bool slurp(const char* path, std::vector<uint8_t>& out) {
  std::ifstream in(path, std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", path);
    return false;
  }
  out.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
  return true;
}

int main(int argc, char** argv) {
  Decide decide_frame = nullptr;
  if (argc == 6 && std::string(argv[1]) == "upb") decide_frame = decide<DIALECT_UPB>;
  if (argc == 6 && std::string(argv[1]) == "protobufjs") decide_frame = decide<DIALECT_PROTOBUFJS>;
  if (!decide_frame) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM PARAMS TABLE BLOB\n", argv[0]);
    return 2;
  }
  std::vector<uint8_t> data, raw_params, raw_table, raw_blob;
  if (!slurp(argv[2], data) || !slurp(argv[3], raw_params) || !slurp(argv[4], raw_table) || !slurp(argv[5], raw_blob))
    return 2;
  SelectParams params;
  if (raw_params.size() != sizeof(params)) {
    std::fprintf(stderr, "PARAMS holds %zu bytes, a SelectParams %zu\n", raw_params.size(), sizeof(params));
    return 2;
  }
  std::memcpy(&params, raw_params.data(), sizeof(params));
  const size_t slots = size_t(params.slot_mask) + 1;
  if ((slots & (slots - 1)) != 0 || raw_table.size() != slots * sizeof(MediaEntry)) {
    std::fprintf(stderr, "TABLE holds %zu bytes, not %zu entries\n", raw_table.size(), slots);
    return 2;
  }
  if (data.size() >= (1u << 31)) {
    std::fprintf(stderr, "stream too large for int32 offsets\n");
    return 2;
  }
  // exact-size blocks: new[] of MediaEntry is aligned for its uint64
  const std::unique_ptr<MediaEntry[]> table(new MediaEntry[slots]);
  std::memcpy(table.get(), raw_table.data(), raw_table.size());
  const std::unique_ptr<uint8_t[]> blob(new uint8_t[raw_blob.size()]);
  if (!raw_blob.empty()) std::memcpy(blob.get(), raw_blob.data(), raw_blob.size());
  for (size_t k = 0; k < slots; ++k) {
    const MediaEntry& e = table[k];
    if (e.len >= 0 && (e.off < 0 || size_t(e.off) + size_t(e.len) > raw_blob.size())) {
      std::fprintf(stderr, "entry %zu points outside BLOB\n", k);
      return 2;
    }
  }
  static const char* const words[] = {"drop", "keep", "host"};
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
    std::puts(words[decide_frame(exact.get(), 0, int(size), params, table.get(), blob.get())]);
  }
  return 0;
}
