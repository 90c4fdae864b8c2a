// The per-frame code of the gfx950 export kernels (beholder_amd/ops/hip/telemetry_export.hpp),
// compiled for the host and run over a framed stream. Built by tests/test_hip_export_host.py with
// -fsanitize=address,undefined: every frame is read from a heap block of exactly its own size and
// every row is written into a heap block of exactly its length, so a read one byte past a frame or a
// write one byte past a row is a sanitizer report here, not a fault on a GPU.
//
//   export_host_asan upb|protobufjs STREAM keep|drop BASE
//
// STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py); frame k has the index
// BASE + k. One line per frame goes to stdout: `drop`, `host`, or `b64|status|progress ROW` with the
// row in hex. Every row is built twice: by write_row, one byte after the other, and piecewise as the
// emit kernel builds it: row_byte for every position outside a string that has escapes, and such a
// string in pieces of 64 input bytes, each "lane" taking one byte, with the widths and offsets
// computed per piece. The program fails where the two differ, where either disagrees with row_len or
// the plan's row_len, or where a span leaves the frame.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_export.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, bool, uint64_t, RowPlan&);

static bool inside(int off, int len, size_t size) {
  return len >= 0 && (len == 0 || (off >= 5 && size_t(off) + size_t(len) <= size));
}

// escaped_bytes of telemetry_export.hip with a loop over the 64 lanes; returns the bytes written.
static int escaped_piecewise(const uint8_t* buf, int off, int len, uint8_t* out) {
  int cursor = 0;
  for (int piece = 0; piece < len; piece += 64) {
    int width[64], before[64], total = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const int k = piece + lane;
      width[lane] = k < len ? esc_width(buf[off + k]) : 0;
      before[lane] = total;
      total += width[lane];
    }
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < width[lane]; ++j)
        out[cursor + before[lane] + j] = static_cast<uint8_t>(esc_byte(buf[off + piece + lane], j));
    cursor += total;
  }
  return cursor;
}

static void plain_piecewise(const uint8_t* buf, const RowPlan& plan, uint64_t index, uint8_t* out, int from, int to) {
  for (int lane = 0; lane < 64; ++lane)
    for (int b = from + lane; b < to; b += 64) out[b] = static_cast<uint8_t>(row_byte(buf, plan, index, b));
}

// ex_emit's body for one frame.
static bool row_piecewise(const uint8_t* buf, const RowPlan& plan, uint64_t index, uint8_t* out) {
  int at = 0;
  if (plan.kind != EX_B64 && (plan.id_esc != plan.id_len || plan.host_esc != plan.host_len)) {
    int32_t id_start, host_start;
    string_starts(plan, index, id_start, host_start);
    if (plan.id_esc != plan.id_len) {
      plain_piecewise(buf, plan, index, out, at, id_start);
      if (escaped_piecewise(buf, plan.id_off, plan.id_len, out + id_start) != plan.id_esc) return false;
      at = id_start + plan.id_esc;
    }
    if (plan.host_esc != plan.host_len) {
      plain_piecewise(buf, plan, index, out, at, host_start);
      if (escaped_piecewise(buf, plan.host_off, plan.host_len, out + host_start) != plan.host_esc) return false;
      at = host_start + plan.host_esc;
    }
  }
  plain_piecewise(buf, plan, index, out, at, plan.row_len);
  return true;
}

int main(int argc, char** argv) {
  Classify classify_frame = nullptr;
  if (argc == 5 && std::string(argv[1]) == "upb") classify_frame = export_classify<DIALECT_UPB>;
  if (argc == 5 && std::string(argv[1]) == "protobufjs") classify_frame = export_classify<DIALECT_PROTOBUFJS>;
  const std::string undecoded = argc == 5 ? argv[3] : "";
  if (!classify_frame || (undecoded != "keep" && undecoded != "drop")) {
    std::fprintf(stderr, "usage: %s upb|protobufjs STREAM keep|drop BASE\n", argv[0]);
    return 2;
  }
  const uint64_t base = std::strtoull(argv[4], nullptr, 10);
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
  uint64_t index = base;
  for (size_t i = 0; i < n; ++index) {
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
    RowPlan plan;
    const int kind = classify_frame(exact.get(), 0, int(size), undecoded == "drop", index, plan);
    if (kind != plan.kind) {
      std::fprintf(stderr, "export_classify returns %d and writes kind %d\n", kind, plan.kind);
      return 2;
    }
    const long long length = row_len(plan, index);
    if (length != plan.row_len) {
      std::fprintf(stderr, "row_len is %lld and the plan's row_len %d\n", length, plan.row_len);
      return 2;
    }
    if (kind == EX_DROP || kind == EX_HOST) {
      if (length != 0) {
        std::fprintf(stderr, "a frame the device does not write has the length %lld\n", length);
        return 2;
      }
      std::puts(kind == EX_DROP ? "drop" : "host");
      continue;
    }
    if (kind != EX_B64 && kind != EX_STATUS && kind != EX_PROGRESS) {
      std::fprintf(stderr, "unknown kind %d\n", kind);
      return 2;
    }
    if (!inside(plan.id_off, plan.id_len, size) || !inside(plan.host_off, plan.host_len, size)) {
      std::fprintf(stderr, "a span lies outside a frame of %zu bytes\n", size);
      return 2;
    }
    const std::unique_ptr<uint8_t[]> whole(new uint8_t[size_t(length)]), pieces(new uint8_t[size_t(length)]);
    std::memset(pieces.get(), 0xee, size_t(length));
    const long long written = write_row(exact.get(), plan, index, whole.get());
    if (written != length) {
      std::fprintf(stderr, "write_row writes %lld bytes of a row of %lld\n", written, length);
      return 2;
    }
    if (!row_piecewise(exact.get(), plan, index, pieces.get())) {
      std::fprintf(stderr, "a string's pieces do not add up to its escaped length\n");
      return 2;
    }
    if (std::memcmp(whole.get(), pieces.get(), size_t(length)) != 0) {
      std::fprintf(stderr, "frame %llu: the row in pieces differs from write_row's\n",
                   static_cast<unsigned long long>(index));
      return 2;
    }
    std::fputs(kind == EX_B64 ? "b64 " : kind == EX_STATUS ? "status " : "progress ", stdout);
    for (long long k = 0; k < length; ++k) std::printf("%02x", whole[size_t(k)]);
    std::putchar('\n');
  }
  return 0;
}
