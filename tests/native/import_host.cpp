// The per-line code of the gfx950 import kernels (beholder_amd/ops/hip/telemetry_import.hpp),
// compiled for the host and run over NDJSON text. Built by tests/test_hip_import_host.py with
// -fsanitize=address,undefined: every line is read from a heap block of exactly its own size and
// every frame is written into a heap block of exactly its length, so a read one byte past a line or a
// write one byte past a frame is a sanitizer report here, not a fault on a GPU.
//
//   import_host_asan TEXT
//
// TEXT holds rows, one per line; a `\n` is added where it does not end in one, as the upload does.
// The first line of stdout is `starts` and the line starts, found as the two split kernels find them:
// newline_mask per lane of 16 bytes, a count per tile of 4096, a running sum over the tiles, then a rank
// per newline. One line per input line follows: `blank`, `host`, or `b64|status|progress FRAME` with the
// frame in hex. Every frame is built twice: by write_frame, one byte after the other, and piecewise as
// the emit kernel builds it: frame_byte for every position outside a string whose text has escapes,
// and such a string in pieces of 64 text bytes, each "lane" taking one byte, with the masks a ballot
// would give. The program fails where the two differ, where either disagrees with frame_len or the
// plan's out_len, or where a span leaves the line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_import.hpp"

using namespace bh;

static bool inside(int off, int len, size_t size) {
  return len >= 0 && off >= 0 && size_t(off) + size_t(len) <= size;
}

// The split: im_count, the scan and im_starts of telemetry_import.hip with loops for the blocks and lanes.
static std::vector<int32_t> split(const uint8_t* buf, int64_t size) {
  const int64_t tiles = (size + SPLIT_TILE_BYTES - 1) / SPLIT_TILE_BYTES;
  std::vector<int64_t> before(size_t(tiles) + 1, 0);
  for (int64_t tile = 0; tile < tiles; ++tile) {
    int count = 0;
    for (int lane = 0; lane < 256; ++lane)
      count += __builtin_popcount(newline_mask(buf, size, tile * SPLIT_TILE_BYTES + lane * SPLIT_LANE_BYTES));
    before[size_t(tile) + 1] = before[size_t(tile)] + count;
  }
  const int64_t n_lines = before[size_t(tiles)];
  std::vector<int32_t> starts(size_t(n_lines) + 1, -1);
  starts[0] = 0;
  for (int64_t tile = 0; tile < tiles; ++tile) {
    int64_t rank = before[size_t(tile)];
    for (int lane = 0; lane < 256; ++lane) {
      const int64_t at = tile * SPLIT_TILE_BYTES + lane * SPLIT_LANE_BYTES;
      for (uint32_t mask = newline_mask(buf, size, at); mask; mask &= mask - 1) {
        const int k = __builtin_ctz(mask);
        if (rank < n_lines) starts[size_t(rank) + 1] = static_cast<int32_t>(at + k + 1);
        ++rank;
      }
    }
  }
  return starts;
}

// unescaped_bytes of telemetry_import.hip with a loop over the 64 lanes; returns the bytes written.
static int unescaped_piecewise(const uint8_t* buf, int off, int text, int len, uint8_t* out) {
  Pieces pieces;
  int cursor = 0;
  for (int piece = 0; piece < text; piece += 64) {
    uint64_t backslashes = 0, us = 0, live = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const int k = piece + lane;
      if (k >= text) continue;
      live |= 1ull << lane;
      if (buf[off + k] == '\\') backslashes |= 1ull << lane;
      if (buf[off + k] == 'u') us |= 1ull << lane;
    }
    const uint64_t begins = pieces.next(backslashes, us, live);
    for (int lane = 0; lane < 64; ++lane) {
      const int place = cursor + __builtin_popcountll(begins & ((1ull << lane) - 1));
      if (((begins >> lane) & 1) && place < len) out[place] = static_cast<uint8_t>(unit_byte(buf + off, piece + lane, text));
    }
    cursor += __builtin_popcountll(begins);
  }
  return cursor;
}

static void plain_piecewise(const uint8_t* buf, const FramePlan& plan, uint8_t* out, int from, int to) {
  for (int lane = 0; lane < 64; ++lane)
    for (int b = from + lane; b < to; b += 64) out[b] = static_cast<uint8_t>(frame_byte(buf, plan, b));
}

// im_emit's body for one line.
static bool frame_piecewise(const uint8_t* buf, const FramePlan& plan, uint8_t* out) {
  int at = 0;
  if (plan.kind != IM_B64 && (plan.id_text != plan.id_len || plan.host_text != plan.host_len)) {
    int32_t id_start, host_start;
    string_starts(plan, id_start, host_start);
    if (plan.id_text != plan.id_len) {
      plain_piecewise(buf, plan, out, at, id_start);
      if (unescaped_piecewise(buf, plan.id_off, plan.id_text, plan.id_len, out + id_start) != plan.id_len) return false;
      at = id_start + plan.id_len;
    }
    if (plan.host_text != plan.host_len) {
      plain_piecewise(buf, plan, out, at, host_start);
      if (unescaped_piecewise(buf, plan.host_off, plan.host_text, plan.host_len, out + host_start) != plan.host_len)
        return false;
      at = host_start + plan.host_len;
    }
  }
  plain_piecewise(buf, plan, out, at, plan.out_len);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s TEXT\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (!data.empty() && data.back() != '\n') data.push_back('\n');
  if (data.size() >= (1u << 31)) {
    std::fprintf(stderr, "text too large for int32 offsets\n");
    return 2;
  }
  const size_t size = data.size();
  const std::unique_ptr<uint8_t[]> text(new uint8_t[size ? size : 1]);  // exactly the text: a read past it is a report
  if (size) std::memcpy(text.get(), data.data(), size);
  const std::vector<int32_t> starts = split(text.get(), static_cast<int64_t>(size));
  std::fputs("starts", stdout);
  for (const int32_t s : starts) std::printf(" %d", s);
  std::putchar('\n');
  for (size_t m = 0; m + 1 < starts.size(); ++m) {
    if (starts[m] < 0 || starts[m + 1] <= starts[m] || size_t(starts[m + 1]) > size) {
      std::fprintf(stderr, "line %zu: the starts %d and %d are no line\n", m, starts[m], starts[m + 1]);
      return 2;
    }
    const size_t length = size_t(starts[m + 1] - 1 - starts[m]);  // without its newline
    const std::unique_ptr<uint8_t[]> exact(new uint8_t[length ? length : 1]);
    if (length) std::memcpy(exact.get(), text.get() + starts[m], length);
    FramePlan plan;
    const int kind = import_classify(exact.get(), 0, int(length), plan);
    if (kind != plan.kind) {
      std::fprintf(stderr, "import_classify returns %d and writes kind %d\n", kind, plan.kind);
      return 2;
    }
    const int32_t out_len = frame_len(plan);
    if (out_len != plan.out_len) {
      std::fprintf(stderr, "frame_len is %d and the plan's out_len %d\n", out_len, plan.out_len);
      return 2;
    }
    if (kind == IM_BLANK || kind == IM_HOST) {
      if (out_len != 0) {
        std::fprintf(stderr, "a line the device does not write has the length %d\n", out_len);
        return 2;
      }
      std::puts(kind == IM_BLANK ? "blank" : "host");
      continue;
    }
    if (kind != IM_B64 && kind != IM_STATUS && kind != IM_PROGRESS) {
      std::fprintf(stderr, "unknown kind %d\n", kind);
      return 2;
    }
    if (!inside(plan.id_off, plan.id_text, length) || !inside(plan.host_off, plan.host_text, length) ||
        plan.id_len > plan.id_text || plan.host_len > plan.host_text || out_len < 5 || size_t(out_len) + 15 > length) {
      std::fprintf(stderr, "line %zu: a span lies outside a line of %zu bytes, or the frame is no shorter\n", m, length);
      return 2;
    }
    const std::unique_ptr<uint8_t[]> whole(new uint8_t[size_t(out_len)]), pieces(new uint8_t[size_t(out_len)]);
    std::memset(pieces.get(), 0xee, size_t(out_len));
    const long long written = write_frame(exact.get(), plan, whole.get());
    if (written != out_len) {
      std::fprintf(stderr, "write_frame writes %lld bytes of a frame of %d\n", written, out_len);
      return 2;
    }
    if (!frame_piecewise(exact.get(), plan, pieces.get())) {
      std::fprintf(stderr, "line %zu: a string's pieces do not add up to its decoded length\n", m);
      return 2;
    }
    if (std::memcmp(whole.get(), pieces.get(), size_t(out_len)) != 0) {
      std::fprintf(stderr, "line %zu: the frame in pieces differs from write_frame's\n", m);
      return 2;
    }
    std::fputs(kind == IM_B64 ? "b64 " : kind == IM_STATUS ? "status " : "progress ", stdout);
    for (int32_t k = 0; k < out_len; ++k) std::printf("%02x", whole[size_t(k)]);
    std::putchar('\n');
  }
  return 0;
}
