// The per-frame and per-position code of the gfx950 compare kernels
// (beholder_amd/ops/hip/telemetry_compare.hpp), compiled for the host and run over two framed
// streams. Built by tests/test_hip_compare_host.py with -fsanitize=address,undefined: every frame is
// read from a heap block of exactly its own size, and the bounds live in heap arrays of exactly
// `groups` words, so a read or write one element past either is a sanitizer report here, not a fault
// on a GPU.
//
//   compare_host_asan A B T0 T1 T2 T3
//
// A and B hold `u32 L | u8 topic | body` frames (transport/framing.py); T0-T3 are the decimal words
// of DedupeParams::topics (ops/gpu_compare.py params_of). The frames are joined, A's first. The
// program does by hand what the transitions' stages do on the device: equal contents get one dense
// number, and the rows are sorted by it with std::stable_sort, so a content's run holds A's frames
// in stream order and then B's. Then cmp_bounds_at and cmp_verdict run over every position. One
// line per joined frame goes to stdout:
//   skip                       its topic is not selected
//   host                       its content is above DEDUPE_DEVICE_MAX
//   only HASH                  it takes part and is unmatched
//   matched HASH PARTNER       it is matched with joined frame PARTNER
// and a last line `counts MATCHED DISTINCT_A DISTINCT_B COMMON` from the run heads.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_compare.hpp"

using namespace bh;

struct Frame {
  std::unique_ptr<uint8_t[]> bytes;  // exactly the frame
  int size;
};

static bool read_frames(const char* path, std::vector<Frame>& frames) {
  std::ifstream in(path, std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", path);
    return false;
  }
  const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (data.size() >= (1u << 31)) {
    std::fprintf(stderr, "stream too large for int32 offsets\n");
    return false;
  }
  const size_t n = data.size();
  for (size_t i = 0; i < n;) {
    uint32_t L = 0;
    if (n - i >= 4) std::memcpy(&L, &data[i], 4);  // little-endian hosts only, as the kernels' are
    if (L == 0 || n - i - 4 < L) {
      std::fprintf(stderr, "%s: truncated or empty frame at byte %zu\n", path, i);
      return false;
    }
    const size_t size = 4 + size_t(L);
    Frame f{std::unique_ptr<uint8_t[]>(new uint8_t[size]), int(size)};
    std::memcpy(f.bytes.get(), &data[i], size);
    frames.push_back(std::move(f));
    i += size;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s A B T0 T1 T2 T3\n", argv[0]);
    return 2;
  }
  std::vector<Frame> frames;
  if (!read_frames(argv[1], frames)) return 2;
  const size_t n_a = frames.size();
  if (!read_frames(argv[2], frames)) return 2;
  const size_t n = frames.size();
  DedupeParams params{};
  for (int k = 0; k < 4; ++k) params.topics[k] = std::strtoull(argv[3 + k], nullptr, 10);

  // classify: the kind and row of every joined frame, and the content numbers
  std::vector<int> kinds(n);
  std::vector<StatusEvent> rows(n);
  std::map<std::string, uint32_t> number;
  struct Event {
    uint32_t key;
    uint64_t val;
  };
  std::vector<Event> events;
  for (size_t m = 0; m < n; ++m) {
    const Frame& f = frames[m];
    const int32_t side = m >= n_a ? SIDE_B : SIDE_A;
    kinds[m] = cmp_row(f.bytes.get(), 0, f.size, side, params, rows[m]);
    if (kinds[m] != DK_ROW) {
      if (rows[m].kind != TR_SKIP) return 3;
      continue;
    }
    const StatusEvent& ev = rows[m];
    if (ev.kind != TR_EVENT || ev.id_off != 4 || ev.id_len != f.size - 4 || ev.status != side) return 3;
    const std::string content(reinterpret_cast<const char*>(f.bytes.get()) + ev.id_off, size_t(ev.id_len));
    const uint32_t key = number.emplace(content, uint32_t(number.size())).first->second;
    events.push_back({key, (uint64_t(m) << 32) | uint32_t(ev.status)});
  }
  std::stable_sort(events.begin(), events.end(), [](const Event& x, const Event& y) { return x.key < y.key; });
  const int count = int(events.size());
  const uint32_t groups = uint32_t(number.size());
  // heap arrays of exactly their sizes (a zero-sized one is never indexed)
  std::unique_ptr<uint32_t[]> keys(new uint32_t[size_t(count)]);
  std::unique_ptr<uint64_t[]> vals(new uint64_t[size_t(count)]);
  for (int p = 0; p < count; ++p) {
    keys[size_t(p)] = events[size_t(p)].key;
    vals[size_t(p)] = events[size_t(p)].val;
  }
  std::unique_ptr<int32_t[]> run_start(new int32_t[groups]), side_start(new int32_t[groups]);
  std::unique_ptr<int32_t[]> run_end(new int32_t[groups]);
  // unwritten bounds match nothing
  for (uint32_t g = 0; g < groups; ++g) run_start[g] = side_start[g] = run_end[g] = -1;
  for (int p = 0; p < count; ++p)
    cmp_bounds_at(keys.get(), vals.get(), count, groups, p, run_start.get(), side_start.get(), run_end.get());

  std::vector<long long> partner(n, -2);  // -2: no sorted position, -1: unmatched
  unsigned long matched = 0, distinct_a = 0, distinct_b = 0, common = 0;
  for (int p = 0; p < count; ++p) {
    const CmpVerdict v =
        cmp_verdict(keys.get(), vals.get(), count, groups, p, run_start.get(), side_start.get(), run_end.get());
    const uint32_t m = cmp_frame_of(vals[size_t(p)]);
    if (m >= n || v.side != (m >= n_a ? SIDE_B : SIDE_A)) return 3;
    if (v.matched && (v.partner < 0 || v.partner >= count)) return 3;
    partner[m] = v.matched ? (long long)cmp_frame_of(vals[size_t(v.partner)]) : -1;
    matched += v.matched && v.side == SIDE_A;
    distinct_a += v.run_head && v.in_a;
    distinct_b += v.run_head && v.in_b;
    common += v.run_head && v.in_a && v.in_b;
  }
  for (size_t m = 0; m < n; ++m) {
    if (kinds[m] == DK_KEEP) std::puts("skip");
    else if (kinds[m] == DK_HOST) std::puts("host");
    else if (partner[m] == -2) return 3;
    else if (partner[m] == -1) std::printf("only %016" PRIx64 "\n", rows[m].hash);
    else std::printf("matched %016" PRIx64 " %lld\n", rows[m].hash, partner[m]);
  }
  std::printf("counts %lu %lu %lu %lu\n", matched, distinct_a, distinct_b, common);
  return 0;
}
