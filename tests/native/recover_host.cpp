// The per-offset code of the gfx950 recover kernels (beholder_amd/ops/hip/telemetry_recover.hpp),
// compiled for the host and run over a buffer. Built by tests/test_hip_recover_host.py with
// -fsanitize=address,undefined: the buffer is a heap block of exactly its own size, so a read one byte
// past it is a sanitizer report here, not a fault on a GPU.
//
//   recover_host_asan upb|protobufjs BUFFER MAX_FRAME FINAL RESYNC ANSWERS
//
// FINAL and RESYNC are 0 or 1. ANSWERS is a text file of offsets, one per line: the offsets among
// those flagged for the host (RC_ASK_HOST) that the host found to be anchors; the others it found not
// to be. Output, one line each:
//   c P FLAGS END   for every offset P in [0, n): candidate()'s flag byte and end, before the answers
//   s P SUCC        for every P in [0, n]: successor() over the tables with the answers written back
//   r P             for every P in [0, n] that the doubling rounds reach, in a plain serial rendition:
//                   the kernels' rounds, one offset after the other
// The program fails where an end or a successor leaves [0, n].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "telemetry_recover.hpp"

using namespace bh;

using Candidate = int (*)(const uint8_t*, int, int, int, int, int&);

int main(int argc, char** argv) {
  Candidate candidate_at = nullptr;
  if (argc == 7 && std::string(argv[1]) == "upb") candidate_at = candidate<DIALECT_UPB>;
  if (argc == 7 && std::string(argv[1]) == "protobufjs") candidate_at = candidate<DIALECT_PROTOBUFJS>;
  if (!candidate_at) {
    std::fprintf(stderr, "usage: %s upb|protobufjs BUFFER MAX_FRAME FINAL RESYNC ANSWERS\n", argv[0]);
    return 2;
  }
  const int max_frame = std::atoi(argv[3]);
  const bool final_part = std::atoi(argv[4]) != 0, resync = std::atoi(argv[5]) != 0;
  std::ifstream in(argv[2], std::ios::binary);
  std::ifstream answers(argv[6]);
  if (!in || !answers || max_frame < 1 || max_frame > (16 << 20)) {
    std::fprintf(stderr, "cannot read %s or %s, or MAX_FRAME is outside 1..16 MiB\n", argv[2], argv[6]);
    return 2;
  }
  const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (data.size() > size_t(RC_LIMIT)) {
    std::fprintf(stderr, "more than RC_LIMIT bytes\n");
    return 2;
  }
  const int n = int(data.size());
  const std::unique_ptr<uint8_t[]> exact(new uint8_t[data.size()]);
  if (n) std::memcpy(exact.get(), data.data(), data.size());
  const uint8_t* buf = exact.get();
  const long long horizon = 2LL * (4 + max_frame);
  const int decided = final_part ? n : int(n - horizon + 1 > 0 ? n - horizon + 1 : 0);

  std::vector<uint8_t> flags(size_t(n) + 1, 0);
  std::vector<int32_t> end(size_t(n) + 1, n);
  for (int p = 0; p < n; ++p) {
    int e = -1;
    const int f = candidate_at(buf, n, decided, max_frame, p, e);
    if (e < 0 || e > n || ((f & RC_WF) && e < p + 5) || (!(f & RC_WF) && (e != n || f != 0))) {
      std::fprintf(stderr, "offset %d: flags %d and end %d do not go together\n", p, f, e);
      return 2;
    }
    flags[size_t(p)] = uint8_t(f);
    end[size_t(p)] = e;
    std::printf("c %d %d %d\n", p, f, e);
  }
  for (int p = 0; p < n; ++p)
    if (flags[size_t(p)] & RC_ASK_HOST) flags[size_t(p)] = RC_WF;
  for (long long q; answers >> q;) {
    if (q < 0 || q >= n || !(flags[size_t(q)] & RC_WF)) {
      std::fprintf(stderr, "answer %lld is no offset that was asked\n", q);
      return 2;
    }
    flags[size_t(q)] = RC_WF | RC_ANCHOR;
  }

  std::vector<int32_t> next(size_t(n) + 1, n);
  for (int p = n - 1; p >= 0; --p) next[size_t(p)] = (flags[size_t(p)] & RC_ANCHOR) ? p : next[size_t(p) + 1];
  std::vector<int32_t> jump(size_t(n) + 1, n), spare(size_t(n) + 1, n);
  for (int p = 0; p <= n; ++p) {
    const int s = p == n ? n : successor(flags.data(), end.data(), n, decided, p, next[size_t(p) + 1]);
    if (s < 0 || s > n || (p < decided && s <= p)) {
      std::fprintf(stderr, "offset %d: the successor %d is not ahead of it inside the buffer\n", p, s);
      return 2;
    }
    jump[size_t(p)] = s;
    std::printf("s %d %d\n", p, s);
  }

  std::vector<uint8_t> reach(size_t(n) + 1, 0);
  reach[size_t(resync ? next[0] : 0)] = 1;
  for (int round = doubling_rounds(n); round > 0; --round) {
    for (int p = 0; p <= n; ++p) {
      const int j = jump[size_t(p)];
      if (reach[size_t(p)]) reach[size_t(j)] = 1;
      spare[size_t(p)] = jump[size_t(j)];
    }
    jump.swap(spare);
  }
  for (int p = 0; p <= n; ++p)
    if (reach[size_t(p)]) std::printf("r %d\n", p);
  return 0;
}
