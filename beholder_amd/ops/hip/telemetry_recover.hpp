// The per-offset code of `recover` (beholder_amd/recover.py rules_of), shared by the kernels
// (telemetry_recover.hip) and a host program for CPU tests (tests/native/recover_host.cpp): like
// telemetry_normalise.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same
// code runs under ASan/UBSan on a CPU.
//
// Over a buffer of n bytes (n <= 2^28, so every offset and every end fits an int32):
//   well_framed(p)  p + 4 <= n, the little-endian L at p has 1 <= L <= max_frame, end(p) = p + 4 + L <= n
//   anchor(q)       well_framed(q), the topic byte is 1 or 2, the body decodes (read_message, upb in its
//                   STRICT form), the decoded mediaId is not empty, and end(q) == n or well_framed(end(q))
//
// candidate<DIALECT>(buf, n, decided, max_frame, p, end) gives the flag byte of offset p and end(p):
//   RC_WF        well_framed(p); end is end(p). Without it end is n.
//   RC_ANCHOR    anchor(p), decided on the device.
//   RC_ASK_HOST  everything but the decode is settled and holds, and the decode is the host's: under
//                upb a mediaId span (or, in a progress message, a host span) with a byte >= 0x80,
//                which the codec accepts only as UTF-8, or a start-group (OK_HOST). The host writes
//                RC_ANCHOR or nothing in its place. Under protobufjs nothing is asked: a string is
//                never an error, and it is empty only where its clamped span is empty.
// An offset p >= decided carries no flag at all: a part that is not the last decides nothing there
// (recover.decided_end), and in the last part decided == n.
//
// successor() is the walk's one step over these tables; the kernels fuse it into the scan's last
// launch and the host program calls it as it is.
#pragma once
#include "media_table.hpp"

namespace bh {

constexpr int RC_WF = 1, RC_ANCHOR = 2, RC_ASK_HOST = 4;

// The most bytes one call takes: ops/gpu_recover.py LIMIT.
constexpr int RC_LIMIT = 1 << 28;

// Whether a header at p that holds L fits: p + 4 <= n is the caller's. L <= max_frame <= 2^24 comes
// first, so the sum stays far below 2^31.
BH_FN bool header_fits(uint32_t L, int p, int n, int max_frame) {
  return L >= 1u && L <= static_cast<uint32_t>(max_frame) && p + 4 + static_cast<int>(L) <= n;
}

// The little-endian word at buf[i, i + 4), byte by byte: i has no alignment.
BH_FN uint32_t load_le32(const uint8_t* __restrict__ buf, int i) {
  return static_cast<uint32_t>(buf[i]) | static_cast<uint32_t>(buf[i + 1]) << 8 |
         static_cast<uint32_t>(buf[i + 2]) << 16 | static_cast<uint32_t>(buf[i + 3]) << 24;
}

BH_FN bool well_framed(const uint8_t* __restrict__ buf, int n, int max_frame, int p) {
  return p + 4 <= n && header_fits(load_le32(buf, p), p, n, max_frame);
}

// The flags of a decided offset p with p + 4 <= n whose header holds L and, where L >= 1 fits, the
// topic byte `topic`: the caller has read both (the kernel from LDS). Reads buf only inside
// [p + 5, end) and the four header bytes at end.
template <int DIALECT>
BH_FN int candidate_of_header(const uint8_t* __restrict__ buf, int n, int max_frame, int p, uint32_t L, uint32_t topic,
                              int& end) {
  end = n;
  if (!header_fits(L, p, n, max_frame)) return 0;  // almost every offset leaves here
  end = p + 4 + static_cast<int>(L);
  if (topic != 1u && topic != 2u) return RC_WF;
  if (end != n && !well_framed(buf, n, max_frame, end)) return RC_WF;
  const bool is_status = topic == 1u;
  Row r;
  const int start = p + 5;
  read_message<DIALECT, true>(buf, start, end, is_status, r);
  if (r.ok == OK_ERROR) return RC_WF;
  if constexpr (DIALECT == DIALECT_PROTOBUFJS) {
    return r.id_len > 0 ? RC_WF | RC_ANCHOR : RC_WF;
  } else {
    if (r.ok == OK_HOST) return RC_WF | RC_ASK_HOST;
    if (r.id_len <= 0) return RC_WF;  // empty if it decodes, no anchor if it does not
    if (has_high_byte(buf + r.id_off, r.id_len) || (!is_status && has_high_byte(buf + r.host_off, r.host_len)))
      return RC_WF | RC_ASK_HOST;
    return RC_WF | RC_ANCHOR;
  }
}

// The same from the buffer alone.
template <int DIALECT>
BH_FN int candidate(const uint8_t* __restrict__ buf, int n, int decided, int max_frame, int p, int& end) {
  end = n;
  if (p >= decided || p + 4 > n) return 0;
  const uint32_t L = load_le32(buf, p);
  const uint32_t topic = header_fits(L, p, n, max_frame) ? buf[p + 4] : 0u;  // L >= 1: p + 4 < n
  return candidate_of_header<DIALECT>(buf, n, max_frame, p, L, topic, end);
}

// Where the walk goes from p, 0 <= p <= n: to end(p) from a well-framed p; from any other decided p to
// the end of the first anchor behind it, `next_after` = next[p + 1] being that anchor's offset or n;
// to n from an offset that is not decided, from one with no anchor behind it, and from n itself.
BH_FN int successor(const uint8_t* __restrict__ flags, const int32_t* __restrict__ end, int n, int decided, int p,
                    int next_after) {
  if (p >= decided) return n;
  if (flags[p] & RC_WF) return end[p];
  return next_after < n ? end[next_after] : n;
}

// How many doubling rounds reach every node of a walk over n bytes: every hop between decided
// offsets advances at least 5 bytes (a frame holds 5; a gap ends behind an anchor's 5), so a walk has
// at most n / 5 + 1 decided nodes, and k rounds mark the first 2^k of them. The launcher's, so host
// code under hipcc too: constexpr.
constexpr int doubling_rounds(int n) {
  int rounds = 0;
  for (int v = n / 5 + 1; v > 0; v >>= 1) ++rounds;
  return rounds;
}

}  // namespace bh
