// The per-frame code of `thin` (beholder_amd/thin.py mark_of), shared by the classify kernel
// (telemetry_thin.hip) and a host program for CPU tests (tests/native/thin_host.cpp): like
// telemetry_transitions.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the
// same code runs under ASan/UBSan on a CPU.
//
// thin_classify<DIALECT>(buf, head, end, step, ev, mark) answers for the frame buf[head, end)
// (`u32 L | u8 topic | body`): TH_SKIP for a frame of another topic than 2, which is not read at all;
// TH_ERROR where the CPU codec raises; TH_HOST where the device does not decide and the host asks
// thin.mark_of instead; TH_EVENT for a progress event, with its id span, the fold's hash of the id
// and its status in `ev`, and its mark word in `mark`. The rule for TH_HOST is the coalesce's for a
// progress frame: a decoded id with a byte >= 0x80, whose identity is the decoded string; in the upb
// dialect also a non-ASCII host (upb raises where it is no UTF-8) and a start-group.
//
// The row is the transitions' StatusEvent and TH_* are TR_*, so the claim kernel of
// telemetry_transitions.hip runs over the rows unchanged.
//
// The mark word is uint32(status) << 32 | uint32(bucket), bucket = floor(progress / step) in int32:
// two events of one media repeat each other iff their words are equal. The host string takes no part.
#pragma once
#include "telemetry_transitions.hpp"

namespace bh {

constexpr int TH_SKIP = TR_SKIP, TH_ERROR = TR_ERROR, TH_HOST = TR_HOST, TH_EVENT = TR_EVENT;

// Python's progress // step for step >= 1. The quotient of the truncating division lies in
// [INT32_MIN, INT32_MAX] (the one overflow, INT32_MIN / -1, needs a negative step), and where a
// remainder pulls it down by one, step >= 2 and so the quotient is above -2^30.
BH_FN int32_t floor_div(int32_t progress, int32_t step) {
  const int32_t q = progress / step;
  return (progress % step) < 0 ? q - 1 : q;
}

BH_FN uint64_t mark_word(int32_t status, int32_t bucket) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(status)) << 32) | static_cast<uint32_t>(bucket);
}

template <int DIALECT>
BH_FN int thin_classify(const uint8_t* __restrict__ buf, const int head, const int end, const int32_t step,
                        StatusEvent& ev, uint64_t& mark) {
  ev = StatusEvent{0, 0, 0, 0, TH_SKIP};
  mark = 0;
  if (buf[head + 4] != 2) return TH_SKIP;
  Row r;
  const int start = head + 5;
  read_message<DIALECT, true>(buf, start, end, false, r);
  int kind = r.ok == OK_HOST ? TH_HOST : r.ok == OK_DECODED ? TH_EVENT : TH_ERROR;
  if (kind == TH_EVENT) {
    uint32_t high;
    const uint64_t hash = hash64_bytes(buf + r.id_off, r.id_len, high);
    if (high || (DIALECT == DIALECT_UPB && has_high_byte(buf + r.host_off, r.host_len))) {
      kind = TH_HOST;
    } else {
      ev.hash = hash;
      ev.id_off = r.id_off;
      ev.id_len = r.id_len;
      ev.status = r.status;
      mark = mark_word(r.status, floor_div(r.progress, step));
    }
  }
  ev.kind = kind;
  return kind;
}

}  // namespace bh
