// The per-frame code of `stages` (beholder_amd/stages.py), shared by the classify and settle kernels
// (telemetry_stages.hip) and a host program for CPU tests (tests/native/stages_host.cpp): like
// telemetry_hosts.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same code
// runs under ASan/UBSan on a CPU.
//
// stages_classify<DIALECT>(buf, head, end, ev, aux) answers for the frame buf[head, end)
// (`u32 L | u8 topic | body`). A topic-1 frame goes through the transitions' classify as it is, a
// topic-2 frame through the thin's thin_classify as it is (with step 1 the low half of its mark word
// is the progress itself), so the rules for ST_ERROR and ST_HOST are those two tools', frame by
// frame. Every other topic is ST_SKIP and is not read. An event gets the transitions' StatusEvent row
// and its aux word: the progress in the low half (0 for a status event) and AUX_STATUS above it for a
// status event. ST_* are TR_*, so the claim kernel of telemetry_transitions.hip runs over the rows of
// both topics unchanged.
//
// bucket_of(count, last) is the bucket of a stage of `count` progress events whose last reported
// `last`: comparisons and one division of a value in [0, 100), so no int32 overflows.
#pragma once
#include "telemetry_thin.hpp"

namespace bh {

constexpr int ST_SKIP = TR_SKIP, ST_ERROR = TR_ERROR, ST_HOST = TR_HOST, ST_EVENT = TR_EVENT;

constexpr uint64_t AUX_STATUS = 1ull << 32;  // set in the aux word of a status event

// The buckets, in ops/gpu_stages.py and beholder_amd/stages.py BUCKETS as in the settle kernel.
constexpr uint32_t B_NONE = 0, B_BELOW = 1, B_TENTHS = 2, B_FULL = 12, B_OVER = 13, BUCKETS = 14;

// The words of one media's row, in ops/gpu_stages.py as in the settle kernel: its run's bounds in the
// sorted arrays, its lead's count and last progress, 1 + the position of its open stage's status
// event (0: no status event) and the progress of its last event.
constexpr uint32_t M_START = 0, M_END = 1, M_LEAD = 2, M_LEAD_LAST = 3, M_OPEN = 4, M_LAST = 5, MEDIA_WORDS = 6;

BH_FN uint32_t bucket_of(uint32_t count, int32_t last) {
  if (count == 0) return B_NONE;
  if (last < 0) return B_BELOW;
  if (last < 100) return B_TENTHS + static_cast<uint32_t>(last) / 10u;
  return last == 100 ? B_FULL : B_OVER;
}

BH_FN bool aux_is_status(uint64_t aux) { return (aux & AUX_STATUS) != 0; }
BH_FN int32_t aux_progress(uint64_t aux) { return static_cast<int32_t>(static_cast<uint32_t>(aux & 0xffffffffull)); }

template <int DIALECT>
BH_FN int stages_classify(const uint8_t* __restrict__ buf, const int head, const int end, StatusEvent& ev,
                          uint64_t& aux) {
  aux = 0;
  const uint8_t topic = buf[head + 4];
  if (topic == 1) {
    const int kind = classify<DIALECT>(buf, head, end, ev);
    if (kind == ST_EVENT) aux = AUX_STATUS;
    return kind;
  }
  if (topic == 2) {
    uint64_t mark;
    const int kind = thin_classify<DIALECT>(buf, head, end, 1, ev, mark);
    if (kind == ST_EVENT) aux = mark & 0xffffffffull;  // floor_div(progress, 1)
    return kind;
  }
  ev = StatusEvent{0, 0, 0, 0, ST_SKIP};
  return ST_SKIP;
}

}  // namespace bh
