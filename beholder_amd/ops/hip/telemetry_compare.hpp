// The per-frame and per-position code of `compare` (beholder_amd/compare.py): what kind of frame
// this is and its row, and, over the frames sorted by content, where a content's run and its B half
// start and whether a position is matched. Shared by the kernels (telemetry_compare.hip) and a host
// program for CPU tests (tests/native/compare_host.cpp): like telemetry_dedupe.hpp, this header also
// compiles with a plain C++17 compiler (BH_FN), so the same code runs under ASan/UBSan on a CPU.
//
// Two captures lie in one joined stream, A's n_a frames first; the side of frame m is m >= n_a. A
// frame's content is the dedupe's (its topic byte and body), so dedupe_kind and content_hash are
// used as they are: DK_KEEP is "skipped" here, DK_HOST a content above DEDUPE_DEVICE_MAX that the
// host pairs, DK_ROW a frame that takes part on the device. Its row has the transitions' layout,
// {hash, id_off = content start, id_len = content length, status = side, kind = TR_EVENT}, which is
// what lets the transitions' claim, compact and sort run over it unchanged: equal contents get one
// dense number (the key), and the sort leaves every content's frames adjacent and in joined order,
// A's occurrences in stream order and then B's. vals[p] is frame << 32 | side.
//
// The pairing rule over a run [run_start, run_end) whose B half starts at side_start: a position's
// rank is its distance from its side's start, and it is matched iff its rank is below
// min(side_start - run_start, run_end - side_start). Its partner is the position of the same rank
// on the other side.
#pragma once
#include "telemetry_dedupe.hpp"
#include "telemetry_transitions.hpp"

namespace bh {

constexpr int32_t SIDE_A = 0, SIDE_B = 1;

// The kind of the frame buf[head, end) (DK_* of telemetry_dedupe.hpp) and, for DK_ROW, its row.
// Every other kind gets a TR_SKIP row, which the claim passes over.
BH_FN int cmp_row(const uint8_t* __restrict__ buf, const int head, const int end, const int32_t side,
                  const DedupeParams& s, StatusEvent& ev) {
  ev = StatusEvent{0, 0, 0, 0, TR_SKIP};
  const int kind = dedupe_kind(buf, head, end, s);
  if (kind == DK_ROW) {
    ev.id_off = head + 4;
    ev.id_len = end - head - 4;  // 1..DEDUPE_DEVICE_MAX
    ev.hash = content_hash<true>(buf + ev.id_off, ev.id_len);
    ev.status = side;
    ev.kind = TR_EVENT;
  }
  return kind;
}

BH_FN int32_t cmp_side_of(const uint64_t val) { return static_cast<int32_t>(val & 1ull); }
BH_FN uint32_t cmp_frame_of(const uint64_t val) { return static_cast<uint32_t>(val >> 32); }

// What sorted position p writes of its content's bounds: each of run_start[key], side_start[key]
// and run_end[key] has exactly one writer among the positions, so the stores are plain.
//   run_start   the run's first position
//   side_start  the first position of the run that holds a B frame, or the run's end if it has none
//   run_end     one past the run's last position
// `groups` bounds the key: a position whose key is not below it writes nothing.
BH_FN void cmp_bounds_at(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals, const int events,
                         const uint32_t groups, const int p, int32_t* __restrict__ run_start,
                         int32_t* __restrict__ side_start, int32_t* __restrict__ run_end) {
  const uint32_t key = keys[p];
  if (key >= groups) return;  // never: a key is a claimed slot's rank
  const int32_t side = cmp_side_of(vals[p]);
  const bool first = p == 0 || keys[p - 1] != key;
  const bool last = p + 1 >= events || keys[p + 1] != key;
  if (first) run_start[key] = p;
  if (side == SIDE_B && (first || cmp_side_of(vals[p - 1]) == SIDE_A)) side_start[key] = p;
  if (last) {
    run_end[key] = p + 1;
    if (side == SIDE_A) side_start[key] = p + 1;  // a run without a B frame
  }
}

struct CmpVerdict {
  bool matched;
  int32_t side;
  int32_t partner;  // the partner's sorted position where matched, else -1
  bool run_head;    // this is its run's first position: it counts the run
  bool in_a, in_b;  // for a run head: the content occurs in A, in B
};

// The verdict for sorted position p from the bounds an earlier launch wrote. Bounds that do not
// enclose p (never: cmp_bounds_at wrote them for these very keys) give an unmatched verdict, so a
// partner is always a position in [0, events).
BH_FN CmpVerdict cmp_verdict(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals, const int events,
                             const uint32_t groups, const int p, const int32_t* __restrict__ run_start,
                             const int32_t* __restrict__ side_start, const int32_t* __restrict__ run_end) {
  CmpVerdict v{false, cmp_side_of(vals[p]), -1, false, false, false};
  const uint32_t key = keys[p];
  if (key >= groups) return v;
  const int32_t rs = run_start[key], ss = side_start[key], re = run_end[key];
  if (!(0 <= rs && rs <= ss && ss <= re && re <= events && rs <= p && p < re)) return v;
  const int32_t in_a = ss - rs, in_b = re - ss;
  const int32_t pairs = in_a < in_b ? in_a : in_b;
  const int32_t rank = v.side == SIDE_B ? p - ss : p - rs;
  v.run_head = p == rs;
  v.in_a = in_a > 0;
  v.in_b = in_b > 0;
  if (rank >= 0 && rank < pairs) {
    v.matched = true;
    v.partner = v.side == SIDE_B ? rs + rank : ss + rank;
  }
  return v;
}

}  // namespace bh
