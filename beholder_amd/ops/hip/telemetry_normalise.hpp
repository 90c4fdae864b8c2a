// The per-frame code of `normalise` (beholder_amd/normalise.py canon_of), shared by the kernels
// (telemetry_normalise.hip) and a host program for CPU tests (tests/native/normalise_host.cpp): like
// telemetry_thin.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same code
// runs under ASan/UBSan on a CPU.
//
// norm_classify<DIALECT>(buf, head, end, drop, plan) reads the frame buf[head, end)
// (`u32 L | u8 topic | body`) by its topic (read_message, upb in its STRICT form) and fills one Plan:
//   NM_COPY      the frame stays as it is: another topic, or a decode error, where undecoded frames
//                are kept. id_off is the frame's start and out_len its length.
//   NM_DROP      the same frames where undecoded frames are dropped. out_len is 0.
//   NM_HOST      the device does not write this frame and the host asks normalise.canon_of instead: a
//                decoded frame whose id span or host span holds a byte >= 0x80, in either dialect
//                (under upb the host decides whether it is UTF-8, under protobufjs the re-encoding
//                may substitute U+FFFD); under upb also a start-group (OK_HOST). out_len is 0.
//   NM_STATUS    a decoded status event: id span and status; progress and host_len are 0.
//   NM_PROGRESS  a decoded progress event: id span, status, progress and host span.
// For the last two out_len is the length of the canonical frame, which canon_byte writes out.
//
// The canonical frame of a decoded event is the service's own encoding of what it decoded:
//   u32 out_len - 4 | u8 topic
//   mediaId   0x0a varint(id_len) bytes             where id_len > 0
//   status    0x10 varint(int64(status))            where status != 0: a negative one takes 10 bytes
//   progress  0x18 varint(int64(progress))          where progress != 0
//   host      0x22 varint(host_len) bytes           where host_len > 0
// Tag and varint bytes are computed from the plan; string bytes are copied from the input span.
#pragma once
#include "media_table.hpp"

namespace bh {

constexpr int NM_COPY = 0, NM_DROP = 1, NM_HOST = 2, NM_STATUS = 3, NM_PROGRESS = 4;

struct Plan {
  int32_t id_off, id_len;  // absolute in buf; NM_COPY: the frame's start, and unused
  int32_t status, progress;
  int32_t host_off, host_len;
  int32_t kind;            // NM_*
  int32_t out_len;         // the output frame's length, header included; 0 where the device writes none
};
static_assert(sizeof(Plan) == 32, "ops/gpu_normalise.py views the plans as (n, 8) int32");

// The most bytes by which a canonical frame exceeds the input frame it was decoded from.
//
// Header and topic are 5 bytes on both sides. Every canonical field is written from the last
// occurrence of that field in the input body, and the occurrences of different fields are disjoint
// byte ranges of the body, so it is enough to bound each field against its own occurrence.
//  * A string of n >= 1 bytes takes 1 + len(varint(n)) + n canonical bytes. Its occurrence holds a
//    tag of at least 1 byte, a length varint whose value is at least n (upb: exactly n; protobufjs
//    clamps the span to the message end, so the value may be larger, and an overlong varint is
//    longer), hence at least len(varint(n)) bytes, and the n bytes themselves: no growth. An empty
//    string is not written at all.
//  * An int32 x != 0 takes 1 + len(varint(int64(x))) canonical bytes. Its occurrence holds a tag of at
//    least 1 byte and a varint of k bytes that are all inside the body (protobufjs reads bytes past
//    the end as continuation bytes, and then fails). For x > 0 the varint carries at most 7k value
//    bits, so x < 2^(7k) and the canonical varint has at most k bytes: no growth. For x < 0 bit 31 of
//    the value is set, which takes k >= 5, and the canonical varint has 10 bytes: 5 more at most.
// A progress event has two such fields and a status event one, so the bound is 10, and the frame
// `02 | 10 ff ff ff ff 0f | 18 ff ff ff ff 0f` reaches it. Frames left to the host are not covered:
// U+FFFD takes three bytes where the input had one.
constexpr int NM_GROWTH_MAX = 10;

BH_FN int varint_len(uint64_t v) { return (63 - __builtin_clzll(v | 1ull)) / 7 + 1; }

// Byte k of the varint of v, which has n bytes.
BH_FN uint32_t varint_byte(uint64_t v, int k, int n) {
  return (static_cast<uint32_t>(v >> (7 * k)) & 0x7fu) | (k + 1 < n ? 0x80u : 0u);
}

BH_FN uint64_t sign_extended(int32_t x) { return static_cast<uint64_t>(static_cast<int64_t>(x)); }

BH_FN int string_field_len(int32_t n) { return n > 0 ? 1 + varint_len(static_cast<uint64_t>(n)) + n : 0; }
BH_FN int int_field_len(int32_t x) { return x != 0 ? 1 + varint_len(sign_extended(x)) : 0; }

// The length of the output frame of `plan`, from its fields alone (out_len holds the same).
BH_FN int canon_len(const Plan& plan) {
  if (plan.kind == NM_COPY) return plan.out_len;
  if (plan.kind != NM_STATUS && plan.kind != NM_PROGRESS) return 0;
  return 5 + string_field_len(plan.id_len) + int_field_len(plan.status) + int_field_len(plan.progress) +
         string_field_len(plan.host_len);
}

// Byte `rel` of the output frame of `plan`, 0 <= rel < canon_len(plan); the kind is NM_COPY, NM_STATUS
// or NM_PROGRESS. Reads buf only inside the plan's spans.
BH_FN uint32_t canon_byte(const uint8_t* __restrict__ buf, const Plan& plan, int rel) {
  if (plan.kind == NM_COPY) return buf[plan.id_off + rel];
  if (rel < 4) return (static_cast<uint32_t>(plan.out_len - 4) >> (8 * rel)) & 0xffu;
  if (rel == 4) return plan.kind == NM_STATUS ? 1u : 2u;
  // Where fields 2, 3 and 4 start; field 1 starts at 5. A field that is not written has no bytes and
  // starts where the next one does, so counting the starts at or below rel skips it. The starts
  // depend on the plan alone: in the emit kernel they are scalars, and what is left per lane is
  // selects, one shift and at most one load.
  const int a2 = 5 + string_field_len(plan.id_len);
  const int a3 = a2 + int_field_len(plan.status);
  const int a4 = a3 + int_field_len(plan.progress);
  const int field = 1 + (rel >= a2) + (rel >= a3) + (rel >= a4);
  const int k = rel - (field == 1 ? 5 : field == 2 ? a2 : field == 3 ? a3 : a4);  // inside the field
  const bool is_string = field == 1 || field == 4;
  const uint64_t v = field == 1   ? static_cast<uint64_t>(plan.id_len)
                     : field == 2 ? sign_extended(plan.status)
                     : field == 3 ? sign_extended(plan.progress)
                                  : static_cast<uint64_t>(plan.host_len);
  const int head = varint_len(v);
  if (k == 0) return static_cast<uint32_t>(field << 3 | (is_string ? 2 : 0));
  if (k <= head || !is_string) return varint_byte(v, k - 1, head);  // a number ends with its varint
  return buf[(field == 1 ? plan.id_off : plan.host_off) + (k - 1 - head)];
}

template <int DIALECT>
BH_FN int norm_classify(const uint8_t* __restrict__ buf, const int head, const int end, const bool drop, Plan& plan) {
  const uint32_t topic = buf[head + 4];
  const int undecoded = drop ? NM_DROP : NM_COPY;
  plan = Plan{head, 0, 0, 0, 0, 0, undecoded, drop ? 0 : end - head};
  if (topic != 1 && topic != 2) return undecoded;
  const bool is_status = topic == 1;
  Row r;
  const int start = head + 5;
  read_message<DIALECT, true>(buf, start, end, is_status, r);
  if (r.ok == OK_ERROR) return undecoded;
  int kind = is_status ? NM_STATUS : NM_PROGRESS;
  if (r.ok == OK_HOST || has_high_byte(buf + r.id_off, r.id_len) ||
      (!is_status && has_high_byte(buf + r.host_off, r.host_len)))
    kind = NM_HOST;
  if (kind == NM_HOST) {
    plan = Plan{head, 0, 0, 0, 0, 0, NM_HOST, 0};
    return kind;
  }
  plan.id_off = r.id_off;
  plan.id_len = r.id_len;
  plan.status = r.status;
  plan.progress = is_status ? 0 : r.progress;
  plan.host_off = is_status ? 0 : r.host_off;
  plan.host_len = is_status ? 0 : r.host_len;
  plan.kind = kind;
  plan.out_len = canon_len(plan);
  return kind;
}

}  // namespace bh
