// The per-frame decision of `coalesce` (beholder_amd/coalesce.py key_of) and the hash of its keys,
// shared by the classify kernel (telemetry_coalesce.hip) and a host program for CPU tests
// (tests/native/coalesce_host.cpp): like telemetry_select.hpp, this header also compiles with a plain
// C++17 compiler (BH_FN), so the same code runs under ASan/UBSan on a CPU.
//
// classify<DIALECT>(buf, head, end, params, key) answers for the frame buf[head, end)
// (`u32 L | u8 topic | body`): DROP, KEEP, KEYED with `key` filled, or HOST where the device does
// not decide and the host asks coalesce.key_of instead. The rule for HOST is exactly the fold's
// (telemetry_fold.hip): a decoded id with a byte >= 0x80, whose identity is the decoded string; in
// the upb dialect also a non-ASCII host and a start-group. A frame whose answer does not depend on
// what it holds (a status frame under status=all with undecoded=keep, say) is not read at all, so
// it never goes to the host.
//
// The policy (coalesce.Policy) arrives flattened into CoalesceParams::flags.
#pragma once
#include "media_table.hpp"

namespace bh {

constexpr int CL_DROP = 0, CL_KEEP = 1, CL_KEYED = 2, CL_HOST = 3;

// CoalesceParams::flags
constexpr uint32_t CF_STATUS_ALL = 1;      // status=all: a decoded status frame is kept (else keyed)
constexpr uint32_t CF_PROGRESS_KEYED = 2;  // progress=last or per-status: a decoded progress frame is keyed
constexpr uint32_t CF_PER_STATUS = 4;      // progress=per-status: the status is part of a progress key
constexpr uint32_t CF_PROGRESS_ALL = 8;    // progress=all: kept; with none of the three: dropped
constexpr uint32_t CF_UNDECODED_KEEP = 16; // undecoded=keep: error and other frames are kept (else dropped)

struct CoalesceParams {
  uint64_t hash_mask;  // ANDed onto the hash before the home slot is taken (all ones in production)
  uint32_t flags;      // CF_* bits
  uint32_t slot_mask;  // group table slots - 1
};
static_assert(sizeof(CoalesceParams) == 16, "ops/gpu_coalesce.py CoalesceParams mirrors this layout");

// What makes two keyed frames the same key: topic, status, id length and id bytes. `status` is 0
// unless the policy makes it part of the key, so it is always compared.
struct CoalesceKey {
  uint64_t hash;
  int32_t id_off;  // absolute in buf
  int32_t id_len;
  int32_t status;
  uint32_t topic;  // 1 or 2
};

// The fold's hash of the id bytes (media_table.hpp hash64_bytes), then the topic and the status
// mixed in: ops/gpu_coalesce.py key_hash is the same. It only orders the probe. `high` is non-zero
// where an id byte is >= 0x80.
BH_FN uint64_t key_hash(const uint8_t* __restrict__ p, int n, uint32_t topic, int32_t status, uint32_t& high) {
  uint64_t h = hash64_bytes(p, n, high);
  h ^= (static_cast<uint64_t>(topic) << 32) | static_cast<uint32_t>(status);
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;
}

template <int DIALECT>
BH_FN int classify(const uint8_t* __restrict__ buf, const int head, const int end, const CoalesceParams& s,
                   CoalesceKey& key) {
  const uint32_t topic = buf[head + 4];
  const int undecoded = (s.flags & CF_UNDECODED_KEEP) ? CL_KEEP : CL_DROP;
  if (topic != 1 && topic != 2) return undecoded;
  const bool is_status = topic == 1;
  int decoded;
  if (is_status) decoded = (s.flags & CF_STATUS_ALL) ? CL_KEEP : CL_KEYED;
  else decoded = (s.flags & CF_PROGRESS_KEYED) ? CL_KEYED : (s.flags & CF_PROGRESS_ALL) ? CL_KEEP : CL_DROP;
  if (decoded == undecoded) return decoded;  // the frame's bytes do not matter
  Row r;
  const int start = head + 5;
  read_message<DIALECT, true>(buf, start, end, is_status, r);
  if (r.ok == OK_HOST) return CL_HOST;
  if (r.ok != OK_DECODED) return undecoded;
  const int32_t status = (!is_status && (s.flags & CF_PER_STATUS)) ? r.status : 0;
  uint32_t high;
  key.hash = key_hash(buf + r.id_off, r.id_len, topic, status, high);
  if (high) return CL_HOST;
  if (DIALECT == DIALECT_UPB && !is_status && has_high_byte(buf + r.host_off, r.host_len)) return CL_HOST;
  key.id_off = r.id_off;
  key.id_len = r.id_len;
  key.status = status;
  key.topic = topic;
  return decoded;
}

}  // namespace bh
