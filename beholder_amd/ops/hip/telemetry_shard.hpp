// The per-frame decision of `shard` (beholder_amd/shard.py route_of), shared by the route kernel
// (telemetry_shard.hip) and a host program for CPU tests (tests/native/shard_host.cpp): like
// telemetry_select.hpp and telemetry_coalesce.hpp, this header also compiles with a plain C++17
// compiler (BH_FN), so the same code runs under ASan/UBSan on a CPU.
//
// route<DIALECT>(buf, head, end, params) answers for the frame buf[head, end)
// (`u32 L | u8 topic | body`): a shard number in [0, shards), ROUTE_DROP, or ROUTE_HOST where the
// device does not decide and the host asks shard.route_of instead. The rule for ROUTE_HOST is exactly
// telemetry_coalesce.hpp's, which is the fold's: a decoded id with a byte >= 0x80, whose identity is
// the decoded string; in the upb dialect also a non-ASCII host and a start-group. A frame whose
// answer does not depend on what it holds (another topic; every frame where one shard takes the
// undecoded ones too) is not read at all, so it never goes to the host.
//
// The shard of a decoded frame is the high half of the fold's hash of its id bytes (hash64_bytes of
// media_table.hpp), scaled to [0, shards) by one 32 x 32 -> 64 bit multiply and a shift:
// shard.shard_of is the same.
#pragma once
#include "telemetry_select.hpp"

namespace bh {

constexpr int ROUTE_DROP = -1, ROUTE_HOST = -2;
constexpr uint32_t MAX_SHARDS = 256;

// ShardParams::flags
constexpr uint32_t SF_UNDECODED_FIRST = 1;  // undecoded=first: error and other frames go to shard 0 (else dropped)

struct ShardParams {
  uint32_t shards;  // 1..MAX_SHARDS
  uint32_t flags;   // SF_* bits
};
static_assert(sizeof(ShardParams) == 8, "ops/gpu_shard.py ShardParams mirrors this layout");

BH_FN int shard_of_hash(uint64_t hash, uint32_t shards) {
  return static_cast<int>((static_cast<uint64_t>(static_cast<uint32_t>(hash >> 32)) * shards) >> 32);
}

template <int DIALECT>
BH_FN int route(const uint8_t* __restrict__ buf, const int head, const int end, const ShardParams& s) {
  const uint32_t topic = buf[head + 4];
  const int undecoded = (s.flags & SF_UNDECODED_FIRST) ? 0 : ROUTE_DROP;
  if (topic != 1 && topic != 2) return undecoded;
  if (s.shards == 1 && undecoded == 0) return 0;  // the frame's bytes do not matter
  const bool is_status = topic == 1;
  Row r;
  const int start = head + 5;
  read_message<DIALECT, true>(buf, start, end, is_status, r);
  if (r.ok == OK_HOST) return ROUTE_HOST;
  if (r.ok != OK_DECODED) return undecoded;
  uint32_t high;
  const uint64_t hash = hash64_bytes(buf + r.id_off, r.id_len, high);
  if (high) return ROUTE_HOST;
  if (DIALECT == DIALECT_UPB && !is_status && has_high_byte(buf + r.host_off, r.host_len)) return ROUTE_HOST;
  return shard_of_hash(hash, s.shards);
}

}  // namespace bh
