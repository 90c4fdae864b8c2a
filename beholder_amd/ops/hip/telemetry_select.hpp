// The per-frame predicate of `extract` (beholder_amd/extract.py) and the probe of its media table,
// shared by the mark kernel (telemetry_select.hip) and a host program for CPU tests
// (tests/native/select_host.cpp): like telemetry_readers.hpp, this header also compiles with a plain
// C++17 compiler (BH_FN), so the same code runs under ASan/UBSan on a CPU.
//
// decide<DIALECT>(buf, head, end, params, table, blob) answers for the frame buf[head, end)
// (`u32 L | u8 topic | body`): KEEP, DROP, or HOST where the device does not decide and the host
// asks extract.predicate instead. The rule for HOST is exactly the fold's (telemetry_fold.hip): a
// decoded id with a byte >= 0x80, whose identity is the decoded string; in the upb dialect also a
// non-ASCII host and a start-group. Query ids that are not ASCII never come here: a frame that could
// match one is a HOST frame by that rule.
//
// The selector (extract.Selector) arrives flattened into SelectParams; a field that was not given
// is all ones (topics, outcomes) or has its F_ bit clear (media, status).
//
// The media table is built on the host (ops/gpu_extract.py build_media_table) from the ASCII query
// ids: open addressing over `slot_mask + 1` entries, a power of two of at least twice the ids, so an
// empty entry always ends a probe chain. The hash and the home slot are media_table.hpp's. A hit is
// decided by length, hash and then the bytes, never by the hash alone.
#pragma once
#include "media_table.hpp"

namespace bh {

constexpr int DECIDE_DROP = 0, DECIDE_KEEP = 1, DECIDE_HOST = 2;

// bits of SelectParams::outcomes, in the order of extract.OUTCOMES
constexpr uint32_t OUT_DECODED = 1, OUT_ERROR = 2, OUT_OTHER = 4;

// SelectParams::flags
constexpr uint32_t F_MEDIA = 1;    // the media table takes part
constexpr uint32_t F_STATUS = 2;   // status_mask / F_UNKNOWN take part
constexpr uint32_t F_UNKNOWN = 4;  // a status that is no known enum number matches
constexpr uint32_t F_INVERT = 8;

struct SelectParams {
  uint64_t topics[4];    // bit t of the 256: topic byte t matches
  uint64_t status_mask;  // bit s: status s matches (0-63)
  uint64_t known_mask;   // bit s: s is a number of TelemetryStatusEntry
  uint64_t hash_mask;    // ANDed onto the hash before the home slot is taken (all ones in production)
  uint32_t outcomes;     // OUT_* bits
  uint32_t flags;        // F_* bits
  uint32_t slot_mask;    // table entries - 1
  uint32_t reserved;
};
static_assert(sizeof(SelectParams) == 72, "ops/gpu_extract.py SelectParams mirrors this layout");

struct MediaEntry {
  uint64_t hash;
  int32_t off;  // into the blob of id bytes
  int32_t len;  // < 0: the entry is empty
};
static_assert(sizeof(MediaEntry) == 16, "ops/gpu_extract.py builds the table as 16-byte entries");

// Is the id p[0, n) with this hash in the table? Ends at the first empty entry.
BH_FN bool table_has(const MediaEntry* __restrict__ table, const uint8_t* __restrict__ blob, const SelectParams& s,
                     const uint8_t* __restrict__ p, int n, uint64_t hash) {
  uint32_t slot = home_slot(hash, s.hash_mask, s.slot_mask);
  for (;;) {
    const MediaEntry e = table[slot];
    if (e.len < 0) return false;
    if (e.len == n && e.hash == hash && bytes_equal(blob + e.off, p, n)) return true;
    slot = (slot + 1) & s.slot_mask;
  }
}

template <int DIALECT>
BH_FN int decide(const uint8_t* __restrict__ buf, const int head, const int end, const SelectParams& s,
                 const MediaEntry* __restrict__ table, const uint8_t* __restrict__ blob) {
  const uint32_t topic = buf[head + 4];
  const bool invert = (s.flags & F_INVERT) != 0;
  Row r;
  uint32_t outcome = OUT_OTHER;
  uint64_t hash = 0;
  if (topic == 1 || topic == 2) {
    const bool is_status = topic == 1;
    const int start = head + 5;
    read_message<DIALECT, true>(buf, start, end, is_status, r);
    if (r.ok == OK_HOST) return DECIDE_HOST;
    if (r.ok == OK_DECODED) {
      uint32_t high;
      hash = hash64_bytes(buf + r.id_off, r.id_len, high);
      if (high) return DECIDE_HOST;
      if (DIALECT == DIALECT_UPB && !is_status && has_high_byte(buf + r.host_off, r.host_len)) return DECIDE_HOST;
      outcome = OUT_DECODED;
    } else {
      outcome = OUT_ERROR;
    }
  }
  bool match = ((s.topics[topic >> 6] >> (topic & 63u)) & 1ull) != 0 && (s.outcomes & outcome) != 0;
  if (match && (s.flags & (F_MEDIA | F_STATUS))) match = outcome == OUT_DECODED;
  if (match && (s.flags & F_STATUS)) {
    const uint32_t st = static_cast<uint32_t>(r.status);
    const bool in_range = st < 64u;
    const bool listed = in_range && ((s.status_mask >> (st & 63u)) & 1ull) != 0;
    const bool known = in_range && ((s.known_mask >> (st & 63u)) & 1ull) != 0;
    match = listed || ((s.flags & F_UNKNOWN) != 0 && !known);
  }
  if (match && (s.flags & F_MEDIA)) match = table_has(table, blob, s, buf + r.id_off, r.id_len, hash);
  return match != invert ? DECIDE_KEEP : DECIDE_DROP;
}

}  // namespace bh
