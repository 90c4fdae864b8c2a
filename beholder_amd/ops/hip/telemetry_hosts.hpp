// The per-frame code of `hosts` (beholder_amd/hosts.py), shared by the classify kernel
// (telemetry_hosts.hip) and a host program for CPU tests (tests/native/hosts_host.cpp): like
// telemetry_thin.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same code
// runs under ASan/UBSan on a CPU.
//
// hosts_classify<DIALECT>(buf, head, end, media, worker, progress) answers for the frame
// buf[head, end) (`u32 L | u8 topic | body`): HO_SKIP for a frame of another topic than 2, which is not
// read at all; HO_ERROR where the CPU codec raises; HO_HOST where the device does not decide and the
// CPU decodes instead; HO_EVENT for a progress event. An event gets two rows of the transitions'
// StatusEvent layout, both with its status: `media` keyed by the span of its id and the fold's hash
// of it, `worker` keyed by the span of its host string (field 4, the worker's name) and the same hash
// of that; and its progress.
//
// The rule for HO_HOST, in both dialects: a byte >= 0x80 in the id or in the worker string (the
// identity of either is the decoded string, and only the service's codec knows what U+FFFD makes of
// it; upb raises where it is no UTF-8), and upb's start-group.
//
// HO_* are TR_*, so the claim kernel of telemetry_transitions.hip runs over either row unchanged.
#pragma once
#include "telemetry_transitions.hpp"

namespace bh {

constexpr int HO_SKIP = TR_SKIP, HO_ERROR = TR_ERROR, HO_HOST = TR_HOST, HO_EVENT = TR_EVENT;

// The words of one worker's row of counters, in ops/gpu_hosts.py as in the walk kernel: the media it
// starts, the handovers it takes and loses, its rewinds, then its events per status class. Its stints
// are starts + taken and its events the sum of the classes: neither has a word.
constexpr uint32_t W_STARTS = 0, W_TAKEN = 1, W_LOST = 2, W_REWINDS = 3, W_CLASS = 4;
constexpr uint32_t WORKER_WORDS = W_CLASS + CLASSES;

// The key of an event in the pair table: its media number above its worker number.
BH_FN uint64_t pair_key(uint32_t media, uint32_t worker) { return (static_cast<uint64_t>(media) << 32) | worker; }

template <int DIALECT>
BH_FN int hosts_classify(const uint8_t* __restrict__ buf, const int head, const int end, StatusEvent& media,
                         StatusEvent& worker, int32_t& progress) {
  media = StatusEvent{0, 0, 0, 0, HO_SKIP};
  worker = media;
  progress = 0;
  if (buf[head + 4] != 2) return HO_SKIP;
  Row r;
  const int start = head + 5;
  read_message<DIALECT, true>(buf, start, end, false, r);
  int kind = r.ok == OK_HOST ? HO_HOST : r.ok == OK_DECODED ? HO_EVENT : HO_ERROR;
  if (kind == HO_EVENT) {
    uint32_t id_high, worker_high;
    const uint64_t id_hash = hash64_bytes(buf + r.id_off, r.id_len, id_high);
    const uint64_t worker_hash = hash64_bytes(buf + r.host_off, r.host_len, worker_high);
    if (id_high | worker_high) {
      kind = HO_HOST;
    } else {
      media.hash = id_hash;
      media.id_off = r.id_off;
      media.id_len = r.id_len;
      media.status = r.status;
      worker.hash = worker_hash;
      worker.id_off = r.host_off;
      worker.id_len = r.host_len;
      worker.status = r.status;
      progress = r.progress;
    }
  }
  media.kind = kind;
  worker.kind = kind;
  return kind;
}

}  // namespace bh
