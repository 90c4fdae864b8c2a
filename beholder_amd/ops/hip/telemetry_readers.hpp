// Readers for the telemetry messages (models/proto/api.proto), shared by the batched decode
// (telemetry_decode.hip), the stream fold (telemetry_fold.hip) and a host program for CPU tests.
//
// read_message<DIALECT, STRICT> fills one Row:
//   {id_off, id_len, status, progress, host_off, host_len, ok, seen}
// (offsets absolute in buf; ok = OK_ERROR where the CPU codec raises DecodeError; seen has one
// SEEN_* bit per known field the message carried).
//
// The header also compiles for the host with a plain C++17 compiler (BH_FN below), so the same
// readers run under ASan/UBSan on a CPU: tests/native/readers_host.cpp.
//
// Readers are parameterised by message type:
//   MSG_PROGRESS  api.TelemetryProgress: mediaId=1, status=2, progress=3, host=4 known
//   MSG_STATUS    api.TelemetryStatus:   mediaId=1, status=2 known; 3 and 4 are unknown fields and
//                 go the way every unknown field of the dialect goes
//
// Two dialects, the same two the CPU codec has (ops/__init__.py DIALECTS); valid input decodes
// identically in both:
//
//  * DIALECT_PROTOBUFJS (the service's default, handlers.py `_dialect`): protobufjs 6.8.8's
//    BufferReader and generated decoder, rule for rule as ops/csrc/pbjs.hpp models them:
//      - the tag and every known field are read with Reader.uint32(): up to 5 bytes, a byte past
//        the end reads as `undefined` (0, continuation), a 5th byte with its continuation bit
//        skips 5 more bytes unchecked and fails only if that passes the end;
//      - a known field is read with its declared type whatever wire type its tag carries
//        (mediaId / host: string, status: enum, progress: int32, both `uint32() | 0`);
//      - strings are clamped to the message end (BufferReader.string), never an error;
//      - field number 0 and unknown fields are skipped with skipType(wt & 7): varints unbounded
//        but end-checked, 64/32-bit and length-delimited bounds-checked, groups skipped up to
//        the next end-group tag of any field (counted, not recursed), wire types 4/6/7 fail.
//  * DIALECT_UPB (google.protobuf's rules, the tooling oracle): last value wins, unknown fields
//    of wire types 0/1/2/5 are skipped, a known field with an unexpected wire type is skipped
//    like an unknown one, field 0, truncation or wire types 3/4/6/7 set ok = OK_ERROR. A tag is a
//    varint of up to 10 bytes and its field number is all of key >> 3, up to 61 bits: a number
//    past 32 bits is an unknown field whatever its low 32 bits say.
//    With STRICT the reader follows ops/csrc/wire.hpp to the letter where the plain one is
//    looser: a tag is a varint of at most 5 bytes whose value fits 32 bits, and a start-group
//    (which wire.hpp skips with a stack of field numbers) sets ok = OK_HOST: the caller hands
//    that message to the CPU codec instead of guessing. The batched decode keeps the plain
//    reader, its table is unchanged; the fold uses STRICT.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BH_FN __device__ __forceinline__
#define BH_UNROLL _Pragma("unroll")
#else
#define BH_FN inline
#define BH_UNROLL
#endif

namespace bh {

constexpr int DIALECT_UPB = 0;
constexpr int DIALECT_PROTOBUFJS = 1;

constexpr int MSG_PROGRESS = 0;
constexpr int MSG_STATUS = 1;

// Row::ok
constexpr int32_t OK_ERROR = 0;    // the CPU codec raises DecodeError
constexpr int32_t OK_DECODED = 1;
constexpr int32_t OK_HOST = 2;     // a STRICT upb read only: decode this one on the host

// Row::seen
constexpr int32_t SEEN_ID = 1, SEEN_STATUS = 2, SEEN_PROGRESS = 4, SEEN_HOST = 8;

// One row of the (n, 8) int32 table the decode kernel stores; ops/gpu_decode.py FIELDS names the
// same columns. A fresh Row is an empty message that decoded.
struct Row {
  int32_t id_off = 0, id_len = 0;
  int32_t status = 0, progress = 0;
  int32_t host_off = 0, host_len = 0;
  int32_t ok = OK_DECODED;
  int32_t seen = 0;
};
static_assert(sizeof(Row) == 32, "ops/gpu_decode.py views the table as (n, 8) int32");

// ---- upb ------------------------------------------------------------------------------------

BH_FN bool read_varint(const uint8_t* __restrict__ p, int end, int& i, uint64_t& v) {
  v = 0;
  BH_UNROLL
  for (int shift = 0; shift < 70; shift += 7) {
    if (i >= end) return false;
    const uint32_t b = p[i++];
    v |= static_cast<uint64_t>(b & 0x7fu) << shift;
    if (!(b & 0x80u)) return true;
  }
  return false;  // more than 10 bytes
}

// wire.hpp Reader::tag: at most 5 bytes, the value fits 32 bits
BH_FN bool read_tag_strict(const uint8_t* __restrict__ p, int end, int& i, uint64_t& v) {
  v = 0;
  BH_UNROLL
  for (int k = 0; k < 5; ++k) {
    if (i >= end) return false;
    const uint32_t b = p[i++];
    v |= static_cast<uint64_t>(b & 0x7fu) << (7 * k);
    if (!(b & 0x80u)) return v <= 0xffffffffull;
  }
  return false;
}

template <int MSG, bool STRICT>
BH_FN void decode_upb(const uint8_t* __restrict__ buf, int i, const int end, Row& r) {
  while (i < end) {
    uint64_t key;
    if (STRICT ? !read_tag_strict(buf, end, i, key) : !read_varint(buf, end, i, key)) { r.ok = OK_ERROR; return; }
    uint32_t field = static_cast<uint32_t>(key >> 3);
    const uint32_t wt = static_cast<uint32_t>(key & 7);
    // The field number is the whole key >> 3: 2^32 + 1 is an unknown field, not mediaId, and 2^32 is
    // not field 0. A STRICT key fits 32 bits already, so its code stays as it was.
    if constexpr (!STRICT) {
      if (key >> 35) field = 0xffffffffu;  // stands for every number past 32 bits: known to no message
    }
    if (field == 0) { r.ok = OK_ERROR; return; }
    if (wt == 0) {
      uint64_t v;
      if (!read_varint(buf, end, i, v)) { r.ok = OK_ERROR; return; }
      if (field == 2) { r.status = static_cast<int32_t>(v); r.seen |= SEEN_STATUS; }
      else if (MSG == MSG_PROGRESS && field == 3) {
        r.progress = static_cast<int32_t>(v);
        r.seen |= SEEN_PROGRESS;
      }
    } else if (wt == 2) {
      uint64_t len;
      if (!read_varint(buf, end, i, len) || len > static_cast<uint64_t>(end - i)) { r.ok = OK_ERROR; return; }
      if (field == 1) { r.id_off = i; r.id_len = static_cast<int>(len); r.seen |= SEEN_ID; }
      else if (MSG == MSG_PROGRESS && field == 4) {
        r.host_off = i;
        r.host_len = static_cast<int>(len);
        r.seen |= SEEN_HOST;
      }
      i += static_cast<int>(len);
    } else if (wt == 1) {
      if (end - i < 8) { r.ok = OK_ERROR; return; }
      i += 8;
    } else if (wt == 5) {
      if (end - i < 4) { r.ok = OK_ERROR; return; }
      i += 4;
    } else if (STRICT && wt == 3) {
      r.ok = OK_HOST;
      return;
    } else {
      r.ok = OK_ERROR;
      return;
    }
  }
}

// ---- protobufjs 6.8.8 -------------------------------------------------------------------------
// Positions are relative to the message start and may step past its end: Reader.uint32() reads
// `undefined` bytes before it reports the overrun, exactly as pbjs.hpp does. 32-bit arithmetic
// (messages are < 2^31 bytes, checked on the host) and an unchecked fast path while at least 5
// bytes remain keep the per-byte work at the upb kernel's level; only the last bytes of a
// message take the bounds-checked path.

struct PbjsReader {
  const uint8_t* __restrict__ p;  // message start
  int len;
  int pos;

  BH_FN int at(int i) const { return i < len ? int(p[i]) : -1; }

  // Reader.prototype.uint32
  BH_FN bool uint32(uint32_t& out) {
    if (pos + 5 <= len) {  // every byte it may read is inside the message
      uint32_t b = p[pos++];
      uint32_t v = b & 127u;
      if (b < 128u) { out = v; return true; }
      b = p[pos++]; v |= (b & 127u) << 7;
      if (b < 128u) { out = v; return true; }
      b = p[pos++]; v |= (b & 127u) << 14;
      if (b < 128u) { out = v; return true; }
      b = p[pos++]; v |= (b & 127u) << 21;
      if (b < 128u) { out = v; return true; }
      b = p[pos++]; v |= (b & 15u) << 28;
      if (b < 128u) { out = v; return true; }
      pos += 5;  // the 64-bit tail, unchecked byte by byte
      if (pos > len) { pos = len; return false; }
      out = v;
      return true;
    }
    uint32_t v = 0;
    BH_UNROLL
    for (int k = 0; k < 4; ++k) {
      const int b = at(pos);
      v |= uint32_t(b < 0 ? 0 : (b & 127)) << (7 * k);
      ++pos;
      if (b >= 0 && b < 128) { out = v; return true; }
    }
    const int b = at(pos);
    v |= uint32_t(b < 0 ? 0 : (b & 15)) << 28;
    ++pos;
    if (b >= 0 && b < 128) { out = v; return true; }
    pos += 5;
    if (pos > len) { pos = len; return false; }
    out = v;
    return true;
  }

  BH_FN bool skip_n(uint32_t n) {
    if (n > uint32_t(len - pos)) return false;  // pos <= len here
    pos += int(n);
    return true;
  }

  BH_FN bool skip_varint() {
    for (;;) {
      if (pos >= len) return false;
      if (!(p[pos++] & 128)) return true;
    }
  }

  // Reader.prototype.skipType(wireType), groups counted instead of recursed into
  BH_FN bool skip_type(uint32_t wt) {
    uint32_t depth = 0;
    for (;;) {
      switch (wt) {
        case 0: if (!skip_varint()) return false; break;
        case 1: if (!skip_n(8)) return false; break;
        case 2: {
          uint32_t n;
          if (!uint32(n) || !skip_n(n)) return false;
          break;
        }
        case 3: ++depth; break;
        case 5: if (!skip_n(4)) return false; break;
        case 4:
          if (depth > 0) { --depth; break; }
          return false;
        default: return false;
      }
      if (depth == 0) return true;
      uint32_t t;
      if (!uint32(t)) return false;
      wt = t & 7;
    }
  }

  // BufferReader.prototype.string: the byte range clamped to the end
  BH_FN bool string(int& off, int& n) {
    uint32_t L;
    if (!uint32(L)) return false;
    const int e = L < uint32_t(len - pos) ? pos + int(L) : len;  // pos <= len here
    off = pos;
    n = e - pos;
    pos = e;
    return true;
  }
};

template <int MSG>
BH_FN void decode_pbjs(const uint8_t* __restrict__ buf, const int start, const int end, Row& r) {
  PbjsReader rd{buf + start, end - start, 0};
  while (rd.pos < rd.len) {
    uint32_t t;
    if (!rd.uint32(t)) { r.ok = OK_ERROR; return; }
    const uint32_t field = t >> 3;
    if (field == 1 || (MSG == MSG_PROGRESS && field == 4)) {  // string mediaId / host
      int off, n;
      if (!rd.string(off, n)) { r.ok = OK_ERROR; return; }
      if (field == 1) { r.id_off = start + off; r.id_len = n; r.seen |= SEEN_ID; }
      else { r.host_off = start + off; r.host_len = n; r.seen |= SEEN_HOST; }
    } else if (field == 2 || (MSG == MSG_PROGRESS && field == 3)) {  // enum status / int32 progress: uint32() | 0
      uint32_t v;
      if (!rd.uint32(v)) { r.ok = OK_ERROR; return; }
      if (field == 2) { r.status = static_cast<int32_t>(v); r.seen |= SEEN_STATUS; }
      else { r.progress = static_cast<int32_t>(v); r.seen |= SEEN_PROGRESS; }
    } else if (!rd.skip_type(t & 7)) {
      r.ok = OK_ERROR;
      return;
    }
  }
}

// ---- the one entry point ------------------------------------------------------------------------
// Reads buf[start, end) as a TelemetryStatus (is_status) or a TelemetryProgress into r, a fresh Row.
// STRICT picks the upb reader's form; protobufjs has one form and ignores it. start and end come by
// reference so that the fold kernels compile to the instructions they had with the readers called
// directly (by value, hipcc loads offs[m + 1] later and allocates registers differently).
template <int DIALECT, bool STRICT>
BH_FN void read_message(const uint8_t* __restrict__ buf, const int& start, const int& end, const bool is_status,
                        Row& r) {
  static_assert(DIALECT == DIALECT_UPB || DIALECT == DIALECT_PROTOBUFJS, "unknown dialect");
  if constexpr (DIALECT == DIALECT_PROTOBUFJS) {
    if (is_status) decode_pbjs<MSG_STATUS>(buf, start, end, r);
    else decode_pbjs<MSG_PROGRESS>(buf, start, end, r);
  } else {
    if (is_status) decode_upb<MSG_STATUS, STRICT>(buf, start, end, r);
    else decode_upb<MSG_PROGRESS, STRICT>(buf, start, end, r);
  }
}

}  // namespace bh
