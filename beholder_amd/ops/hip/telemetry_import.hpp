// The per-line code of `import` (beholder_amd/import_rows.py frame_of_row), shared by the kernels
// (telemetry_import.hip) and a host program for CPU tests (tests/native/import_host.cpp): like
// telemetry_export.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same
// code runs under ASan/UBSan on a CPU.
//
// The input is text: NDJSON rows, one per line, which is what `export` writes. Nothing frames it, so the
// device finds the lines itself. newline_mask gives the `\n` bytes among the 16 bytes that one lane of
// the split takes; the two split kernels and the host program count and rank them with it.
//
// import_classify(buf, a, b, plan) reads the line buf[a, b) (its `\n` excluded), strips the bytes
// space, \t and \r from both ends, and fills one FramePlan:
//   IM_BLANK     nothing is left of the line: no frame, and no error.
//   IM_B64       a row with `topic` and `b64`: the base64 text's span, the decoded length, the topic byte.
//   IM_STATUS    a row with topic 1 and `json`: the id's text span and decoded length, and the status.
//   IM_PROGRESS  a row with topic 2 and `json`: the same with progress and the host's span.
//   IM_HOST      every other line: the device does not write it, and the host asks frame_of_row, which
//                says what its frame is or why it is malformed. The device never decides that a row is
//                malformed. out_len is 0.
// For IM_B64, IM_STATUS and IM_PROGRESS out_len is the frame's exact length, 0 otherwise.
//
// The grammar the reader decides is the export's three row shapes, relaxed:
//   row     = `{` member (`,` member)* `}` with JSON whitespace (space \t \r) between any two tokens
//   member  = "i": skipped | "name": skipped | "topic": topic | "b64": base64 | "json": object
//             in any order, each at most once; skipped is an integer token, a string or null
//   topic   = "v1.telemetry.status" | "v1.telemetry.progress" | an integer in 0..255
//   object  = `{` ("mediaId": string | "status": int32 | "progress": int32 | "host": string)* `}`
//             in any order, each at most once
//   integer = -?(0|[1-9][0-9]*)
//   string  = bytes 0x20..0x7f, and the escapes \" \\ \/ \b \f \n \r \t \u00XX with XX below 0x80
//   base64  = a string of the standard alphabet with correct padding, no escapes; bits left over in
//             the last character are ignored, as base64.b64decode ignores them
// A row has `topic`, and `b64` or `json`; `b64` wins. With `json` alone the topic is 1 or 2, and a
// status row's object holds neither progress nor host. Whatever does not fit goes to the host: a byte
// >= 0x80 anywhere in the line, a \uXXXX of 0x80 or more, a status given by name, another key or a key
// twice, a float, a number out of range, and everything the reader does not recognise.
//
// Why the output is smaller than the input, so that no output-size check is needed. A frame is
// `u32 L | u8 topic | body`, 5 bytes plus the body. The two minimal rows are `{"topic":0,"b64":""}`,
// 20 bytes, and `{"topic":1,"json":{}}`, 21 bytes: both give a frame of 5. Every byte of a body costs
// at least one byte of text on top of that: 3 base64 bytes take 4 characters; a string of n bytes
// takes its key (10 or 7 bytes with the colon), two quotes and at least n bytes of text (an escape
// takes 2 or 6 for one byte; a \uXXXX that the host decodes takes 6 for at most 3 bytes of UTF-8, a
// surrogate pair 12 for 4) against a tag, a length varint of at most 5 bytes and the n bytes; a number
// takes its key (9 or 11 bytes) and at least 1 digit against a tag and at most 5 varint bytes where it
// is positive, and at least 2 characters against a tag and 10 varint bytes where it is negative; a
// status by name gives no more bytes than a number. So a frame is at least 15 bytes shorter than its
// row, a line that gives no frame gives nothing, and the output stays below the input's 2^31.
//
// A frame is binary. walk_frame names its pieces in order to a sink; the length (frame_len), the byte
// at a position (frame_byte), a sequential writer (write_frame) and the places of the two strings
// (string_starts) are four sinks over that one walk, so they cannot disagree about what a frame is.
//
// A byte of the frame is a constant-time function of its position everywhere except inside a string
// whose text has escapes: there the text is walked in pieces of 64 bytes. Of each piece the mask of
// its backslashes and a carry from the piece before tell every position whether it begins a unit (a
// plain byte, or the backslash of a 2- or 6-byte escape, which unit_byte turns into its one byte) or
// lies inside one: Pieces::next. The kernel takes the mask from a ballot and the host program from a
// loop; both call the same code for the rest.
#pragma once
#include "telemetry_normalise.hpp"

namespace bh {

constexpr int IM_BLANK = 0, IM_B64 = 1, IM_STATUS = 2, IM_PROGRESS = 3, IM_HOST = 4;

struct FramePlan {
  int32_t kind;              // IM_*
  int32_t topic;             // the topic byte
  int32_t id_off, id_text;   // the id's text between its quotes, absolute in buf; IM_B64: the base64 text
  int32_t id_len;            // its decoded length; IM_B64: the body's length
  int32_t host_off, host_text, host_len;
  int32_t status, progress;
  int32_t out_len;           // the frame's length, header included; 0 where the device writes none
  int32_t reserved;
};
static_assert(sizeof(FramePlan) == 48, "ops/gpu_import.py views the plans as (n, 12) int32");

// ---- the split --------------------------------------------------------------------------------

constexpr int SPLIT_LANE_BYTES = 16;  // one wide load
constexpr int SPLIT_TILE_BYTES = 256 * SPLIT_LANE_BYTES;  // what a block of 256 lanes takes

// Bit k is set where byte k of the little-endian word is `\n`.
BH_FN uint32_t newline_bits(uint32_t w) {
  uint32_t bits = 0;
  BH_UNROLL
  for (int k = 0; k < 4; ++k) bits |= ((w >> (8 * k)) & 0xffu) == '\n' ? 1u << k : 0u;
  return bits;
}

// The lane's bytes buf[at, at + 16) that lie below size, as a 16-bit mask of its `\n` bytes. at is a
// multiple of 16 and buf is 16-byte aligned, so bytes that are all below size are one wide load.
BH_FN uint32_t newline_mask(const uint8_t* __restrict__ buf, int64_t size, int64_t at) {
  if (at >= size) return 0;
  uint32_t w[4] = {0, 0, 0, 0};
  if (at + SPLIT_LANE_BYTES <= size) {
#ifdef __HIPCC__
    const uint4 wide = *reinterpret_cast<const uint4*>(buf + at);
    w[0] = wide.x, w[1] = wide.y, w[2] = wide.z, w[3] = wide.w;
#else
    for (int k = 0; k < SPLIT_LANE_BYTES; ++k) w[k >> 2] |= static_cast<uint32_t>(buf[at + k]) << (8 * (k & 3));
#endif
  } else {
    const int left = static_cast<int>(size - at);  // 1..15
    for (int k = 0; k < left; ++k) w[k >> 2] |= static_cast<uint32_t>(buf[at + k]) << (8 * (k & 3));
  }
  return newline_bits(w[0]) | newline_bits(w[1]) << 4 | newline_bits(w[2]) << 8 | newline_bits(w[3]) << 12;
}

// ---- the reader -------------------------------------------------------------------------------

BH_FN bool is_blank(uint32_t c) { return c == ' ' || c == '\t' || c == '\r'; }

BH_FN void skip_blank(const uint8_t* __restrict__ buf, int& at, int end) {
  while (at < end && is_blank(buf[at])) ++at;
}

// 0..15, or -1.
BH_FN int hex_value(uint32_t c) {
  if (c >= '0' && c <= '9') return static_cast<int>(c - '0');
  c |= 0x20u;
  return c >= 'a' && c <= 'f' ? static_cast<int>(c - 'a') + 10 : -1;
}

// The byte that the escape `\e` stands for, or -1 where e begins none of the two-byte escapes.
BH_FN int short_escape(uint32_t e) {
  switch (e) {
    case '"': return '"';
    case '\\': return '\\';
    case '/': return '/';
    case 'b': return 8;
    case 'f': return 12;
    case 'n': return 10;
    case 'r': return 13;
    case 't': return 9;
    default: return -1;
  }
}

// A string whose opening quote is at buf[at - 1]: its text buf[off, off + text) and how many bytes it
// decodes to; at ends after the closing quote. False for what the grammar above does not hold, a
// string that does not end before `end` included.
BH_FN bool read_string(const uint8_t* __restrict__ buf, int& at, int end, int32_t& off, int32_t& text, int32_t& len) {
  off = at;
  int n = 0;
  while (at < end) {
    const uint32_t c = buf[at];
    if (c == '"') {
      text = at - off;
      len = n;
      ++at;
      return true;
    }
    if (c < 0x20 || c >= 0x80) return false;
    if (c != '\\') {
      ++at;
    } else if (at + 1 < end && short_escape(buf[at + 1]) >= 0) {
      at += 2;
    } else if (at + 5 < end && buf[at + 1] == 'u' && buf[at + 2] == '0' && buf[at + 3] == '0' &&
               hex_value(buf[at + 4]) >= 0 && hex_value(buf[at + 4]) < 8 && hex_value(buf[at + 5]) >= 0) {
      at += 6;
    } else {
      return false;
    }
    ++n;
  }
  return false;
}

// Whether the text buf[off, off + text) is exactly s.
template <int N>
BH_FN bool text_is(const uint8_t* __restrict__ buf, int32_t off, int32_t text, const char (&s)[N]) {
  if (text != N - 1) return false;
  for (int k = 0; k < N - 1; ++k)
    if (buf[off + k] != static_cast<uint8_t>(s[k])) return false;
  return true;
}

// What may follow a number or a literal: blank, `,`, `}` or the line's end.
BH_FN bool ends_token(const uint8_t* __restrict__ buf, int at, int end) {
  return at >= end || is_blank(buf[at]) || buf[at] == ',' || buf[at] == '}';
}

constexpr int64_t INT_TOKEN_MAX = int64_t(1) << 40;  // where a longer integer token's value stays: past every range here

// An integer token at buf[at]: its value, capped at +-2^40. False for what is no integer token.
BH_FN bool read_integer(const uint8_t* __restrict__ buf, int& at, int end, int64_t& value) {
  const bool negative = at < end && buf[at] == '-';
  if (negative) ++at;
  if (at >= end || buf[at] < '0' || buf[at] > '9') return false;
  int64_t v = 0;
  if (buf[at] == '0') {
    ++at;
  } else {
    while (at < end && buf[at] >= '0' && buf[at] <= '9') {
      v = v * 10 + (buf[at] - '0');
      if (v > INT_TOKEN_MAX) v = INT_TOKEN_MAX;
      ++at;
    }
  }
  if (!ends_token(buf, at, end)) return false;  // 01, 1.0, 1e5, 1x
  value = negative ? -v : v;
  return true;
}

// The value of "i" or "name", which import ignores: an integer token, a string or null.
BH_FN bool skip_value(const uint8_t* __restrict__ buf, int& at, int end) {
  if (at >= end) return false;
  if (buf[at] == '"') {
    int32_t off, text, len;
    ++at;
    return read_string(buf, at, end, off, text, len);
  }
  if (buf[at] == 'n') {
    if (end - at < 4 || buf[at + 1] != 'u' || buf[at + 2] != 'l' || buf[at + 3] != 'l') return false;
    at += 4;
    return ends_token(buf, at, end);
  }
  int64_t ignored;
  return read_integer(buf, at, end, ignored);
}

// 0..63 for a character of the standard alphabet, -1 otherwise.
BH_FN int b64_value(uint32_t c) {
  if (c >= 'A' && c <= 'Z') return static_cast<int>(c - 'A');
  if (c >= 'a' && c <= 'z') return static_cast<int>(c - 'a') + 26;
  if (c >= '0' && c <= '9') return static_cast<int>(c - '0') + 52;
  return c == '+' ? 62 : c == '/' ? 63 : -1;
}

// A base64 string whose opening quote is at buf[at - 1]: characters of the alphabet, then at most
// two `=`, a multiple of four in all. len is the decoded length.
BH_FN bool read_base64(const uint8_t* __restrict__ buf, int& at, int end, int32_t& off, int32_t& text, int32_t& len) {
  off = at;
  int pads = 0;
  while (at < end && buf[at] != '"') {
    if (buf[at] == '=') ++pads;
    else if (b64_value(buf[at]) < 0 || pads) return false;
    ++at;
  }
  if (at >= end) return false;
  text = at - off;
  ++at;
  if ((text & 3) != 0 || pads > 2) return false;
  len = text / 4 * 3 - pads;
  return true;
}

// Byte j of the bytes that the base64 text at p decodes to, 0 <= j < len: it comes from the four
// characters at 4 * (j / 3), which lie inside the text.
BH_FN uint32_t b64_decoded_byte(const uint8_t* __restrict__ p, int j) {
  const uint8_t* q = p + 4 * (j / 3);
  uint32_t v = 0;
  BH_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int six = b64_value(q[k]);
    v = v << 6 | static_cast<uint32_t>(six < 0 ? 0 : six);  // a pad
  }
  return (v >> (16 - 8 * (j % 3))) & 0xffu;
}

// ---- the frame --------------------------------------------------------------------------------

// The pieces of the frame of `plan` (IM_B64, IM_STATUS or IM_PROGRESS), in order:
//   sink.header(topic)                     the length word and the topic byte, 5 bytes
//   sink.tag(byte)                         a field's tag
//   sink.varint(v)                         a varint
//   sink.string(which, off, text, len)     the len bytes that the text buf[off, off + text) decodes to;
//                                          which is 0 for the id and 1 for the host
//   sink.base64(off, text, len)            the len bytes that the base64 text decodes to
template <class Sink>
BH_FN void walk_frame(const FramePlan& plan, Sink& sink) {
  sink.header(plan.topic);
  if (plan.kind == IM_B64) {
    sink.base64(plan.id_off, plan.id_text, plan.id_len);
    return;
  }
  if (plan.id_len > 0) {
    sink.tag(0x0a);
    sink.varint(static_cast<uint64_t>(plan.id_len));
    sink.string(0, plan.id_off, plan.id_text, plan.id_len);
  }
  if (plan.status != 0) {
    sink.tag(0x10);
    sink.varint(sign_extended(plan.status));
  }
  if (plan.kind == IM_PROGRESS) {
    if (plan.progress != 0) {
      sink.tag(0x18);
      sink.varint(sign_extended(plan.progress));
    }
    if (plan.host_len > 0) {
      sink.tag(0x22);
      sink.varint(static_cast<uint64_t>(plan.host_len));
      sink.string(1, plan.host_off, plan.host_text, plan.host_len);
    }
  }
}

struct FrameLengthSink {
  int64_t total = 0;
  BH_FN void header(int32_t) { total += 5; }
  BH_FN void tag(uint32_t) { total += 1; }
  BH_FN void varint(uint64_t v) { total += varint_len(v); }
  BH_FN void string(int, int32_t, int32_t, int32_t len) { total += len; }
  BH_FN void base64(int32_t, int32_t, int32_t len) { total += len; }
};

// The frame's exact length, from the plan's fields alone (out_len holds the same). Every length in
// the plan is below the line's, so the sum stays below 2^31.
BH_FN int32_t frame_len(const FramePlan& plan) {
  if (plan.kind != IM_B64 && plan.kind != IM_STATUS && plan.kind != IM_PROGRESS) return 0;
  FrameLengthSink sink;
  walk_frame(plan, sink);
  return static_cast<int32_t>(sink.total);
}

struct FrameStartSink {
  int32_t at = 0;
  int32_t start[2] = {0, 0};
  BH_FN void header(int32_t) { at += 5; }
  BH_FN void tag(uint32_t) { at += 1; }
  BH_FN void varint(uint64_t v) { at += varint_len(v); }
  BH_FN void string(int which, int32_t, int32_t, int32_t len) {
    start[which] = at;
    at += len;
  }
  BH_FN void base64(int32_t, int32_t, int32_t len) { at += len; }
};

// Where the id's bytes and the host's bytes begin in the frame of an event.
BH_FN void string_starts(const FramePlan& plan, int32_t& id_start, int32_t& host_start) {
  FrameStartSink sink;
  walk_frame(plan, sink);
  id_start = sink.start[0];
  host_start = sink.start[1];
}

struct FrameByteSink {
  const uint8_t* __restrict__ buf;
  int32_t out_len;
  int32_t rel;
  int32_t at = 0;
  uint32_t byte = 0;
  BH_FN bool inside(int32_t n) const { return rel >= at && rel < at + n; }
  BH_FN void header(int32_t topic) {
    if (inside(5)) byte = rel < 4 ? (static_cast<uint32_t>(out_len - 4) >> (8 * rel)) & 0xffu : static_cast<uint32_t>(topic);
    at += 5;
  }
  BH_FN void tag(uint32_t t) {
    if (inside(1)) byte = t;
    at += 1;
  }
  BH_FN void varint(uint64_t v) {
    const int n = varint_len(v);
    if (inside(n)) byte = varint_byte(v, rel - at, n);
    at += n;
  }
  BH_FN void string(int, int32_t off, int32_t, int32_t len) {
    if (inside(len)) byte = buf[off + (rel - at)];  // a plain copy: text == len is the caller's business
    at += len;
  }
  BH_FN void base64(int32_t off, int32_t, int32_t len) {
    if (inside(len)) byte = b64_decoded_byte(buf + off, rel - at);
    at += len;
  }
};

// Byte `rel` of the frame, 0 <= rel < plan.out_len, outside a string whose text has escapes. Reads
// buf only inside the plan's spans.
BH_FN uint32_t frame_byte(const uint8_t* __restrict__ buf, const FramePlan& plan, int32_t rel) {
  FrameByteSink sink{buf, plan.out_len, rel};
  walk_frame(plan, sink);
  return sink.byte;
}

// The byte of the unit that begins at p[k] in a string's text of n bytes that read_string accepted: the
// byte itself, or what the escape stands for.
BH_FN uint32_t unit_byte(const uint8_t* __restrict__ p, int k, int n) {
  const uint32_t c = p[k];
  if (c != '\\' || k + 1 >= n) return c;
  const uint32_t e = p[k + 1];
  if (e != 'u') return static_cast<uint32_t>(short_escape(e)) & 0xffu;
  if (k + 5 >= n) return 0;
  return (static_cast<uint32_t>(hex_value(p[k + 4])) << 4 | static_cast<uint32_t>(hex_value(p[k + 5]))) & 0xffu;
}

// A string's text in pieces of 64 bytes, piece after piece. next(backslashes, us, live) takes the
// masks of one piece (bit k: the piece's byte k is a backslash, is `u`, lies inside the text) and
// returns the mask of the bytes that begin a unit; between the pieces it carries whether the last
// byte was an escaping backslash, and how many bytes of a \u00XX are still to come.
struct Pieces {
  uint64_t escaped_first = 0;  // bit 0: the next piece's first byte is escaped
  uint64_t hex_first = 0;      // the next piece's first bytes that are a \u escape's hex digits

  BH_FN uint64_t next(uint64_t backslashes, uint64_t us, uint64_t live) {
    // A backslash escapes where the run of backslashes before it is even; a run that reaches the
    // piece's start goes on into the piece before, whose parity escaped_first holds.
    uint64_t escaping = 0;
    int run = static_cast<int>(escaped_first & 1);
    for (int k = 0; k < 64; ++k) {  // wave-uniform in the kernel: scalar code, once per piece
      const bool slash = (backslashes >> k) & 1;
      if (slash && (run & 1) == 0) escaping |= 1ull << k;
      run = slash ? run + 1 : 0;
    }
    const uint64_t escaped = escaping << 1 | (escaped_first & 1);
    const uint64_t u = escaped & us;  // the `u` of a \u00XX
    const uint64_t hex = u << 1 | u << 2 | u << 3 | u << 4 | hex_first;
    escaped_first = escaping >> 63;
    hex_first = u >> 63 | u >> 62 | u >> 61 | u >> 60;
    return live & ~(escaped | hex);
  }
};

struct FrameWriteSink {
  const uint8_t* __restrict__ buf;
  uint8_t* __restrict__ out;
  int32_t out_len;
  int64_t at = 0;
  BH_FN void put(uint32_t byte) { out[at++] = static_cast<uint8_t>(byte); }
  BH_FN void header(int32_t topic) {
    for (int k = 0; k < 4; ++k) put((static_cast<uint32_t>(out_len - 4) >> (8 * k)) & 0xffu);
    put(static_cast<uint32_t>(topic));
  }
  BH_FN void tag(uint32_t t) { put(t); }
  BH_FN void varint(uint64_t v) {
    const int n = varint_len(v);
    for (int k = 0; k < n; ++k) put(varint_byte(v, k, n));
  }
  BH_FN void string(int, int32_t off, int32_t text, int32_t) {
    for (int k = 0; k < text;) {
      put(unit_byte(buf + off, k, text));
      k += buf[off + k] != '\\' ? 1 : (k + 1 < text && buf[off + k + 1] == 'u') ? 6 : 2;
    }
  }
  BH_FN void base64(int32_t off, int32_t, int32_t len) {
    for (int j = 0; j < len; ++j) put(b64_decoded_byte(buf + off, j));
  }
};

// The frame, one byte after the other, into out[0, out_len); returns how many bytes it wrote.
BH_FN int64_t write_frame(const uint8_t* __restrict__ buf, const FramePlan& plan, uint8_t* __restrict__ out) {
  FrameWriteSink sink{buf, out, plan.out_len};
  walk_frame(plan, sink);
  return sink.at;
}

// ---- the plan ---------------------------------------------------------------------------------

constexpr uint32_t KEY_I = 1, KEY_NAME = 2, KEY_TOPIC = 4, KEY_B64 = 8, KEY_JSON = 16;     // a row's keys
constexpr uint32_t KEY_ID = 1, KEY_STATUS = 2, KEY_PROGRESS = 4, KEY_HOSTNAME = 8;        // the object's

// `"key" :` at buf[at], blanks allowed: the key's text span. False for anything else.
BH_FN bool read_key(const uint8_t* __restrict__ buf, int& at, int end, int32_t& off, int32_t& text) {
  if (at >= end || buf[at] != '"') return false;
  ++at;
  int32_t len;
  if (!read_string(buf, at, end, off, text, len) || len != text) return false;  // a key with an escape: the host's
  skip_blank(buf, at, end);
  if (at >= end || buf[at] != ':') return false;
  ++at;
  skip_blank(buf, at, end);
  return true;
}

// After a member: `,` and on (true, more = true), or the closing brace (true, more = false).
BH_FN bool after_member(const uint8_t* __restrict__ buf, int& at, int end, bool& more) {
  skip_blank(buf, at, end);
  if (at >= end || (buf[at] != ',' && buf[at] != '}')) return false;
  more = buf[at] == ',';
  ++at;
  if (more) skip_blank(buf, at, end);
  return true;
}

BH_FN bool read_int32(const uint8_t* __restrict__ buf, int& at, int end, int32_t& value) {
  int64_t v;
  if (!read_integer(buf, at, end, v) || v < INT32_MIN || v > INT32_MAX) return false;
  value = static_cast<int32_t>(v);
  return true;
}

// The value of "json" at buf[at]: the object's fields into plan, its keys into seen.
BH_FN bool read_object(const uint8_t* __restrict__ buf, int& at, int end, FramePlan& plan, uint32_t& seen) {
  if (at >= end || buf[at] != '{') return false;
  ++at;
  skip_blank(buf, at, end);
  if (at < end && buf[at] == '}') {
    ++at;
    return true;
  }
  for (bool more = true; more;) {  // every turn moves at forward, or ends the loop
    int32_t off, text;
    if (!read_key(buf, at, end, off, text)) return false;
    const uint32_t key = text_is(buf, off, text, "mediaId")    ? KEY_ID
                         : text_is(buf, off, text, "status")   ? KEY_STATUS
                         : text_is(buf, off, text, "progress") ? KEY_PROGRESS
                         : text_is(buf, off, text, "host")     ? KEY_HOSTNAME
                                                               : 0u;
    if (key == 0 || (seen & key)) return false;
    seen |= key;
    if (key == KEY_ID || key == KEY_HOSTNAME) {
      if (at >= end || buf[at] != '"') return false;
      ++at;
      const bool ok = key == KEY_ID ? read_string(buf, at, end, plan.id_off, plan.id_text, plan.id_len)
                                    : read_string(buf, at, end, plan.host_off, plan.host_text, plan.host_len);
      if (!ok) return false;
    } else if (!read_int32(buf, at, end, key == KEY_STATUS ? plan.status : plan.progress)) {
      return false;
    }
    if (!after_member(buf, at, end, more)) return false;
  }
  return true;
}

// The line buf[a, b) into plan; returns plan.kind. Reads buf only inside [a, b).
BH_FN int import_classify(const uint8_t* __restrict__ buf, int a, int b, FramePlan& plan) {
  while (a < b && is_blank(buf[a])) ++a;
  while (b > a && is_blank(buf[b - 1])) --b;
  plan = FramePlan{IM_BLANK, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (a == b) return IM_BLANK;
  const FramePlan host{IM_HOST, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  FramePlan event = plan;  // what "json" holds
  int32_t b64_off = 0, b64_text = 0, b64_len = 0;
  uint32_t seen = 0, fields = 0;
  int at = a;
  bool ok = buf[at] == '{';
  if (ok) {
    ++at;
    skip_blank(buf, at, b);
    if (at < b && buf[at] == '}') {
      ok = false;  // no topic
    } else {
      for (bool more = true; ok && more;) {  // every turn moves at forward, or ends the loop
        int32_t off, text;
        if (!read_key(buf, at, b, off, text)) {
          ok = false;
          break;
        }
        const uint32_t key = text_is(buf, off, text, "i")       ? KEY_I
                             : text_is(buf, off, text, "name")  ? KEY_NAME
                             : text_is(buf, off, text, "topic") ? KEY_TOPIC
                             : text_is(buf, off, text, "b64")   ? KEY_B64
                             : text_is(buf, off, text, "json")  ? KEY_JSON
                                                                : 0u;
        if (key == 0 || (seen & key)) {
          ok = false;
          break;
        }
        seen |= key;
        if (key == KEY_I || key == KEY_NAME) {
          ok = skip_value(buf, at, b);
        } else if (key == KEY_TOPIC) {
          if (at < b && buf[at] == '"') {
            int32_t len;
            ++at;
            ok = read_string(buf, at, b, off, text, len);
            if (ok && text_is(buf, off, text, "v1.telemetry.status")) event.topic = 1;
            else if (ok && text_is(buf, off, text, "v1.telemetry.progress")) event.topic = 2;
            else ok = false;
          } else {
            int64_t v = 0;
            ok = read_integer(buf, at, b, v) && v >= 0 && v <= 255;
            event.topic = static_cast<int32_t>(v);
          }
        } else if (key == KEY_B64) {
          ok = at < b && buf[at] == '"';
          if (ok) {
            ++at;
            ok = read_base64(buf, at, b, b64_off, b64_text, b64_len);
          }
        } else {
          ok = read_object(buf, at, b, event, fields);
        }
        ok = ok && after_member(buf, at, b, more);
      }
    }
  }
  ok = ok && at == b && (seen & KEY_TOPIC) && (seen & (KEY_B64 | KEY_JSON));
  if (ok && (seen & KEY_B64)) {
    plan = FramePlan{IM_B64, event.topic, b64_off, b64_text, b64_len, 0, 0, 0, 0, 0, 0, 0};
  } else if (ok && (event.topic == 1 || event.topic == 2) &&
             !(event.topic == 1 && (fields & (KEY_PROGRESS | KEY_HOSTNAME)))) {
    plan = event;
    plan.kind = event.topic == 1 ? IM_STATUS : IM_PROGRESS;
  } else {
    plan = host;
    return IM_HOST;
  }
  plan.out_len = frame_len(plan);
  return plan.kind;
}

}  // namespace bh
