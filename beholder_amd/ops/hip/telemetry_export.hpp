// The per-frame code of `export` (beholder_amd/export.py row_of), shared by the kernels
// (telemetry_export.hip) and a host program for CPU tests (tests/native/export_host.cpp): like
// telemetry_normalise.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same
// code runs under ASan/UBSan on a CPU.
//
// export_classify<DIALECT>(buf, head, end, drop, index, plan) reads the frame buf[head, end)
// (`u32 L | u8 topic | body`) by its topic (read_message, upb in its STRICT form) and fills one RowPlan:
//   EX_B64       an undecoded frame (another topic, or a decode error) where those are kept: id_off and
//                id_len are the body's span, topic the topic byte.
//   EX_DROP      the same frames where undecoded frames are dropped. row_len is 0.
//   EX_HOST      the device does not write this frame and the host asks export.row_of instead: a decoded
//                frame whose id span or host span holds a byte >= 0x80, in either dialect (under upb
//                the host decides whether it is UTF-8, under protobufjs the decoding may substitute
//                U+FFFD); under upb also a start-group (OK_HOST). row_len is 0.
//   EX_TOO_LONG  a row of 2^31 bytes or more, which no output the scan can place holds. row_len is 0.
//   EX_STATUS    a decoded status event: id span and status.
//   EX_PROGRESS  a decoded progress event: id span, status, progress and host span.
// For EX_B64, EX_STATUS and EX_PROGRESS row_len is the row's exact length, newline included.
//
// The row is text (export.py has the definition): fixed key text, decimal numbers, JSON strings and
// base64. walk_row names its pieces in order to a sink; the length (row_len), the byte at a position
// (row_byte), a sequential writer (write_row) and the places of the two strings (string_starts) are
// four sinks over that one walk, so they cannot disagree about what a row is.
//
// A byte of the row is a constant-time function of its position everywhere except inside a string
// that has escapes: there the position of input byte k is the sum of esc_width over the k bytes
// before it. id_esc and host_esc hold the strings' escaped lengths. row_byte reads a string as a plain
// copy, which is right exactly where the escaped length equals the length; the kernel walks a string
// with escapes in pieces of 64 input bytes (esc_width, a prefix sum, esc_byte), and the host program
// does the same walk with a loop for the wave.
#pragma once
#include "media_table.hpp"

namespace bh {

constexpr int EX_B64 = 0, EX_DROP = 1, EX_HOST = 2, EX_STATUS = 3, EX_PROGRESS = 4, EX_TOO_LONG = 5;

struct RowPlan {
  int32_t id_off, id_len;  // absolute in buf; EX_B64: the body's span
  int32_t status, progress;
  int32_t host_off, host_len;
  int32_t id_esc, host_esc;  // the spans' lengths as JSON string text, without the quotes
  int32_t kind;              // EX_*
  int32_t topic;             // the frame's topic byte
  int32_t row_len;           // the row's length, newline included; 0 where the device writes none
  int32_t reserved;
};
static_assert(sizeof(RowPlan) == 48, "ops/gpu_export.py views the plans as (n, 12) int32");

constexpr int64_t ROW_LEN_LIMIT = int64_t(1) << 31;

// ---- JSON string text, json.dumps with ensure_ascii=False ------------------------------------

// How many bytes the byte c takes inside a JSON string: 2 for `"`, `\` and \b \t \n \f \r, 6
// (\u00XX) for every other byte below 0x20, 1 for the rest, 0x7f and 0x80.. included.
BH_FN int esc_width(uint32_t c) {
  if (c == '"' || c == '\\') return 2;
  if (c >= 0x20) return 1;
  return (c == 8 || c == 9 || c == 10 || c == 12 || c == 13) ? 2 : 6;
}

BH_FN uint32_t hex_digit(uint32_t v) { return v < 10 ? '0' + v : 'a' + (v - 10); }

// Byte k of those, 0 <= k < esc_width(c).
BH_FN uint32_t esc_byte(uint32_t c, int k) {
  const int w = esc_width(c);
  if (w == 1) return c;
  if (k == 0) return '\\';
  if (w == 2) return c == 8 ? 'b' : c == 9 ? 't' : c == 10 ? 'n' : c == 12 ? 'f' : c == 13 ? 'r' : c;
  return k == 1 ? 'u' : k < 4 ? '0' : hex_digit(k == 4 ? c >> 4 : c & 15u);
}

BH_FN int64_t esc_len(const uint8_t* __restrict__ p, int n) {
  int64_t total = 0;
  for (int k = 0; k < n; ++k) total += esc_width(p[k]);
  return total;
}

// ---- decimal ---------------------------------------------------------------------------------

BH_FN int dec_len(uint64_t v) {
  int n = 1;
  while (v >= 10) {
    v /= 10;
    ++n;
  }
  return n;
}

// Digit k from the left of v, which has n digits.
BH_FN uint32_t dec_byte(uint64_t v, int n, int k) {
  for (int j = n - 1 - k; j > 0; --j) v /= 10;
  return '0' + static_cast<uint32_t>(v % 10);
}

BH_FN uint64_t magnitude(int32_t x) {
  return x < 0 ? uint64_t(0) - static_cast<uint64_t>(static_cast<int64_t>(x)) : static_cast<uint64_t>(x);
}

// ---- base64, the standard alphabet with padding ----------------------------------------------

BH_FN int64_t b64_len(int n) { return 4 * ((static_cast<int64_t>(n) + 2) / 3); }

// Byte k of the base64 text of the n bytes at p, 0 <= k < b64_len(n): it comes from p[3 * (k / 4) ..].
BH_FN uint32_t b64_byte(const uint8_t* __restrict__ p, int n, int64_t k) {
  const int64_t at = 3 * (k >> 2);
  const int j = static_cast<int>(k & 3);
  const int left = static_cast<int>(n - at);  // 1 or more
  if (j > left) return '=';
  const uint32_t b0 = p[at], b1 = left > 1 ? p[at + 1] : 0u, b2 = left > 2 ? p[at + 2] : 0u;
  const uint32_t v = ((b0 << 16 | b1 << 8 | b2) >> (18 - 6 * j)) & 63u;
  return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/';
}

// ---- the row ---------------------------------------------------------------------------------

struct Text {
  const char* p;
  int n;
};
template <int N>
BH_FN Text text_of(const char (&s)[N]) { return Text{s, N - 1}; }

// `"NAME"` of TelemetryStatusEntry (models/proto/api.proto), or `null`.
BH_FN Text name_text(int32_t status) {
  switch (status) {
    case 0: return text_of("\"QUEUED\"");
    case 1: return text_of("\"DOWNLOADING\"");
    case 2: return text_of("\"CONVERTING\"");
    case 3: return text_of("\"UPLOADING\"");
    case 4: return text_of("\"DEPLOYED\"");
    case 5: return text_of("\"ERRORED\"");
    default: return text_of("null");
  }
}

// The pieces of the row of `plan` (EX_B64, EX_STATUS or EX_PROGRESS) for frame `index`, in order:
//   sink.text(Text)                      fixed bytes
//   sink.number(magnitude, negative)     a decimal
//   sink.string(which, off, len, esc)    the JSON text of buf[off, off + len), esc bytes; which is 0
//                                        for the id and 1 for the host
//   sink.base64(off, len)                the base64 text of buf[off, off + len)
template <class Sink>
BH_FN void walk_row(const RowPlan& plan, uint64_t index, Sink& sink) {
  sink.text(text_of("{\"i\":"));
  sink.number(index, false);
  if (plan.kind == EX_B64) {
    sink.text(text_of(",\"topic\":"));
    if (plan.topic == 1) sink.text(text_of("\"v1.telemetry.status\""));
    else if (plan.topic == 2) sink.text(text_of("\"v1.telemetry.progress\""));
    else sink.number(static_cast<uint64_t>(plan.topic), false);
    sink.text(text_of(",\"b64\":\""));
    sink.base64(plan.id_off, plan.id_len);
    sink.text(text_of("\"}\n"));
    return;
  }
  const bool is_status = plan.kind == EX_STATUS;
  sink.text(is_status ? text_of(",\"topic\":\"v1.telemetry.status\",\"json\":{\"mediaId\":\"")
                      : text_of(",\"topic\":\"v1.telemetry.progress\",\"json\":{\"mediaId\":\""));
  sink.string(0, plan.id_off, plan.id_len, plan.id_esc);
  sink.text(text_of("\",\"status\":"));
  sink.number(magnitude(plan.status), plan.status < 0);
  if (!is_status) {
    sink.text(text_of(",\"progress\":"));
    sink.number(magnitude(plan.progress), plan.progress < 0);
    sink.text(text_of(",\"host\":\""));
    sink.string(1, plan.host_off, plan.host_len, plan.host_esc);
    sink.text(text_of("\""));
  }
  sink.text(text_of("},\"name\":"));
  sink.text(name_text(plan.status));
  sink.text(text_of("}\n"));
}

struct LengthSink {
  int64_t total = 0;
  BH_FN void text(Text t) { total += t.n; }
  BH_FN void number(uint64_t v, bool negative) { total += dec_len(v) + (negative ? 1 : 0); }
  BH_FN void string(int, int32_t, int32_t, int32_t esc) { total += esc; }
  BH_FN void base64(int32_t, int32_t len) { total += b64_len(len); }
};

// The row's exact length, from the plan's fields alone (row_len holds the same where it fits).
BH_FN int64_t row_len(const RowPlan& plan, uint64_t index) {
  if (plan.kind != EX_B64 && plan.kind != EX_STATUS && plan.kind != EX_PROGRESS) return 0;
  LengthSink sink;
  walk_row(plan, index, sink);
  return sink.total;
}

struct StartSink {
  int64_t at = 0;
  int64_t start[2] = {0, 0};
  BH_FN void text(Text t) { at += t.n; }
  BH_FN void number(uint64_t v, bool negative) { at += dec_len(v) + (negative ? 1 : 0); }
  BH_FN void string(int which, int32_t, int32_t, int32_t esc) {
    start[which] = at;
    at += esc;
  }
  BH_FN void base64(int32_t, int32_t len) { at += b64_len(len); }
};

// Where the id's text and the host's text begin in the row of a decoded event.
BH_FN void string_starts(const RowPlan& plan, uint64_t index, int32_t& id_start, int32_t& host_start) {
  StartSink sink;
  walk_row(plan, index, sink);
  id_start = static_cast<int32_t>(sink.start[0]);
  host_start = static_cast<int32_t>(sink.start[1]);
}

struct ByteSink {
  const uint8_t* __restrict__ buf;
  int64_t rel;
  int64_t at = 0;
  uint32_t byte = 0;
  BH_FN bool inside(int64_t n) const { return rel >= at && rel < at + n; }
  BH_FN void text(Text t) {
    if (inside(t.n)) byte = static_cast<uint8_t>(t.p[rel - at]);
    at += t.n;
  }
  BH_FN void number(uint64_t v, bool negative) {
    const int digits = dec_len(v), sign = negative ? 1 : 0;
    if (inside(sign + digits)) {
      const int k = static_cast<int>(rel - at);
      byte = k < sign ? '-' : dec_byte(v, digits, k - sign);
    }
    at += sign + digits;
  }
  BH_FN void string(int, int32_t off, int32_t, int32_t esc) {
    if (inside(esc)) byte = buf[off + (rel - at)];  // a plain copy: esc == len is the caller's business
    at += esc;
  }
  BH_FN void base64(int32_t off, int32_t len) {
    const int64_t n = b64_len(len);
    if (inside(n)) byte = b64_byte(buf + off, len, rel - at);
    at += n;
  }
};

// Byte `rel` of the row, 0 <= rel < row_len(plan, index), outside a string that has escapes. Reads buf
// only inside the plan's spans.
BH_FN uint32_t row_byte(const uint8_t* __restrict__ buf, const RowPlan& plan, uint64_t index, int64_t rel) {
  ByteSink sink{buf, rel};
  walk_row(plan, index, sink);
  return sink.byte;
}

struct WriteSink {
  const uint8_t* __restrict__ buf;
  uint8_t* __restrict__ out;
  int64_t at = 0;
  BH_FN void put(uint32_t byte) { out[at++] = static_cast<uint8_t>(byte); }
  BH_FN void text(Text t) {
    for (int k = 0; k < t.n; ++k) put(static_cast<uint8_t>(t.p[k]));
  }
  BH_FN void number(uint64_t v, bool negative) {
    const int digits = dec_len(v);
    if (negative) put('-');
    for (int k = 0; k < digits; ++k) put(dec_byte(v, digits, k));
  }
  BH_FN void string(int, int32_t off, int32_t len, int32_t) {
    for (int k = 0; k < len; ++k) {
      const uint32_t c = buf[off + k];
      const int w = esc_width(c);
      for (int j = 0; j < w; ++j) put(esc_byte(c, j));
    }
  }
  BH_FN void base64(int32_t off, int32_t len) {
    const int64_t n = b64_len(len);
    for (int64_t k = 0; k < n; ++k) put(b64_byte(buf + off, len, k));
  }
};

// The row, one byte after the other, into out[0, row_len); returns how many bytes it wrote.
BH_FN int64_t write_row(const uint8_t* __restrict__ buf, const RowPlan& plan, uint64_t index, uint8_t* __restrict__ out) {
  WriteSink sink{buf, out};
  walk_row(plan, index, sink);
  return sink.at;
}

template <int DIALECT>
BH_FN int export_classify(const uint8_t* __restrict__ buf, const int head, const int end, const bool drop,
                          const uint64_t index, RowPlan& plan) {
  const int32_t topic = buf[head + 4];
  plan = RowPlan{head + 5, end - head - 5, 0, 0, 0, 0, 0, 0, drop ? EX_DROP : EX_B64, topic, 0, 0};
  int64_t id_esc = 0, host_esc = 0;
  if (topic == 1 || topic == 2) {
    const bool is_status = topic == 1;
    Row r;
    read_message<DIALECT, true>(buf, head + 5, end, is_status, r);
    if (r.ok != OK_ERROR) {
      if (r.ok == OK_HOST || has_high_byte(buf + r.id_off, r.id_len) ||
          (!is_status && has_high_byte(buf + r.host_off, r.host_len))) {
        plan = RowPlan{head + 5, 0, 0, 0, 0, 0, 0, 0, EX_HOST, topic, 0, 0};
        return EX_HOST;
      }
      id_esc = esc_len(buf + r.id_off, r.id_len);
      host_esc = is_status ? 0 : esc_len(buf + r.host_off, r.host_len);
      plan.id_off = r.id_off;
      plan.id_len = r.id_len;
      plan.status = r.status;
      plan.progress = is_status ? 0 : r.progress;
      plan.host_off = is_status ? 0 : r.host_off;
      plan.host_len = is_status ? 0 : r.host_len;
      plan.kind = is_status ? EX_STATUS : EX_PROGRESS;
    }
  }
  if (plan.kind == EX_DROP) return EX_DROP;
  // each escaped length is below 6 * 2^31, so the sums below stay far inside 64 bits
  const bool fits = id_esc < ROW_LEN_LIMIT && host_esc < ROW_LEN_LIMIT;
  plan.id_esc = fits ? static_cast<int32_t>(id_esc) : 0;
  plan.host_esc = fits ? static_cast<int32_t>(host_esc) : 0;
  const int64_t length = fits ? row_len(plan, index) : ROW_LEN_LIMIT;
  if (length >= ROW_LEN_LIMIT) {
    plan = RowPlan{head + 5, 0, 0, 0, 0, 0, 0, 0, EX_TOO_LONG, topic, 0, 0};
    return EX_TOO_LONG;
  }
  plan.row_len = static_cast<int32_t>(length);
  return plan.kind;
}

}  // namespace bh
