// The per-frame code of the gfx950 anonymise kernels (beholder_amd/ops/hip/telemetry_anonymise.hpp),
// compiled for the host. Built by tests/test_hip_anonymise_host.py with -fsanitize=address,undefined:
// every string and every frame is read from a heap block of exactly its own size, so a read one byte
// past it is a sanitizer report here, not a fault on a GPU.
//
//   anonymise_host_asan hash LINES
//   anonymise_host_asan stream upb|protobufjs STREAM keep|drop FIELDS HEXKEY
//
// hash: LINES holds `HEXKEY mediaId|host HEXSTRING` per line, the string not empty; one digest per
// line goes to stdout, 32 hex digits put together from anon_digit, from the state after the key block
// as the launcher computes it (anon_midstates) and anon_digest.
//
// stream: STREAM holds `u32 L | u8 topic | body` frames (transport/framing.py), FIELDS is 1 (mediaId),
// 2 (host) or 3. One line per frame goes to stdout: `drop`, `host`, or `copy|status|progress FRAME
// GROWTH` with the output frame in hex, put together from anon_byte for every rel < anon_len into a
// block of exactly that size, and its length minus the input frame's. The program fails where
// anon_len and the plan's out_len differ, where a span leaves the frame, or where a frame grows by
// more than AN_GROWTH_MAX.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "telemetry_anonymise.hpp"

using namespace bh;

using Classify = int (*)(const uint8_t*, int, int, bool, int, const Midstates&, AnonPlan&);

static bool unhex(const std::string& text, std::vector<uint8_t>& out) {
  out.clear();
  if (text.size() % 2) return false;
  for (size_t i = 0; i < text.size(); i += 2) {
    unsigned byte = 0;
    if (std::sscanf(text.substr(i, 2).c_str(), "%2x", &byte) != 1) return false;
    out.push_back(uint8_t(byte));
  }
  return true;
}

// An exact-size heap copy: a key, a string or a frame with nothing readable behind it.
static std::unique_ptr<uint8_t[]> exact_copy(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(block.get(), p, n);
  return block;
}

static bool midstates_of(const std::string& hexkey, Midstates& mids) {
  std::vector<uint8_t> key;
  if (!unhex(hexkey, key)) return false;
  const auto block = exact_copy(key.data(), key.size());
  return anon_midstates(block.get(), int(key.size()), mids);
}

static int hash_mode(const char* path) {
  std::ifstream in(path);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream words(line);
    std::string hexkey, field, hexstring;
    words >> hexkey >> field >> hexstring;
    Midstates mids;
    std::vector<uint8_t> text;
    if (!midstates_of(hexkey, mids) || (field != "mediaId" && field != "host") || !unhex(hexstring, text) ||
        text.empty()) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    const auto block = exact_copy(text.data(), text.size());
    uint32_t digest[4];
    anon_digest(field == "host" ? mids.host : mids.id, block.get(), int(text.size()), digest);
    for (int k = 0; k < AN_DIGITS; ++k) std::putchar(int(anon_digit(digest, k)));
    std::putchar('\n');
  }
  return 0;
}

static bool inside(int off, int len, size_t size) {
  if (off == AN_REPLACED) return len == AN_DIGITS;
  return len >= 0 && (len == 0 || (off >= 5 && size_t(off) + size_t(len) <= size));
}

static int stream_mode(char** argv) {
  Classify classify_frame = nullptr;
  if (std::string(argv[2]) == "upb") classify_frame = anon_classify<DIALECT_UPB>;
  if (std::string(argv[2]) == "protobufjs") classify_frame = anon_classify<DIALECT_PROTOBUFJS>;
  const std::string undecoded = argv[4];
  const int fields = std::atoi(argv[5]);
  Midstates mids;
  if (!classify_frame || (undecoded != "keep" && undecoded != "drop") || fields < 1 || fields > 3 ||
      !midstates_of(argv[6], mids)) {
    std::fprintf(stderr, "usage: %s stream upb|protobufjs STREAM keep|drop 1|2|3 HEXKEY\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[3], std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[3]);
    return 2;
  }
  const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (data.size() >= (1u << 31)) {
    std::fprintf(stderr, "stream too large for int32 offsets\n");
    return 2;
  }
  const size_t n = data.size();
  for (size_t i = 0; i < n;) {
    uint32_t L = 0;
    if (n - i >= 4) std::memcpy(&L, &data[i], 4);  // little-endian hosts only, as the kernels' are
    if (L == 0 || n - i - 4 < L) {
      std::fprintf(stderr, "truncated or empty frame at byte %zu\n", i);
      return 2;
    }
    const size_t size = 4 + size_t(L);
    const auto exact = exact_copy(&data[i], size);
    i += size;
    AnonPlan plan;
    const int kind = classify_frame(exact.get(), 0, int(size), undecoded == "drop", fields, mids, plan);
    if (kind != plan.p.kind) {
      std::fprintf(stderr, "anon_classify returns %d and writes kind %d\n", kind, plan.p.kind);
      return 2;
    }
    const int length = anon_len(plan);
    if (length != plan.p.out_len) {
      std::fprintf(stderr, "anon_len is %d and the plan's out_len %d\n", length, plan.p.out_len);
      return 2;
    }
    if (kind == NM_DROP || kind == NM_HOST) {
      if (length != 0) {
        std::fprintf(stderr, "a frame the device does not write has the length %d\n", length);
        return 2;
      }
      std::puts(kind == NM_DROP ? "drop" : "host");
      continue;
    }
    if (kind != NM_COPY && kind != NM_STATUS && kind != NM_PROGRESS) {
      std::fprintf(stderr, "unknown kind %d\n", kind);
      return 2;
    }
    if (kind != NM_COPY &&
        (!inside(plan.p.id_off, plan.p.id_len, size) || !inside(plan.p.host_off, plan.p.host_len, size))) {
      std::fprintf(stderr, "a span lies outside a frame of %zu bytes\n", size);
      return 2;
    }
    const long long growth = static_cast<long long>(length) - static_cast<long long>(size);
    if (length < 5 || growth > AN_GROWTH_MAX || (kind == NM_COPY && growth != 0)) {
      std::fprintf(stderr, "a frame of %zu bytes becomes one of %d: more than AN_GROWTH_MAX\n", size, length);
      return 2;
    }
    const std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(length)]);
    for (int rel = 0; rel < length; ++rel) out[size_t(rel)] = uint8_t(anon_byte(exact.get(), plan, rel));
    std::fputs(kind == NM_COPY ? "copy " : kind == NM_STATUS ? "status " : "progress ", stdout);
    for (int rel = 0; rel < length; ++rel) std::printf("%02x", out[size_t(rel)]);
    std::printf(" %lld\n", growth);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "hash") return hash_mode(argv[2]);
  if (argc == 7 && std::string(argv[1]) == "stream") return stream_mode(argv);
  std::fprintf(stderr, "usage: %s hash LINES | stream upb|protobufjs STREAM keep|drop 1|2|3 HEXKEY\n", argv[0]);
  return 2;
}
