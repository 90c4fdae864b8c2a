// The per-frame code of `anonymise` (beholder_amd/anonymise.py anon_of), shared by the kernels
// (telemetry_anonymise.hip) and a host program for CPU tests (tests/native/anonymise_host.cpp): like
// telemetry_normalise.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same
// code runs under ASan/UBSan on a CPU.
//
// An anonymised frame is the normalise's canonical frame (telemetry_normalise.hpp) with the chosen
// strings, mediaId and host, replaced by keyed pseudonyms: the 32 lowercase hex digits of
//   blake2s(string, key=key, digest_size=16, person="bh.media" or "bh.host")
// so a replaced string of n >= 1 bytes is written as tag, 0x20, 32 digits, and an empty one is not
// written at all, as before.
//
// anon_classify<DIALECT>(buf, head, end, drop, fields, mids, plan) reads the frame exactly as
// norm_classify does (it calls it), applies the same NM_HOST rule plus one of its own (below), hashes
// the spans of the chosen fields and fills one AnonPlan: the normalise's Plan, in which a replaced
// string has the offset AN_REPLACED and the length 32, plus four digest words per string. So
// anon_len is canon_len of that Plan, and anon_byte is canon_byte except inside the 32 digits of a
// replaced string, where it reads the digest and nothing of the input.
//
// One more kind of frame goes to the host (NM_HOST): a decoded event with a chosen string above
// AN_STRING_MAX bytes, the dedupe's limit. It keeps one lane from running hundreds of compressions
// while its wave waits; 4,096 bytes are 64 of them.
//
// The hash is keyed BLAKE2s (RFC 7693) with a 16-byte digest, written out. The key block is the first
// block of every hash and depends on the key and the field alone, so the launcher's host code runs
// that one compression per field (anon_midstate) and the kernel gets the two states after it by
// value, uniform for every lane: the key itself never goes to the device. A hashed string is never
// empty, so the key block is never the final block.
#pragma once
#include "telemetry_normalise.hpp"

#ifdef __HIPCC__
#define BH_HD __host__ __device__ __forceinline__  // the launcher's host code runs compress too
#define BH_NOUNROLL _Pragma("nounroll")
#else
#define BH_HD inline
#define BH_NOUNROLL
#endif

namespace bh {

constexpr int AN_MEDIA = 1, AN_HOST = 2;  // bits of `fields`: the strings to replace
constexpr int AN_REPLACED = -1;           // Plan::id_off and host_off of a replaced string
constexpr int AN_DIGITS = 32;             // and its length: 16 digest bytes in hex
constexpr int AN_STRING_MAX = 4096;       // a longer chosen string goes to the host
constexpr int AN_KEY_MIN = 16, AN_KEY_MAX = 32;

struct AnonPlan {
  Plan p;                   // telemetry_normalise.hpp; a replaced string: offset AN_REPLACED, length 32
  uint32_t id_digest[4];    // the digest's 16 bytes, little-endian; 0 where the id is not replaced
  uint32_t host_digest[4];
};
static_assert(sizeof(AnonPlan) == 64, "ops/gpu_anonymise.py views the plans as (n, 16) int32");

// The states after the key block, one per field. A kernel argument: 16 scalars.
struct Midstates {
  uint32_t id[8];
  uint32_t host[8];
};

// The most bytes by which an anonymised frame exceeds the input frame it was decoded from.
//
// NM_GROWTH_MAX's argument (telemetry_normalise.hpp) holds field by field, with one change:
//  * A replaced string of n >= 1 bytes takes 1 + 1 + 32 = 34 bytes. Its occurrence holds a tag of at
//    least 1 byte, a length varint of at least 1 byte and the n >= 1 bytes themselves, at least 3: 31
//    more at most. A string that is not replaced does not grow, an empty one is not written.
//  * An int32 grows by 5 at most, as there.
// A progress event has two strings and two int32, so the bound is 31 + 31 + 5 + 5 = 72, and the frame
// `02 | 0a 01 6d | 10 ff ff ff ff 0f | 18 ff ff ff ff 0f | 22 01 68` reaches it. A status event stays
// at 36. Frames left to the host are not covered, as there.
constexpr int AN_GROWTH_MAX = 72;

BH_HD uint32_t b2s_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

#define BH_B2S_G(a, b, c, d, x, y) \
  a += b + (x);                    \
  d = b2s_rotr(d ^ a, 16);         \
  c += d;                          \
  b = b2s_rotr(b ^ c, 12);         \
  a += b + (y);                    \
  d = b2s_rotr(d ^ a, 8);          \
  c += d;                          \
  b = b2s_rotr(b ^ c, 7);
// One round: the columns, then the diagonals. The schedule row is sixteen literals, so every index
// into m[] and v[] is a compile-time constant and both arrays live in registers.
#define BH_B2S_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  BH_B2S_G(v[0], v[4], v[8], v[12], m[s0], m[s1])                                          \
  BH_B2S_G(v[1], v[5], v[9], v[13], m[s2], m[s3])                                          \
  BH_B2S_G(v[2], v[6], v[10], v[14], m[s4], m[s5])                                         \
  BH_B2S_G(v[3], v[7], v[11], v[15], m[s6], m[s7])                                         \
  BH_B2S_G(v[0], v[5], v[10], v[15], m[s8], m[s9])                                         \
  BH_B2S_G(v[1], v[6], v[11], v[12], m[s10], m[s11])                                       \
  BH_B2S_G(v[2], v[7], v[8], v[13], m[s12], m[s13])                                        \
  BH_B2S_G(v[3], v[4], v[9], v[14], m[s14], m[s15])

// BLAKE2s's compression of the block m into h; t is the byte count so far, this block included, which
// stays below 2^32 here, so the counter's high word is 0.
BH_HD void b2s_compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint32_t t, bool last) {
  uint32_t v[16] = {h[0],        h[1],        h[2],        h[3],        h[4],        h[5],
                    h[6],        h[7],        0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                    0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  v[12] ^= t;
  if (last) v[14] = ~v[14];
  BH_B2S_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  BH_B2S_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  BH_B2S_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  BH_B2S_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  BH_B2S_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  BH_B2S_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  BH_B2S_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  BH_B2S_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  BH_B2S_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  BH_B2S_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
  BH_UNROLL
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

#undef BH_B2S_ROUND
#undef BH_B2S_G

// Bytes p[0, n), 0 <= n <= 64, as the sixteen little-endian words of a block, zero-padded. Reads
// nothing past p[n - 1].
BH_HD void b2s_block(const uint8_t* __restrict__ p, int n, uint32_t (&m)[16]) {
  BH_UNROLL
  for (int w = 0; w < 16; ++w) {
    uint32_t x = 0;
    BH_UNROLL
    for (int j = 0; j < 4; ++j)
      if (4 * w + j < n) x |= static_cast<uint32_t>(p[4 * w + j]) << (8 * j);
    m[w] = x;
  }
}

// The state after the key block: h = IV ^ P, then the key, zero-padded to 64 bytes, at counter 64.
// P's word 0 is digest_size 16 | keylen << 8 | fanout 1 << 16 | depth 1 << 24, words 6 and 7 are the
// eight `person` bytes. False for a key that is not AN_KEY_MIN to AN_KEY_MAX bytes.
BH_HD bool anon_midstate(const uint8_t* key, int keylen, const char* person, uint32_t (&h)[8]) {
  if (!key || keylen < AN_KEY_MIN || keylen > AN_KEY_MAX) return false;
  const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                          0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  uint32_t person_words[2] = {0, 0};
  for (int i = 0; i < 8 && person[i]; ++i)  // up to eight bytes, zero-padded
    person_words[i >> 2] |= static_cast<uint32_t>(static_cast<uint8_t>(person[i])) << (8 * (i & 3));
  for (int i = 0; i < 8; ++i) h[i] = iv[i];
  h[0] ^= 16u | static_cast<uint32_t>(keylen) << 8 | 1u << 16 | 1u << 24;
  h[6] ^= person_words[0];
  h[7] ^= person_words[1];
  uint32_t m[16];
  b2s_block(key, keylen, m);
  b2s_compress(h, m, 64u, false);
  return true;
}

BH_HD bool anon_midstates(const uint8_t* key, int keylen, Midstates& mids) {
  return anon_midstate(key, keylen, "bh.media", mids.id) && anon_midstate(key, keylen, "bh.host", mids.host);
}

// The 16-byte digest of p[0, n), n >= 1, continued from the state after the key block. A length that
// is a multiple of 64 ends on a full final block.
BH_FN void anon_digest(const uint32_t (&mid)[8], const uint8_t* __restrict__ p, int n, uint32_t (&digest)[4]) {
  uint32_t h[8];
  BH_UNROLL
  for (int i = 0; i < 8; ++i) h[i] = mid[i];
  uint32_t m[16];
  for (int off = 0;; off += 64) {  // one compression in the code, however many blocks
    const int rest = n - off;
    const bool last = rest <= 64;
    const int take = last ? rest : 64;
    b2s_block(p + off, take, m);
    b2s_compress(h, m, 64u + static_cast<uint32_t>(off + take), last);
    if (last) break;
  }
  BH_UNROLL
  for (int i = 0; i < 4; ++i) digest[i] = h[i];
}

// Byte k of a replaced string, 0 <= k < 32: the high (k even) or low nibble of digest byte k >> 1 as a
// lowercase hex digit. The word is picked by selects: no run-time index into the array.
BH_FN uint32_t anon_digit(const uint32_t (&digest)[4], int k) {
  const int byte = k >> 1, word = byte >> 2;
  const uint32_t w = word == 0 ? digest[0] : word == 1 ? digest[1] : word == 2 ? digest[2] : digest[3];
  const uint32_t nibble = (w >> (8 * (byte & 3) + (k & 1 ? 0 : 4))) & 0xfu;
  return nibble < 10 ? '0' + nibble : 'a' - 10 + nibble;
}

// The length of the output frame of `plan`, from its fields alone (p.out_len holds the same).
BH_FN int anon_len(const AnonPlan& plan) { return canon_len(plan.p); }

// Byte `rel` of the output frame of `plan`, 0 <= rel < anon_len(plan); the kind is NM_COPY, NM_STATUS
// or NM_PROGRESS. Reads buf only inside the spans of the strings that are not replaced.
BH_FN uint32_t anon_byte(const uint8_t* __restrict__ buf, const AnonPlan& plan, int rel) {
  const Plan& p = plan.p;
  if (p.kind != NM_COPY) {
    // a replaced string is tag, 0x20, 32 digits: the id's digits start at 5 + 2
    if (p.id_off == AN_REPLACED && rel >= 7 && rel < 7 + AN_DIGITS) return anon_digit(plan.id_digest, rel - 7);
    if (p.host_off == AN_REPLACED) {
      const int k = rel - (5 + string_field_len(p.id_len) + int_field_len(p.status) + int_field_len(p.progress) + 2);
      if (k >= 0 && k < AN_DIGITS) return anon_digit(plan.host_digest, k);
    }
  }
  return canon_byte(buf, p, rel);  // every other byte is the normalise's
}

template <int DIALECT>
BH_FN int anon_classify(const uint8_t* __restrict__ buf, const int head, const int end, const bool drop,
                        const int fields, const Midstates& mids, AnonPlan& plan) {
  const int kind = norm_classify<DIALECT>(buf, head, end, drop, plan.p);
  BH_UNROLL
  for (int i = 0; i < 4; ++i) plan.id_digest[i] = plan.host_digest[i] = 0;
  if (kind != NM_STATUS && kind != NM_PROGRESS) return kind;
  Plan& p = plan.p;
  const bool id = (fields & AN_MEDIA) && p.id_len > 0, host = (fields & AN_HOST) && p.host_len > 0;
  if ((id && p.id_len > AN_STRING_MAX) || (host && p.host_len > AN_STRING_MAX)) {
    p = Plan{head, 0, 0, 0, 0, 0, NM_HOST, 0};
    return NM_HOST;
  }
  BH_NOUNROLL
  for (int s = 0; s < 2; ++s) {  // the id, then the host: one copy of the hash in the code
    const bool first = s == 0;
    if (!(first ? id : host)) continue;
    uint32_t mid[8], digest[4];
    BH_UNROLL
    for (int i = 0; i < 8; ++i) mid[i] = first ? mids.id[i] : mids.host[i];
    anon_digest(mid, buf + (first ? p.id_off : p.host_off), first ? p.id_len : p.host_len, digest);
    BH_UNROLL
    for (int i = 0; i < 4; ++i) (first ? plan.id_digest[i] : plan.host_digest[i]) = digest[i];
  }
  if (id) p.id_off = AN_REPLACED, p.id_len = AN_DIGITS;
  if (host) p.host_off = AN_REPLACED, p.host_len = AN_DIGITS;
  p.out_len = canon_len(p);
  return kind;
}

}  // namespace bh
