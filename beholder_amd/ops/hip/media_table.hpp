// The open-addressing table that groups a capture's frames by key, in one place: the hash of a key's
// bytes, the byte helpers, and the walk in which a lane claims a slot or finds its key's. Used by the
// fold (telemetry_fold.hip), the extract's host-built table (telemetry_select.hpp), the coalesce, the
// dedupe and the transitions (whose claim kernel the thin runs as it is).
//
// The first part also compiles with a plain C++17 compiler (BH_FN of telemetry_readers.hpp), so the
// host programs under tests/native/ run it under ASan/UBSan on a CPU. claim_slot is device code only.
//
// The table: `slot_mask + 1` slots, a power of two of at least twice the frames, zeroed by the
// caller. claim[slot] is 0 or 1 + the frame that claimed the slot; it is written once, by a 64-bit
// compare-and-swap, and never changes. A key's home slot is hash & hash_mask & slot_mask (hash_mask
// is all ones in production; tests pass small masks so that every probe chain collides). Whether two
// frames have the same key is decided by the caller's compare of the keys themselves, never by the
// hash alone, so no result depends on the hash being free of collisions.
//
// Visibility, the one rule every kernel here keeps: within a launch workgroups meet only in atomics
// (the claims, the cursors, the counts and winners). Every plain load reads what an earlier launch or
// the host wrote, and no kernel waits for another workgroup. A lane that meets a claim reads the
// claimant's row with a plain load, so the rows are written by an earlier launch than the one that
// claims: that is why classify (or decode, or hash) and claim are two kernels and not one.
#pragma once
#include "telemetry_readers.hpp"

namespace bh {

// murmur3's 64-bit finaliser
BH_FN uint64_t finalise64(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// FNV-1a over the n bytes at p, then the finaliser: ops/gpu_fold.py hash64 is the same. `high` is
// non-zero where a byte is >= 0x80.
BH_FN uint64_t hash64_bytes(const uint8_t* __restrict__ p, int n, uint32_t& high) {
  uint64_t h = 0xcbf29ce484222325ull;
  uint32_t any = 0;
  for (int k = 0; k < n; ++k) {
    const uint32_t b = p[k];
    any |= b;
    h = (h ^ b) * 0x100000001b3ull;
  }
  high = any & 0x80u;
  return finalise64(h);
}

BH_FN bool has_high_byte(const uint8_t* __restrict__ p, int n) {
  uint32_t any = 0;
  for (int k = 0; k < n; ++k) any |= p[k];
  return (any & 0x80u) != 0;
}

// Whether the n bytes at a and at b are equal. Both are only read, so they may be the same bytes.
BH_FN bool bytes_equal(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int n) {
  int k = 0;
  while (k < n && a[k] == b[k]) ++k;
  return k == n;
}

BH_FN uint32_t home_slot(uint64_t hash, uint64_t hash_mask, uint32_t slot_mask) {
  return static_cast<uint32_t>(hash & hash_mask) & slot_mask;
}

#ifdef __HIPCC__

struct Claim {
  uint32_t slot;  // the key's slot, always <= slot_mask
  bool claimed;   // this lane's compare-and-swap took it: the lane is the slot's one claimant
};

// The slot of frame `me - 1`'s key: walks from `home`, wrapping at the end, until it claims an empty
// slot with a compare-and-swap of `me` or meets a slot whose claimant has the same key;
// same(frame) answers that for the claimant's frame index. The keys are at most as many as the
// frames and the slots at least twice that (every entry point refuses a smaller table), so the walk
// ends before it has been round once and the bound is never reached; with it the loop ends, and
// returns a slot inside the table, whatever the table holds.
template <class Same>
__device__ __forceinline__ Claim claim_slot(unsigned long long* __restrict__ claim, uint32_t slot_mask, uint32_t home,
                                            unsigned long long me, Same same) {
  uint32_t slot = home & slot_mask;
  for (uint32_t walked = 0; walked <= slot_mask; ++walked) {
    // a claim is written once and never changes, so a non-zero value read here is final
    unsigned long long owner = __hip_atomic_load(&claim[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (owner == 0) owner = atomicCAS(&claim[slot], 0ull, me);
    if (owner == 0) return {slot, true};
    if (same(owner - 1)) return {slot, false};
    slot = (slot + 1) & slot_mask;
  }
  return {slot, false};
}

#endif  // __HIPCC__

}  // namespace bh
