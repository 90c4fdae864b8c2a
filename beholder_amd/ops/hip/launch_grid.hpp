// The grid of a launch: what every launcher here asks before hipLaunchKernelGGL. Host code only.
#pragma once

namespace bh {

// The blocks that `count` items take at `per_block` items a block.
inline int blocks_of(long long count, int per_block) { return static_cast<int>((count + per_block - 1) / per_block); }

}  // namespace bh
