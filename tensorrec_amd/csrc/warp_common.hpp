// tensorrec_amd/csrc/warp_common.hpp -- the pieces of the WARP definition that csrc/loss_warp.hip (the loss kernels) and
// csrc/warp_fused.hip (the one-pass step) must agree on to the bit: ONE copy of each (docs/sampled_losses.md, "WARP").  The hit rule
// and everything else WARP shares with the other sampled losses is csrc/sampled_common.hpp's.
#pragma once
#include "sampled_common.hpp"

// bits 0..k of a 64-bit kept word (k = 63: all)
__device__ __forceinline__ uint64_t wp_upto(int k) { return (2ull << k) - 1ull; }

// the rank weight: r = (n_items - 1) div N, L = logf((float)max(r, 1)) -- r <= 1 is an exact 0
__device__ __forceinline__ float wp_weight(int32_t n_items_m1, int32_t n_trials)
{
    const int32_t r = n_items_m1 / n_trials;
    return r > 1 ? logf((float)r) : 0.f;
}
