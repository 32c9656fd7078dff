// tensorrec_amd/csrc/warp_common.hpp -- the pieces of the WARP definition that csrc/loss_warp.hip (the loss kernels) and
// csrc/warp_fused.hip (the one-pass step) must agree on to the bit: ONE copy of each (docs/sampled_losses.md, "WARP").
#pragma once
#include <math.h>
#include <stdint.h>

// bits 0..k of a 64-bit kept word (k = 63: all)
__device__ __forceinline__ uint64_t wp_upto(int k) { return (2ull << k) - 1ull; }

// the rank weight: r = (n_items - 1) div N, L = logf((float)max(r, 1)) -- r <= 1 is an exact 0
__device__ __forceinline__ float wp_weight(int32_t n_items_m1, int32_t n_trials)
{
    const int32_t r = n_items_m1 / n_trials;
    return r > 1 ? logf((float)r) : 0.f;
}

// A HIT: a sample whose item is the column of an interaction of the user with pos_slot >= 0 (an interaction that is no positive hits
// nothing).  `column`, `slot`: one interaction of the user; `item`: the sample's.
__device__ __forceinline__ bool wp_hit(int32_t column, int32_t slot, int32_t item) { return column == item && slot >= 0; }

// the same test against a list that holds only what can be hit: an interaction's entry is its column, or -1 (no item) where wp_hit
// is false for every item
__device__ __forceinline__ int32_t wp_hit_column(int32_t column, int32_t slot) { return wp_hit(column, slot, column) ? column : -1; }
