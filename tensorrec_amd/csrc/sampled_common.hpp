// tensorrec_amd/csrc/sampled_common.hpp -- what the per-user sampled-loss family shares: ONE copy of each piece that two files must
// agree on to the bit (docs/sampled_losses.md).  The family: the loss kernels of csrc/loss.hip (WMRB), csrc/loss_sampled.hip (sampled
// softmax, BPR), csrc/loss_warp.hip (WARP, with csrc/warp_common.hpp on top of this file) and the one-pass steps
// csrc/softmax_fused.hip, csrc/warp_fused.hip and csrc/bpr_fused.hip.  csrc/softmax_shared.hip and csrc/loss_dense.hip take temperature_ok alone.
#pragma once
#include "common.hpp"
#include <math.h>

#define SAMPLED_WAVE_SR 4          // samples per lane of the wave-per-user forms: S <= 64 * SAMPLED_WAVE_SR

// ---- accidental hits ----------------------------------------------------------------------------------------------------------------
// A HIT: a sample whose item is the column of an interaction of the user with pos_slot >= 0 (an interaction that is no positive hits
// nothing).  `column`, `slot`: one interaction of the user; `item`: the sample's.
__device__ __forceinline__ bool is_hit(int32_t column, int32_t slot, int32_t item) { return column == item && slot >= 0; }

// the same test against a list that holds only what can be hit: an interaction's entry is its column, or -1 (no item) where is_hit
// is false for every item
__device__ __forceinline__ int32_t hit_column(int32_t column, int32_t slot) { return is_hit(column, slot, column) ? column : -1; }

// is `item` a hit of the user row [b, e)?  A row holds a column once and sorted (sparse.Interactions): one binary search in memory
__device__ __forceinline__ bool row_is_hit(const int32_t* __restrict__ x_item, const int32_t* __restrict__ pos_slot, int64_t b, int64_t e,
                                           int32_t item)
{
    int64_t lo = b, hi = e;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (x_item[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < e && is_hit(x_item[lo], pos_slot[lo], item);
}

// The wave-per-user forms keep a row of at most 64 interactions in registers -- lane i holds column i (INT32_MAX beyond the row) and
// its pos_slot -- and search it with lane shuffles instead of memory loads: a branchless lower bound, six steps, taken by
// EVERY lane of the wave (a lane without a sample passes item = -1).  Longer rows (whole == false) take row_is_hit.  `wanted` and
// `whole` are wave-uniform.  Both pieces are shared as TEXT, the idiom of csrc/user_fused_body.hpp: as forced-inline functions they
// compiled to other code in the wave kernels (the order of the argument loads, other instructions for the last step).
struct HitRow { int32_t col; int32_t slot; bool whole; };      // (for a caller that hands the row on)

// (whole, col, slot: lvalues of the caller) = the user's row [b, e), loaded where `wanted`
#define HIT_ROW_LOAD(whole, col, slot, wanted, x_item, pos_slot, b, e, lane) \
    do {                                                                     \
        whole = (e) - (b) <= 64;                                             \
        col = 0x7fffffff;                                                    \
        slot = -1;                                                           \
        if ((wanted) && whole && (b) + (lane) < (e)) {                       \
            col = (x_item)[(b) + (lane)];                                    \
            slot = (pos_slot)[(b) + (lane)];                                 \
        }                                                                    \
    } while (0)

// hit (a bool the caller declares) = is `item` a hit of the whole row (col, slot)?  columns [0, at_row) are below the item; the last
// two shuffles by every lane as well
#define HIT_ROW_TEST(hit, col, slot, item)                                                                   \
    do {                                                                                                     \
        int at_row = 0;                                                                                      \
        _Pragma("unroll") for (int step = 32; step > 0; step >>= 1)                                          \
            if (__shfl(col, at_row + step - 1, 64) < (item)) at_row += step;                                 \
        const int32_t at_col = __shfl(col, at_row, 64), at_slot = __shfl(slot, at_row, 64);                  \
        hit = is_hit(at_col, at_slot, item);                                                                 \
    } while (0)

// hit (a bool the caller declares) = is `item` in the user's hit_column list in LDS, padded with -1 to np4 (a multiple of four)
// entries?  The test of the one-pass steps: broadcast reads, every thread walks the same addresses
#define HIT_SCAN4(hit, l_xid, np4, item)                                                                           \
    do {                                                                                                           \
        hit = false;                                                                                               \
        for (int q4 = 0; q4 < np4; q4 += 4) {                                                                      \
            const int32_t c0 = l_xid[q4], c1 = l_xid[q4 + 1], c2 = l_xid[q4 + 2], c3 = l_xid[q4 + 3];              \
            hit = hit || c0 == (item) || c1 == (item) || c2 == (item) || c3 == (item);                             \
        }                                                                                                          \
    } while (0)

// ---- sampled softmax ----------------------------------------------------------------------------------------------------------------
// the per-positive terms from the user's (M, Z): bz = b Z, D = a + b Z; forward, backward and the one-pass step share the code
__device__ __forceinline__ void ssm_terms(float yp, float M, float Z, float t, float& m, float& b, float& bz, float& D)
{
    m = fmaxf(M, yp);
    const float a = expf((yp - m) * t);
    b = expf((M - m) * t);
    bz = b * Z;
    D = a + bz;
}

// the logQ correction of a kept sample: log_s = log S, log_q = log q(item)
__device__ __forceinline__ float logq_correction(float log_s, float log_q) { return -(log_s + log_q); }

// ---- BPR ----------------------------------------------------------------------------------------------------------------------------
// one cell x = y_s - y_p: softplus(x) = max(x, 0) + log1p(e), sigma(x) = (x >= 0 ? 1 : e) / (1 + e), e = exp(-|x|); library expf /
// log1pf and a correctly rounded division.  The forward and the backward kernel of csrc/loss_sampled.hip take one function each
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float sigmoid_f(float x)
{
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

// both from ONE e, for the one-pass step (csrc/bpr_fused.hip): sp == softplus_f(x) and sg == sigmoid_f(x) bit for bit -- the same
// expressions, e shared
__device__ __forceinline__ void softplus_sigmoid_f(float x, float& sp, float& sg)
{
    const float e = expf(-fabsf(x));
    sp = fmaxf(x, 0.f) + log1pf(e);
    sg = (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

// ---- one user's samples into LDS (four loads per thread in flight, then the four LDS stores: a load -> store loop waits for every
// load on its own).  As TEXT for the kernels of loss.hip, which held it inline, and as the function the others called ----
#define FILL_SAMPLES(l_s, samp, u, S)                                                                                               \
    do {                                                                                                                            \
        for (int s0 = threadIdx.x; s0 < S; s0 += 1024) {                                                                            \
            float t[4];                                                                                                             \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) { const int s = s0 + 256 * k; t[k] = samp[u * S + (s < S ? s : S - 1)]; }  \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) { const int s = s0 + 256 * k; if (s < S) l_s[s] = t[k]; }                  \
        }                                                                                                                           \
    } while (0)

__device__ __forceinline__ void fill_samples(float* l_s, const float* __restrict__ samp, int64_t u, int32_t S) { FILL_SAMPLES(l_s, samp, u, S); }

// ---- fixed-order reductions over a 256-thread workgroup (every thread gets the result).  The two pairs sum in DIFFERENT orders, on
// purpose: each kernel keeps the order it was held to its reference with ----
__device__ __forceinline__ float wave_sum(float v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the halving tree over red[256]: thread i adds slot i + 128, then i + 64, ...
__device__ __forceinline__ float wg_sum_halving(float v, float* red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ float wg_max_halving(float v, float* red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}

// the xor butterfly inside each wave, then the four waves' results from red[4] as (0 + 1) + (2 + 3); no barrier in front: a caller
// gives every reduction of a phase its own red
__device__ __forceinline__ float wg_sum_butterfly(float v, float* red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float wg_max_butterfly(float v, float* red)
{
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- host: the launch forms of the loss kernels ---------------------------------------------------------------------------------------
// dynamic LDS above 64 KB (S close to 16384) has to be asked for
template <typename K>
static inline void allow_lds(K kernel, size_t lds)
{
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// a wave per user (four users per 256-thread workgroup) where the samples fit its registers, else a workgroup per user
static inline bool use_wave_form(int32_t n_sampled) { return n_sampled <= 64 * SAMPLED_WAVE_SR && trec_get_tuning("wmrb_wave", 1); }
static inline dim3 wave_form_grid(int64_t n_users) { return dim3((unsigned)ceil_div64(n_users * 64, 256)); }

// 1 / temperature: finite and > 0
static inline bool temperature_ok(float inv_temperature) { return isfinite(inv_temperature) && inv_temperature > 0.f; }
