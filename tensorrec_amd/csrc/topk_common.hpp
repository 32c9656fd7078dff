// tensorrec_amd/csrc/topk_common.hpp -- helpers shared by the top-k kernels: the (value desc, index asc) order of tf.nn.top_k
// (recommendation_graphs.py:80) as ONE unsigned 64-bit key, its inverse, and its wave-wide maximum by DPP.  Included by
// score_gemm.hip, score_rank.hip, topk_cascade.hip, euclid_topk.hip, by topk_filter.hip through exact_finish.hpp and by exclude.hip /
// candidate_sets.hip through csr_select.hpp.
#pragma once
#include "common.hpp"
#include <math.h>

// largest float strictly below x (x finite or -inf, never NaN): v >= x  <=>  v > float_pred(x)
__device__ __forceinline__ float float_pred(float x)
{
    const unsigned int u = __float_as_uint(x);
    if (x == -INFINITY) return x;
    if ((u << 1) == 0u) return __uint_as_float(0x80000001u);
    return __uint_as_float(x > 0.f ? u - 1u : u + 1u);
}


__device__ __forceinline__ unsigned long long merge_key(float v, int32_t id)
{
    const unsigned int u = (v == 0.f) ? 0u : __float_as_uint(v);            // -0.0 and +0.0 compare equal: one key
    const unsigned int hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)hi << 32) | (unsigned int)(~id);
}

// merge_key(-inf, 0x7fffffff): below the key of every real entry -- an empty place
constexpr unsigned long long MERGE_KEY_EMPTY = 0x007fffff80000000ull;

__device__ __forceinline__ float merge_key_value(unsigned long long key)
{
    const unsigned int hi = (unsigned int)(key >> 32);
    return __uint_as_float((hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi);
}

__device__ __forceinline__ int32_t merge_key_id(unsigned long long key) { return (int32_t)(~(unsigned int)key); }

// place `at` of a result list: the key's value and id, -inf / -1 for an empty place
__device__ __forceinline__ void store_place(float* __restrict__ ov, int32_t* __restrict__ oi, int64_t at, unsigned long long key)
{
    const bool empty = key == MERGE_KEY_EMPTY;
    ov[at] = empty ? -INFINITY : merge_key_value(key);
    oi[at] = empty ? -1 : merge_key_id(key);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long x)
{
    const int lo = (int)(unsigned int)x, hi = (int)(unsigned int)(x >> 32);
    const unsigned int tlo = (unsigned int)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const unsigned int thi = (unsigned int)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const unsigned long long t = ((unsigned long long)thi << 32) | tlo;
    return t > x ? t : x;
}

// maximum over the 64 lanes, returned in every lane
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x)
{
    x = dpp_max_u64<0x128, 0xf>(x);      // row_ror:8
    x = dpp_max_u64<0x124, 0xf>(x);      // row_ror:4
    x = dpp_max_u64<0x122, 0xf>(x);      // row_ror:2
    x = dpp_max_u64<0x121, 0xf>(x);      // row_ror:1   -> every lane: maximum of its 16-lane row
    x = dpp_max_u64<0x142, 0xa>(x);      // row_bcast15 -> rows 1, 3 also cover rows 0, 2
    x = dpp_max_u64<0x143, 0xc>(x);      // row_bcast31 -> row 3 covers all four rows
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)x, 63);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(x >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

