// tensorrec_amd/csrc/csr_select.hpp -- device bodies shared by exclude.hip and candidate_sets.hip: the order-preserving uint32 key
// of a score, the streaming exact top-k of one row of scores by one 1,024-thread workgroup (floor, LDS collect, bitonic sort, radix
// select on overflow -- described at exclude.hip's head), and the count of a user's listed items that stand ahead of a target.
#pragma once
#include "topk_common.hpp"

namespace {

constexpr unsigned int EX_SENTINEL = 0xFFFFFFFFu;     // a negative NaN with every payload bit set: "excluded"
constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / TREC_WAVE;
constexpr int SEL_CAP = 4096;                        // LDS candidate slots of the floor path (32 KB)
constexpr int SEL_BINS = 2048;

__device__ __forceinline__ unsigned int lanes_below(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
}

__device__ __forceinline__ unsigned int sel_key(float f)
{
    unsigned int b = __float_as_uint(f);
    if (b == 0x80000000u) b = 0u;                                   // -0.0 == +0.0: one key
    if ((b & 0x7fffffffu) > 0x7f800000u) return b == EX_SENTINEL ? 0u : 1u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// f(key, column) for every entry of the row; coalesced, float4 when the row is 16-byte aligned
template <typename F>
__device__ __forceinline__ void for_each_key(const float* __restrict__ s, int64_t n, F f)
{
    int64_t done = 0;
    if ((((uintptr_t)s) & 15u) == 0) {
        const f32x4* s4 = (const f32x4*)s;
        const int64_t n4 = n >> 2;
        for (int64_t q = threadIdx.x; q < n4; q += SEL_THREADS) {
            const f32x4 x = s4[q];
            f(sel_key(x[0]), 4 * q);
            f(sel_key(x[1]), 4 * q + 1);
            f(sel_key(x[2]), 4 * q + 2);
            f(sel_key(x[3]), 4 * q + 3);
        }
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < n; i += SEL_THREADS) f(sel_key(s[i]), i);
}

// exclusive / inclusive block prefix of one value per thread (thread order)
__device__ __forceinline__ void block_scan(unsigned int x, unsigned int* wtot, unsigned int& excl, unsigned int& incl)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    unsigned int v = x;
#pragma unroll
    for (int o = 1; o < TREC_WAVE; o <<= 1) {
        const unsigned int t = __shfl_up(v, o, TREC_WAVE);
        if (lane >= o) v += t;
    }
    if (lane == TREC_WAVE - 1) wtot[w] = v;
    __syncthreads();
    unsigned int before = 0;
    for (int i = 0; i < w; ++i) before += wtot[i];
    __syncthreads();
    incl = before + v;
    excl = incl - x;
}

// the bin of a 2,048-bin histogram where the `need`-th entry lies, counting from the top bin (desc) or the bottom bin (!desc);
// every thread returns (bin, entries in the bins before it)
__device__ __forceinline__ void find_bin(const unsigned int* hist, unsigned int need, bool desc, unsigned int* wtot, unsigned int* s_res,
                                         unsigned int& bin, unsigned int& before)
{
    const unsigned int b0 = desc ? SEL_BINS - 1 - 2 * threadIdx.x : 2 * threadIdx.x;
    const unsigned int b1 = desc ? b0 - 1 : b0 + 1;
    unsigned int excl, incl;
    block_scan(hist[b0] + hist[b1], wtot, excl, incl);
    if (excl < need && need <= incl) {
        if (excl + hist[b0] >= need) {
            s_res[0] = b0;
            s_res[1] = excl;
        } else {
            s_res[0] = b1;
            s_res[1] = excl + hist[b0];
        }
    }
    __syncthreads();
    bin = s_res[0];
    before = s_res[1];
    __syncthreads();
}

// bitonic sort of cand[0, n) descending (n a power of two, <= SEL_CAP)
__device__ __forceinline__ void sort_desc(unsigned long long* cand, int n)
{
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += SEL_THREADS) {
                const int i = 2 * stride * (t / stride) + (t % stride);
                const int j = i + stride;
                const bool desc = (i & size) == 0;
                const unsigned long long a = cand[i], b = cand[j];
                if ((a < b) == desc) {
                    cand[i] = b;
                    cand[j] = a;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ unsigned long long cand_key(unsigned int key, int64_t col)
{
    return ((unsigned long long)key << 32) | (unsigned int)(~(unsigned int)col);
}

// exact top-k (value desc, id asc) of the n_cols scores at s, by the whole workgroup: entry c has the id ids[c] (ids ascending; NULL:
// c itself), an entry whose bits are EX_SENTINEL is absent.  ov / oi: the k places of this row, -inf / -1 beyond its entries.
__device__ __forceinline__ void select_row_topk(const float* __restrict__ s, int64_t n_cols, const int32_t* __restrict__ ids, int k,
                                                float* __restrict__ ov, int32_t* __restrict__ oi)
{
    __shared__ unsigned long long cand[SEL_CAP];
    __shared__ unsigned int hist[SEL_BINS];
    __shared__ unsigned int wtot[SEL_WAVES];
    __shared__ unsigned int s_res[2];
    __shared__ unsigned int s_cnt;
    const int lane = lane_id();

    // pass 1: per-thread maximum key and the number of non-excluded entries
    unsigned int tmax = 0, nvalid = 0;
    for_each_key(s, n_cols, [&](unsigned int key, int64_t) {
        tmax = key > tmax ? key : tmax;
        nvalid += key != 0u;
    });
    unsigned int ex, valid;
    block_scan(nvalid, wtot, ex, valid);
    if (threadIdx.x == SEL_THREADS - 1) s_res[0] = valid;
    __syncthreads();
    valid = s_res[0];
    const int m = (int)(valid < (unsigned int)k ? valid : (unsigned int)k);      // places that hold an item
    cand[threadIdx.x] = (unsigned long long)tmax << 32;
    __syncthreads();
    sort_desc(cand, SEL_THREADS);
    unsigned int floor_key = m > 0 ? (unsigned int)(cand[m - 1] >> 32) : 1u;
    if (floor_key == 0u || (unsigned int)m < (unsigned int)k) floor_key = 1u;   // (fewer than k valid: every valid entry)
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();

    // pass 2: the entries reaching the floor
    for_each_key(s, n_cols, [&](unsigned int key, int64_t col) {
        const bool take = key >= floor_key;
        const unsigned long long mask = __ballot(take);
        if (mask == 0ull) return;
        unsigned int base = 0;
        if (lane == __builtin_ctzll(mask)) base = atomicAdd(&s_cnt, (unsigned int)__popcll(mask));
        base = __shfl(base, __builtin_ctzll(mask), TREC_WAVE);
        const unsigned int pos = base + lanes_below(mask);
        if (take && pos < SEL_CAP) cand[pos] = cand_key(key, col);
    });
    __syncthreads();
    unsigned int c = s_cnt;
    __syncthreads();

    if (c > SEL_CAP) {
        // exact path: radix select of the m-th largest key among keys >= floor_key
        unsigned int prefix = 0, himask = 0, need = (unsigned int)m, eq = 0;
        const int shifts[3] = {21, 10, 0};
        const unsigned int dmasks[3] = {0x7ffu, 0x7ffu, 0x3ffu};
        for (int d = 0; d < 3; ++d) {
            for (int i = threadIdx.x; i < SEL_BINS; i += SEL_THREADS) hist[i] = 0;
            __syncthreads();
            const int sh = shifts[d];
            for_each_key(s, n_cols, [&](unsigned int key, int64_t) {
                if (key >= floor_key && (key & himask) == prefix) atomicAdd(&hist[(key >> sh) & dmasks[d]], 1u);
            });
            __syncthreads();
            unsigned int bin, before;
            find_bin(hist, need, true, wtot, s_res, bin, before);
            need -= before;
            eq = hist[bin];
            prefix |= bin << sh;
            himask |= dmasks[d] << sh;
            __syncthreads();
        }
        const unsigned int T = prefix;
        // the kth key is tied beyond the m-th place: the need-th smallest column among the entries equal to T
        unsigned int last_col = 0xffffffffu;
        if (eq > need) {
            unsigned int cpre = 0, cmask = 0, cneed = need;
            const int cshifts[3] = {21, 10, 0};
            const unsigned int cmasks[3] = {0x7ffu, 0x7ffu, 0x3ffu};
            for (int d = 0; d < 3; ++d) {
                for (int i = threadIdx.x; i < SEL_BINS; i += SEL_THREADS) hist[i] = 0;
                __syncthreads();
                const int sh = cshifts[d];
                for_each_key(s, n_cols, [&](unsigned int key, int64_t col) {
                    const unsigned int cc = (unsigned int)col;
                    if (key == T && (cc & cmask) == cpre) atomicAdd(&hist[(cc >> sh) & cmasks[d]], 1u);
                });
                __syncthreads();
                unsigned int bin, before;
                find_bin(hist, cneed, false, wtot, s_res, bin, before);
                cneed -= before;
                cpre |= bin << sh;
                cmask |= cmasks[d] << sh;
                __syncthreads();
            }
            last_col = cpre;
        }
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        for_each_key(s, n_cols, [&](unsigned int key, int64_t col) {
            const bool take = key > T || (key == T && (unsigned int)col <= last_col);
            const unsigned long long mask = __ballot(take);
            if (mask == 0ull) return;
            unsigned int base = 0;
            if (lane == __builtin_ctzll(mask)) base = atomicAdd(&s_cnt, (unsigned int)__popcll(mask));
            base = __shfl(base, __builtin_ctzll(mask), TREC_WAVE);
            const unsigned int pos = base + lanes_below(mask);
            if (take && pos < (unsigned int)k) cand[pos] = cand_key(key, col);
        });
        __syncthreads();
        c = s_cnt < (unsigned int)m ? s_cnt : (unsigned int)m;             // (== m by construction)
        __syncthreads();
    }

    // sort the c candidates (value desc, column asc) and write the first k places
    int n2 = 1;
    while (n2 < (int)c) n2 <<= 1;
    for (int i = (int)c + threadIdx.x; i < n2; i += SEL_THREADS) cand[i] = 0ull;
    __syncthreads();
    if (n2 > 1) sort_desc(cand, n2);
    for (int p = threadIdx.x; p < k; p += SEL_THREADS) {
        if (p < m && p < (int)c) {
            const unsigned int col = ~(unsigned int)cand[p];
            ov[p] = s[col];
            oi[p] = ids ? ids[col] : (int32_t)col;
        } else {
            ov[p] = -INFINITY;
            oi[p] = -1;
        }
    }
}

// the listed items [e0, e1) of one user that stand ahead of the target (t, st) by K2r's rule; SKIP_SELF: the target's own entry in
// the list does not count (its listed score need not be compared with st at all)
template <bool SKIP_SELF>
__device__ __forceinline__ int32_t listed_ahead(const int32_t* __restrict__ l_idx, const float* __restrict__ l_score, int64_t e0, int64_t e1,
                                                int32_t t, float st)
{
    int32_t ahead = 0;
    for (int64_t x = e0; x < e1; ++x) {
        const float sx = l_score[x];
        const int32_t ix = l_idx[x];
        ahead += ((!SKIP_SELF || ix != t) && (sx > st || (sx == st && ix < t))) ? 1 : 0;
    }
    return ahead;
}

}  // namespace
