// tensorrec_amd/csrc/exclude.hip -- exact top-k and pair ranks with each user's "seen" items excluded (docs/exclusion.md).
//
// The exclusions of a call arrive as one CSR: ex_ptr int64 [n_rows + 1] (absolute positions into ex_idx), ex_idx int32 sorted
// ascending and de-duplicated within a row.  `rows` (nullable) maps the kernel's user / slab row r to its CSR row rows[r]
// (identity when NULL) -- the gathered users of the masked slab pass.
//
// 1. trec_exclude_filter_topk (tier 1).  One wave per user reads the user's EXACT top-k' list (value desc, index asc; places
//    beyond the catalogue -inf / -1 at the end), binary-searches every id in the user's exclusion row, and compacts the survivors
//    in order (ballot + mbcnt) into [n, k].  Correctness: the first k non-excluded entries of an exact top-k' list ARE the first k
//    non-excluded items overall -- every item missing from the list is behind its k'-th entry, hence behind every entry of the
//    list.  So a user with >= k survivors is exact; a user whose list ran out of catalogue (k'-th place -1) has no item outside
//    the list and is exact with padding.  Only a user with < k survivors AND a real k'-th item may have non-excluded items
//    beyond the list: flag[u] = 1, and the caller re-does it on the masked slab (2).
//
// 2. trec_topk_rows_excluded (tier 2).  The excluded cells of a score slab are overwritten with a sentinel NaN (bits 0xFFFFFFFF),
//    then one 1,024-thread workgroup per row selects the row's exact top-k (k <= 1024) by an order-preserving uint32 key in which
//    the sentinel is 0 (never selected), a genuine NaN is 1 (behind -inf, ties by index), -inf is 0x007FFFFF and -0.0 is +0.0.
//    Pass 1 streams the row once: every thread keeps the largest key of its strided share, and the k-th largest of those 1,024
//    maxima is a floor L <= the row's k-th largest key (k threads each hold an entry >= L).  Pass 2 appends the entries >= L
//    (typically a few times k) to LDS; a bitonic sort by (key desc, index asc) orders them and the first k are written.  Rows
//    where more than SEL_CAP entries reach L (heavy ties, few valid threads) take the exact path instead: a radix select of the
//    k-th key (11 + 11 + 10 bits), then -- if that key is tied across the k-th place -- a radix select of the index among the
//    tied entries, and one pass that appends exactly k entries.  Places beyond the row's non-excluded entries are -inf / -1.
//
// 3. trec_exclude_rank_adjust.  Pair ranks counted over every item (K2r, trec_rank_of_pairs_by_user) minus the excluded items
//    ahead of the target, with K2r's rule: counts[t] -= #{x in E_u : s_x > s_t or (s_x == s_t and x < t)}.  One wave per user;
//    the scores of both sides must come from the same chain as the count (trec_pair_score_exact, or the score slab itself).
//
// 4. trec_topk_drop_self (predict_similar_items_top_k(exclude_self=True), docs/similar_items.md).  The item-item lists are fetched
//    with one place more than asked for; one wave per row copies the [n, k + 1] list to [n, k] without the first entry whose id is
//    the row's query item.  A row that does not hold its query (k + 1 other items tie with or beat it) keeps its first k entries.
#include "csr_select.hpp"

namespace {

__device__ __forceinline__ bool row_contains(const int32_t* __restrict__ ex_idx, int64_t b, int64_t e, int32_t id)
{
    while (b < e) {
        const int64_t m = (b + e) >> 1;
        const int32_t x = ex_idx[m];
        if (x == id) return true;
        if (x < id) b = m + 1;
        else e = m;
    }
    return false;
}

__global__ __launch_bounds__(256) void exclude_filter_kernel(const float* __restrict__ in_vals, const int32_t* __restrict__ in_idx,
                                                             int kf, int64_t n_users, int k, const int64_t* __restrict__ ex_ptr,
                                                             const int32_t* __restrict__ ex_idx, const int32_t* __restrict__ rows,
                                                             float* __restrict__ out_vals, int32_t* __restrict__ out_idx,
                                                             int32_t* __restrict__ flag, int32_t* __restrict__ n_flagged)
{
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t r = rows ? (int64_t)rows[u] : u;
    const int64_t b = ex_ptr[r], e = ex_ptr[r + 1];
    const float* iv = in_vals + u * kf;
    const int32_t* ii = in_idx + u * kf;
    float* ov = out_vals + u * k;
    int32_t* oi = out_idx + u * k;
    int kept = 0;                                                   // wave-uniform
    for (int j0 = 0; j0 < kf && kept < k; j0 += TREC_WAVE) {
        const int j = j0 + lane;
        int32_t id = -1;
        float v = -INFINITY;
        if (j < kf) {
            id = ii[j];
            v = iv[j];
        }
        const bool keep = id >= 0 && !row_contains(ex_idx, b, e, id);
        const unsigned long long mask = __ballot(keep);
        const int pos = kept + (int)lanes_below(mask);
        if (keep && pos < k) {
            ov[pos] = v;
            oi[pos] = id;
        }
        kept += __popcll(mask);
    }
    for (int p = kept + lane; p < k; p += TREC_WAVE) {
        ov[p] = -INFINITY;
        oi[p] = -1;
    }
    if (lane == 0) {
        const bool redo = kept < k && ii[kf - 1] >= 0;
        flag[u] = redo ? 1 : 0;
        if (redo) atomicAdd(n_flagged, 1);
    }
}

// one wave per row: entry j of the [n_rows, kf] list goes to place j when it stands before the row's first entry holding
// self_id[row], to place j - 1 when it stands behind it, and that entry itself nowhere; without such an entry the last one falls off
__global__ __launch_bounds__(256) void drop_self_kernel(const float* __restrict__ in_vals, const int32_t* __restrict__ in_idx, int kf,
                                                        int64_t n_rows, const int32_t* __restrict__ self_id,
                                                        float* __restrict__ out_vals, int32_t* __restrict__ out_idx)
{
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_rows) return;
    const int lane = lane_id();
    const int k = kf - 1;
    const int32_t self = self_id[u];
    const float* iv = in_vals + u * kf;
    const int32_t* ii = in_idx + u * kf;
    float* ov = out_vals + u * k;
    int32_t* oi = out_idx + u * k;
    int at = kf;                                                    // wave-uniform: place of the dropped entry (kf: none so far)
    for (int j0 = 0; j0 < kf; j0 += TREC_WAVE) {
        const int j = j0 + lane;
        int32_t id = -1;
        float v = -INFINITY;
        if (j < kf) {
            id = ii[j];
            v = iv[j];
        }
        if (at == kf) {
            const unsigned long long mask = __ballot(j < kf && id >= 0 && id == self);
            if (mask != 0ull) at = j0 + (int)__builtin_ctzll(mask);
        }
        const int dst = j < at ? j : j - 1;
        if (j < kf && j != at && dst < k) {
            ov[dst] = v;
            oi[dst] = id;
        }
    }
}

__global__ __launch_bounds__(256) void exclude_mask_kernel(float* __restrict__ scores, int64_t ld, int64_t n_rows, int64_t n_cols,
                                                           const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx,
                                                           const int32_t* __restrict__ rows)
{
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_rows) return;
    const int64_t r = rows ? (int64_t)rows[u] : u;
    const int64_t b = ex_ptr[r], e = ex_ptr[r + 1];
    for (int64_t p = b + lane_id(); p < e; p += TREC_WAVE) {
        const int32_t c = ex_idx[p];
        if (c >= 0 && c < n_cols) scores[u * ld + c] = __uint_as_float(EX_SENTINEL);
    }
}

__global__ __launch_bounds__(SEL_THREADS) void topk_rows_excluded_kernel(const float* __restrict__ scores, int64_t ld, int64_t n_cols,
                                                                         int k, float* __restrict__ out_vals,
                                                                         int32_t* __restrict__ out_idx)
{
    const int64_t row = blockIdx.x;
    select_row_topk(scores + row * ld, n_cols, nullptr, k, out_vals + row * k, out_idx + row * k);
}

__global__ __launch_bounds__(256) void exclude_rank_adjust_kernel(const int64_t* __restrict__ pair_ptr, const int32_t* __restrict__ t_idx,
                                                                  const float* __restrict__ t_score, const int64_t* __restrict__ ex_ptr,
                                                                  const int32_t* __restrict__ ex_idx, const float* __restrict__ ex_score,
                                                                  int64_t n_users, int32_t* __restrict__ counts)
{
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    const int64_t p0 = pair_ptr[u], p1 = pair_ptr[u + 1], e0 = ex_ptr[u], e1 = ex_ptr[u + 1];
    if (p0 == p1 || e0 == e1) return;
    for (int64_t p = p0 + lane_id(); p < p1; p += TREC_WAVE)
        counts[p] -= listed_ahead<false>(ex_idx, ex_score, e0, e1, t_idx[p], t_score[p]);
}

}  // namespace

extern "C" int trec_exclude_filter_topk(const float* in_vals, const int32_t* in_idx, int32_t kf, int64_t n_users, int32_t k,
                                        const int64_t* ex_ptr, const int32_t* ex_idx, const int32_t* rows, float* out_vals,
                                        int32_t* out_idx, int32_t* flag, int32_t* n_flagged, void* stream)
{
    TREC_REQUIRE(in_vals && in_idx && ex_ptr && ex_idx && out_vals && out_idx && flag && n_flagged,
                 "trec_exclude_filter_topk: null pointer");
    TREC_REQUIRE(k >= 1 && kf >= k, "trec_exclude_filter_topk: need 1 <= k <= kf");
    if (n_users == 0) return TREC_OK;
    hipLaunchKernelGGL(exclude_filter_kernel, dim3((unsigned)ceil_div64(n_users, 4)), dim3(256), 0, (hipStream_t)stream, in_vals, in_idx,
                       kf, n_users, k, ex_ptr, ex_idx, rows, out_vals, out_idx, flag, n_flagged);
    return trec_check_launch("trec_exclude_filter_topk");
}

extern "C" int trec_topk_drop_self(const float* in_vals, const int32_t* in_idx, int32_t kf, int64_t n_rows, const int32_t* self_id,
                                   float* out_vals, int32_t* out_idx, void* stream)
{
    TREC_REQUIRE(in_vals && in_idx && self_id && out_vals && out_idx, "trec_topk_drop_self: null pointer");
    TREC_REQUIRE(kf >= 2 && kf <= SEL_THREADS + 1, "trec_topk_drop_self: need 2 <= kf <= 1025");
    TREC_REQUIRE(n_rows >= 0 && n_rows <= 0x7fffffffLL, "trec_topk_drop_self: bad row count");
    if (n_rows == 0) return TREC_OK;
    hipLaunchKernelGGL(drop_self_kernel, dim3((unsigned)ceil_div64(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, in_vals, in_idx, kf,
                       n_rows, self_id, out_vals, out_idx);
    return trec_check_launch("trec_topk_drop_self");
}

extern "C" int trec_topk_rows_excluded(float* scores, int64_t ld, int64_t n_rows, int64_t n_cols, int32_t k, const int64_t* ex_ptr,
                                       const int32_t* ex_idx, const int32_t* rows, float* out_vals, int32_t* out_idx, void* stream)
{
    TREC_REQUIRE(scores && out_vals && out_idx, "trec_topk_rows_excluded: null pointer");
    TREC_REQUIRE((ex_ptr == nullptr) == (ex_idx == nullptr), "trec_topk_rows_excluded: ex_ptr and ex_idx go together");
    TREC_REQUIRE(k >= 1 && k <= SEL_THREADS, "trec_topk_rows_excluded: need 1 <= k <= 1024");
    TREC_REQUIRE(n_cols >= 0 && n_cols <= 0x7fffffffLL && ld >= n_cols, "trec_topk_rows_excluded: bad row length / stride");
    TREC_REQUIRE(n_rows <= 0x7fffffffLL, "trec_topk_rows_excluded: too many rows");
    if (n_rows == 0) return TREC_OK;
    if (ex_ptr) {
        hipLaunchKernelGGL(exclude_mask_kernel, dim3((unsigned)ceil_div64(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, scores, ld,
                           n_rows, n_cols, ex_ptr, ex_idx, rows);
        const int rc = trec_check_launch("trec_topk_rows_excluded (mask)");
        if (rc != TREC_OK) return rc;
    }
    hipLaunchKernelGGL(topk_rows_excluded_kernel, dim3((unsigned)n_rows), dim3(SEL_THREADS), 0, (hipStream_t)stream, scores, ld, n_cols, k,
                       out_vals, out_idx);
    return trec_check_launch("trec_topk_rows_excluded");
}

extern "C" int trec_exclude_rank_adjust(const int64_t* pair_ptr, const int32_t* t_idx, const float* t_score, const int64_t* ex_ptr,
                                        const int32_t* ex_idx, const float* ex_score, int64_t n_users, int32_t* counts, void* stream)
{
    TREC_REQUIRE(pair_ptr && t_idx && t_score && ex_ptr && ex_idx && ex_score && counts, "trec_exclude_rank_adjust: null pointer");
    if (n_users == 0) return TREC_OK;
    hipLaunchKernelGGL(exclude_rank_adjust_kernel, dim3((unsigned)ceil_div64(n_users, 4)), dim3(256), 0, (hipStream_t)stream, pair_ptr,
                       t_idx, t_score, ex_ptr, ex_idx, ex_score, n_users, counts);
    return trec_check_launch("trec_exclude_rank_adjust");
}
