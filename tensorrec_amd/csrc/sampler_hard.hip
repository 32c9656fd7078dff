// tensorrec_amd/csrc/sampler_hard.hip -- EXTENSION (no counterpart in the reference): dynamic negative sampling.  Every user comes
// with a table of M candidate items; the kernel scores them against the CURRENT representations and returns the S the step trains
// on, the H highest-scoring first (docs/hard_negatives.md; tensorrec.HardNegativeSampler draws the candidates and calls this).
//
// THE DEFINITION (tests/hard_negative_reference.py restates it in float64).  User u, candidates c_0 .. c_{M-1}:
//   score  y_j = sum_k U[u,k] V[c_j,k] (+ item_bias[c_j]) in float32.  ONE summation order: lane l of a 32-lane subgroup holds the
//          columns 4 (32 it + l) .. + 3, it = 0 .. d / 128, and chains fmaf(u, v, acc) over them from acc = 0, `it` ascending, the four
//          columns ascending; the 32 partials p_l are then added inside each 16-lane half by the rotations 8, 4, 2, 1 as lane 15
//          of the half does -- t1 = p_15 + p_7, t2 = t1 + (p_11 + p_3), t3 = t2 + ((p_13 + p_5) + (p_9 + p_1)), t4 = t3 + (the
//          same expression one lane down, lanes 14, 6, 10, 2, 12, 4, 8, 0) --, the total is (upper half) + (lower half), and the
//          bias is added last.  Every row takes that order whatever its position: two calls give the same bits, and an item that
//          stands at two positions scores the same at both.  No float atomics.  The user bias is constant per user: not added.
//   hit    candidate j is a hit when `exclude` is set and c_j is the column of an interaction of u with pos_slot >= 0: is_hit /
//          row_is_hit of sampled_common.hpp.
//   order  every non-hit before every hit; among non-hits the larger score first, a NaN score counting as -inf (and -0 as +0), equal
//          scores by ascending position j; hits by ascending j.  The same item at two positions is two candidates.
//   out    slots 0 .. H-1: the first H candidates of that order, best first.  Slots H .. S-1: the first S - H of the REMAINING
//          candidates in the order "non-hits before hits, ascending j" -- the easy tail of a mixed sampler.  M >= S: the row is always
//          full; hits appear only where fewer than S non-hits exist, and then at the end.
//   out_scores (optional, [n_users, M]): y_j of every candidate as computed, hits and NaNs included.
//
// One 256-thread workgroup per user.  (1) candidates and, for rows of up to HN_ROW_LDS interactions, the user's row into LDS; the hit
// test, one thread per candidate (a binary search, in LDS or in memory); (2) the gather: each of the 8 subgroups takes 8 rows per
// round with all their 16-byte loads in flight (the cost of the kernel is these M rows of 4 d bytes), and lane 16 + r of the
// subgroup owns row r: it fetches the bias in the same batch and writes the row's 64-bit key; (3) a bitonic sort of the keys in LDS
// (the idiom of rank.hip), descending; (4) the first H keys are the hard slots; (5) the tail: a prefix count over the unselected
// positions.  A candidate id outside [0, n_items) is the caller's error: the result is undefined, the row address is clamped.
#include "topk_common.hpp"
#include "sampled_common.hpp"

namespace {

constexpr int HN_MAX_M = 4096;        // 4096 keys of 8 bytes: 32 KB of LDS
constexpr int HN_MAX_D = 256;
constexpr int HN_ROW_LDS = 512;       // interaction rows up to this length are searched in LDS
constexpr int HN_ROWS = 8;            // rows a subgroup gathers per round

// the key of candidate j, larger = earlier: the class (1 non-hit, 0 hit), the score in merge_key's order (0 for a hit: hits are
// ordered by position alone), then the position, descending in j
__device__ __forceinline__ unsigned long long hard_key(float y, int j, bool hit)
{
    if (y != y) y = -INFINITY;
    const unsigned long long hi = hit ? 0ull : (merge_key(y, 0) >> 32);
    return ((unsigned long long)(hit ? 0 : 1) << 63) | (hi << 31) | (unsigned long long)(0x7fffffff - j);
}

__device__ __forceinline__ int hard_key_position(unsigned long long key) { return 0x7fffffff - (int)(key & 0x7fffffffull); }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float x)
{
    const int v = __float_as_int(x);
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false));
}

// the sum over each 32-lane subgroup, in every lane of it: four rotations inside the 16-lane rows, row_bcast15 carries the lower
// row's total into the upper one, and lane 31 of the subgroup hands ITS sum to all (one order for every row)
__device__ __forceinline__ float subgroup_sum(float t, int lane)
{
    t = dpp_add<0x128, 0xf>(t);          // row_ror:8
    t = dpp_add<0x124, 0xf>(t);          // row_ror:4
    t = dpp_add<0x122, 0xf>(t);          // row_ror:2
    t = dpp_add<0x121, 0xf>(t);          // row_ror:1
    t = dpp_add<0x142, 0xa>(t);          // row_bcast15 into rows 1, 3
    return __shfl(t, (lane & 32) | 31, 64);
}

template <int ITERS>
__global__ __launch_bounds__(256) void hard_negatives_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ ib, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ xi, const int32_t* __restrict__ ps, const int32_t* __restrict__ cand, int32_t n_items, int32_t M,
    int32_t S, int32_t H, int32_t d, int32_t P, int32_t exclude, int32_t* __restrict__ out, float* __restrict__ out_scores)
{
    extern __shared__ unsigned long long l_key[];                      // [P]: P = M rounded up to a power of two
    int32_t* l_c = (int32_t*)(l_key + P);                              // [P]: the candidates
    int32_t* l_x = l_c + P;                                            // [HN_ROW_LDS]: the user's columns ...
    int32_t* l_slot = l_x + HN_ROW_LDS;                                // ... and their pos_slot
    int32_t* l_scan = l_slot + HN_ROW_LDS;                             // [8]
    unsigned char* l_st = (unsigned char*)(l_scan + 8);                // [P]: bit 0 hit, bit 1 selected as a hard slot

    const int64_t u = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int sub = tid & 31, sg = tid >> 5;                           // 8 subgroups of 32 lanes

    // ---- (1) candidates, the interaction row, the hit test ----
    int64_t b = 0, e = 0;
    if (exclude) { b = indptr[u]; e = indptr[u + 1]; }
    const bool row_lds = e - b <= HN_ROW_LDS;
    for (int j = tid; j < M; j += 256) l_c[j] = cand[u * M + j];
    if (row_lds)
        for (int q = tid; q < (int)(e - b); q += 256) { l_x[q] = xi[b + q]; l_slot[q] = ps[b + q]; }
    __syncthreads();
    for (int j = tid; j < P; j += 256) {
        bool hit = false;
        if (j < M && exclude) hit = row_lds ? row_is_hit(l_x, l_slot, 0, e - b, l_c[j]) : row_is_hit(xi, ps, b, e, l_c[j]);
        l_st[j] = hit ? 1 : 0;
        if (j >= M) l_key[j] = 0ull;                                   // below every real key
    }
    __syncthreads();

    // ---- (2) scores and keys.  Every load is unconditional, from a clamped (always valid) address, and selected afterwards ----
    f32x4 x[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * 32 + sub) * 4;
        const f32x4 v = *(const f32x4*)(U + u * d + (c < d ? c : 0));
        x[it] = (c < d) ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int own = sub - 16;                                          // lane 16 + r of a subgroup owns its row r of the round
    const unsigned int last_item = (unsigned int)(n_items - 1);
    for (int j0 = 0; j0 < M; j0 += 8 * HN_ROWS) {
        int32_t item[HN_ROWS];
#pragma unroll
        for (int r = 0; r < HN_ROWS; ++r) {
            const int j = j0 + sg + 8 * r;
            item[r] = (int32_t)min((unsigned int)l_c[j < M ? j : M - 1], last_item);
        }
        const int my_j = j0 + sg + 8 * own;
        const int32_t my_item = (int32_t)min((unsigned int)l_c[my_j < 0 ? 0 : (my_j < M ? my_j : M - 1)], last_item);
        const float my_bias = ib ? ib[my_item] : 0.f;                  // (uniform branch)
        f32x4 y[HN_ROWS][ITERS];
#pragma unroll
        for (int r = 0; r < HN_ROWS; ++r) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int c = (it * 32 + sub) * 4;
                y[r][it] = *(const f32x4*)(V + (int64_t)item[r] * d + (c < d ? c : 0));
            }
        }
        if (d < ITERS * 128) {                                         // (uniform: columns past d contribute zeros)
#pragma unroll
            for (int r = 0; r < HN_ROWS; ++r) {
#pragma unroll
                for (int it = 0; it < ITERS; ++it)
                    if ((it * 32 + sub) * 4 >= d) y[r][it] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        float mine = 0.f;
#pragma unroll
        for (int r = 0; r < HN_ROWS; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                acc = fmaf(x[it].x, y[r][it].x, acc); acc = fmaf(x[it].y, y[r][it].y, acc);
                acc = fmaf(x[it].z, y[r][it].z, acc); acc = fmaf(x[it].w, y[r][it].w, acc);
            }
            const float total = subgroup_sum(acc, lane);
            mine = (own == r) ? total : mine;
        }
        if (own >= 0 && own < HN_ROWS && my_j < M) {
            float s = mine;
            if (ib) s = s + my_bias;
            if (out_scores) out_scores[u * M + my_j] = s;
            l_key[my_j] = hard_key(s, my_j, l_st[my_j] & 1);
        }
    }
    __syncthreads();

    // ---- (3) bitonic sort of the P keys, descending (the keys are distinct: each holds its position) ----
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear: the lower place of the pair
                const unsigned long long a = l_key[i], c = l_key[i + j];
                const bool descending = (i & k) == 0;
                if ((a < c) == descending) { l_key[i] = c; l_key[i + j] = a; }
            }
            __syncthreads();
        }
    }

    // ---- (4) the hard slots ----
    for (int i = tid; i < H; i += 256) {
        const int j = hard_key_position(l_key[i]);
        out[u * S + i] = l_c[j];
        l_st[j] |= 2;
    }
    if (S == H) return;                                                // (uniform)
    __syncthreads();

    // ---- (5) the tail: the first S - H unselected positions, non-hits before hits, ascending j.  Thread t counts the positions
    //      [t per, (t + 1) per); an inclusive scan over the workgroup (non-hits in the low half of the word, hits in the high) ----
    const int per = P >= 256 ? P >> 8 : 1;
    const int j_begin = tid * per, j_end = min(j_begin + per, (int)M);
    unsigned int cnt = 0;
    for (int j = j_begin; j < j_end; ++j) {
        const unsigned int st = l_st[j];
        if (!(st & 2)) cnt += (st & 1) ? 0x10000u : 1u;
    }
    unsigned int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) l_scan[wave] = (int32_t)incl;
    __syncthreads();
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned int t = (unsigned int)l_scan[w];
        all += t;
        if (w < wave) before += t;
    }
    const unsigned int excl = before + incl - cnt;
    int at_clear = (int)(excl & 0xffffu), at_hit = (int)(all & 0xffffu) + (int)(excl >> 16);
    const int T = S - H;
    for (int j = j_begin; j < j_end; ++j) {
        const unsigned int st = l_st[j];
        if (st & 2) continue;
        const int rank = (st & 1) ? at_hit++ : at_clear++;
        if (rank < T) out[u * S + H + rank] = l_c[j];
    }
}

bool shape_ok(int32_t M, int32_t S, int32_t d) { return S >= 1 && S <= M && M <= HN_MAX_M && d >= 4 && d % 4 == 0 && d <= HN_MAX_D; }

}  // namespace

// THE statement of the coverage: 1 <= S <= M <= 4096, d a multiple of 4 in [4, 256]
extern "C" int trec_hard_negatives_supported(int32_t n_candidates, int32_t n_sampled, int32_t d)
{
    return shape_ok(n_candidates, n_sampled, d) ? 1 : 0;
}

extern "C" int trec_select_hard_negatives(const float* U, const float* V, const float* item_bias, const int64_t* indptr,
                                          const int32_t* x_item, const int32_t* pos_slot, const int32_t* candidates, int64_t n_users,
                                          int64_t n_items, int32_t n_candidates, int32_t n_sampled, int32_t n_hard, int32_t d,
                                          int32_t exclude, int32_t* out, float* out_scores, void* stream)
{
    TREC_REQUIRE(U && V && candidates && out, "trec_select_hard_negatives: null pointer");
    TREC_REQUIRE(n_users >= 0 && n_users <= 2147483647, "trec_select_hard_negatives: n_users must be in [0, 2^31)");
    TREC_REQUIRE(n_items >= 1 && n_items <= 2147483647, "trec_select_hard_negatives: n_items must be in [1, 2^31)");
    TREC_REQUIRE(n_candidates >= 1 && n_sampled >= 1 && n_sampled <= n_candidates && d >= 1,
                 "trec_select_hard_negatives: needs 1 <= n_sampled <= n_candidates and d >= 1");
    TREC_REQUIRE(n_hard >= 1 && n_hard <= n_sampled, "trec_select_hard_negatives: n_hard must be in [1, n_sampled]");
    TREC_REQUIRE(!exclude || (indptr && x_item && pos_slot), "trec_select_hard_negatives: null interaction arrays with exclude");
    if (!shape_ok(n_candidates, n_sampled, d)) {
        trec_set_last_error("trec_select_hard_negatives: configuration not covered (see trec_hard_negatives_supported)");
        return TREC_ERR_UNSUPPORTED;
    }
    if (n_users == 0) return TREC_OK;
    int32_t P = 1;
    while (P < n_candidates) P <<= 1;
    const size_t lds = (size_t)P * (8 + 4 + 1) + sizeof(int32_t) * (2 * HN_ROW_LDS + 8);
    const dim3 grid((unsigned)n_users);
    if (d <= 128)
        hipLaunchKernelGGL(hard_negatives_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, U, V, item_bias, indptr, x_item, pos_slot,
                           candidates, (int32_t)n_items, n_candidates, n_sampled, n_hard, d, P, exclude ? 1 : 0, out, out_scores);
    else
        hipLaunchKernelGGL(hard_negatives_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, U, V, item_bias, indptr, x_item, pos_slot,
                           candidates, (int32_t)n_items, n_candidates, n_sampled, n_hard, d, P, exclude ? 1 : 0, out, out_scores);
    return trec_check_launch("trec_select_hard_negatives");
}
