// tensorrec_amd/csrc/exact_finish.hpp -- the ONE copy of what every exact top-k route ends in: the reference's k-ordered fp32 fmaf
// chain (oracle/tr_oracle.c:orc_score_dense), the operand row load, the staged re-scoring round, the floor rule, the flagging rule
// and the dynamic LDS layout of the finish kernels.  Users: topk_filter.hip (the finish and floor kernels), score_rank.hip
// (pair_score_exact_kernel), candidate_sets.hip (cand_chain).  The bit-identity contract with the oracle lives here: the chain in
// k order, the biases as (s + b_u) + b_i, keys by (value desc, id asc) -- files that use it are compiled -ffp-contract=off.
#pragma once
#include "topk_common.hpp"

#define FILTER_CMAX 64       // survivors per user the finish kernels can re-score (one per lane)
#ifndef FILTER_RB
#define FILTER_RB 8          // survivors re-scored per round (their fp32 rows staged in LDS)
#endif

// acc + sum_j a[j] b[j] over n terms in k order, one __fmaf_rn per term: four terms per step while vec4 (a and b 16-byte aligned),
// then -- or instead -- one by one.  The carry-in lets a caller walk a row in column blocks.
__device__ __forceinline__ float exact_chain(float acc, const float* __restrict__ a, const float* __restrict__ b, int n, bool vec4)
{
    int kk = 0;
    if (vec4) {
        for (; kk + 4 <= n; kk += 4) {
            const f32x4 a4 = *(const f32x4*)(a + kk);
            const f32x4 b4 = *(const f32x4*)(b + kk);
            acc = __fmaf_rn(a4[0], b4[0], acc); acc = __fmaf_rn(a4[1], b4[1], acc);
            acc = __fmaf_rn(a4[2], b4[2], acc); acc = __fmaf_rn(a4[3], b4[3], acc);
        }
    }
    for (; kk < n; ++kk) acc = __fmaf_rn(a[kk], b[kk], acc);
    return acc;
}

// floats 4 chunk .. 4 chunk + 3 of an operand row; !vec (a leading dimension that is no multiple of 4: rows are not 16-byte aligned):
// element by element, zero past kdim
__device__ __forceinline__ f32x4 load_row_chunk(const float* __restrict__ row, int chunk, int kdim, bool vec)
{
    const float* src = row + chunk * 4;
    if (vec) return *(const f32x4*)src;
    f32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (chunk * 4 + e < kdim) ? src[e] : 0.f;
    return w;
}

__device__ __forceinline__ bool rows_are_vec4(int64_t ld_u, int64_t ld_v) { return ((ld_v & 3) == 0) && ((ld_u & 3) == 0); }

__host__ __device__ inline int finish_kd4(int kdim) { return (kdim + 3) & ~3; }

// The dynamic LDS of the staged finish kernels, four waves per workgroup: per wave a queue of item ids, the user's row (kd4 floats)
// and FILTER_RB staged item rows.  Kernel and launcher both take their numbers from here.
struct FinishLds {
    int kd4;                 // floats staged per row (operand rows are padded to kpad >= kd4)
    int queue_slots;         // ids per wave: FILTER_CMAX survivors, or the wide finish's queue
    __host__ __device__ FinishLds(int kdim, int slots) : kd4(finish_kd4(kdim)), queue_slots(slots) {}
    __host__ __device__ int chunks() const { return kd4 >> 2; }
    __host__ __device__ int rstride() const { return kd4 + 4; }          // +4 floats: lanes r = 0..15 start on distinct 4-bank groups
    __host__ __device__ size_t bytes() const { return (size_t)4 * (queue_slots + kd4 + FILTER_RB * rstride()) * 4; }
    __device__ int32_t* queue(char* smem, int wave) const { return (int32_t*)smem + wave * queue_slots; }
    __device__ float* urow(char* smem, int wave) const { return (float*)(smem + 4 * queue_slots * 4) + (size_t)wave * kd4; }
    __device__ float* rows(char* smem, int wave) const
    {
        return (float*)(smem + 4 * queue_slots * 4) + (size_t)4 * kd4 + (size_t)wave * FILTER_RB * rstride();
    }
};
// ... and of the finish kernels that stage nothing but one user row per slot (16 slots: 16 lanes per user; 4: a wave per user)
__device__ __forceinline__ float* finish_user_row(char* smem, int slot, int kdim) { return (float*)smem + (size_t)slot * finish_kd4(kdim); }
static inline size_t finish_user_rows_bytes(int kdim, int slots) { return (size_t)slots * finish_kd4(kdim) * 4; }

static inline int finish_check_operands(const char* name, int32_t kdim, int64_t ld_users, int64_t ld_items)
{
    if (kdim >= 1 && kdim <= 1024 && ld_users >= kdim && ld_items >= finish_kd4(kdim)) return TREC_OK;
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: need kdim <= 1024 and item rows padded to a multiple of 4", name);
    trec_set_last_error(buf);
    return TREC_ERR_INVALID;
}

// One staged round: the fp32 rows of the items ids[0 .. nr) (nr <= FILTER_RB) are fetched with coalesced 16-byte loads (a row =
// `chunks` consecutive lanes) into rows[], lane r walks row r against the user's row in urow[] (LDS: a broadcast at every chain
// step), adds the biases as (s + b_u) + b_i, and lane dst0 + r takes survivor r's key into `mine`.
__device__ __forceinline__ void finish_stage_round(const int32_t* ids, int nr, int dst0, unsigned long long& mine, const float* urow,
                                                   float* rows, int lane, int kdim, int chunks, int rstride, bool vec,
                                                   const float* __restrict__ V, int64_t ld_v, int32_t item_index_base,
                                                   const float* __restrict__ item_bias, bool has_user_bias, float bu)
{
    for (int idx = lane; idx < nr * chunks; idx += 64) {
        const int r = idx / chunks, ch = idx - r * chunks;
        *(f32x4*)(rows + r * rstride + ch * 4) = load_row_chunk(V + (int64_t)(ids[r] - item_index_base) * ld_v, ch, kdim, vec);
    }
    const int32_t item = (lane < nr) ? ids[lane] : item_index_base;
    const float ibv = (item_bias && lane < nr) ? item_bias[item - item_index_base] : 0.f;   // rides with the row loads
    __builtin_amdgcn_wave_barrier();
    unsigned long long key = MERGE_KEY_EMPTY;
    if (lane < nr) {
        float acc = exact_chain(0.0f, urow, rows + lane * rstride, kdim, true);
        if (has_user_bias) acc = acc + bu;
        if (item_bias) acc = acc + ibv;
        key = merge_key(acc, item);
    }
    __builtin_amdgcn_wave_barrier();
    const int srcl = (lane - dst0) & 63;
    const unsigned int lo = (unsigned int)__shfl((int)(unsigned int)key, srcl, 64);
    const unsigned int hi = (unsigned int)__shfl((int)(unsigned int)(key >> 32), srcl, 64);
    if (lane >= dst0 && lane < dst0 + nr) mine = ((unsigned long long)hi << 32) | lo;
}

// tau - width rounded DOWN twice.  tau = -inf (fewer than k entries) keeps everything: -inf.  nan: the bound is unusable (the
// difference is a NaN); what the floor becomes then is the caller's business.
struct FloorBelow { float floor; bool nan; };
__device__ __forceinline__ FloorBelow floor_below(float tau, float width)
{
    FloorBelow r = {tau - width, false};
    if (tau == -INFINITY) r.floor = -INFINITY;
    else if (!(r.floor == r.floor)) r.nan = true;
    else r.floor = float_pred(float_pred(r.floor));
    return r;
}

// the filter's floor from the k-th largest listed key (MERGE_KEY_EMPTY: fewer than k entries, every one survives)
__device__ __forceinline__ float finish_floor_from_kth(unsigned long long kth_key, float eps)
{
    return floor_below(kth_key == MERGE_KEY_EMPTY ? -INFINITY : merge_key_value(kth_key), 2.0f * eps).floor;
}

__device__ __forceinline__ void flag_user(int32_t* __restrict__ flag, int32_t* __restrict__ n_flagged, int64_t u)
{
    if (flag[u] == 0) { flag[u] = 1; atomicAdd(n_flagged, 1); }
}
