// tensorrec_amd/csrc/softmax_shared.hip -- the sampled softmax with ONE set of S negatives shared by every user of the step.
//
// The sample rows are one [S, d] matrix, so the [U, S] logits are a GEMM; nothing of that size is stored.  With t = 1 / temperature,
//     w_us = ((u . v_s + b_u) + b_s) t + c_s          (c_s = -log(S q(item_s)) with the logQ correction, else 0)
// and per user M_u = max_s w_us, Z_u = sum_s exp(w_us - M_u), K_u = sum_p b_p / D_p (docs/sampled_losses.md), the samples' gradient is
//     P_us = t K_u exp(w_us - M_u),   dU_u += sum_s P_us v_s,   dV_s = sum_u P_us u_u,   d b_s = sum_u P_us,   d b_u += t K_u Z_u.
//
// One kernel template, shared_tile_kernel<KT, ROLE>, in the layout of score_rank.hip: 128 RESIDENT rows per workgroup, lane & 31 =
// the wave's resident row with its operand in registers, 32-row tiles of the STREAMED side through LDS (double buffered, swizzled),
// the 32 x 32 score tile in the lane's 16 accumulators (streamed rows rc_cd_row(r, half)), fp32 operands on v_mfma_f32_32x32x2_f32.
//   SS_STATS  users resident, samples streamed: an online (m, z) per lane over its 16 accumulators per tile, the two half-waves of a row
//             combined at the end -> M_u, Z_u.  Columns s >= S enter as -inf.
//   SS_DU     users resident, samples streamed: the tile becomes P in place and is the B operand of a second MFMA whose A operand is
//             the transposed sample tile read from LDS: k-step r pairs the two half-waves' r-th columns.  dU_u += the product.
//   SS_DV     a block of 128 samples resident, a SLICE of the users streamed: the same chain, the same P (w is formed by the same
//             operations in the same order in all three roles, so it is the same float); partial [S, d] products and row sums per
//             slice, added in slice order by reduce_slices_kernel.
// Every sum has a fixed order and there are no float atomics: a call is deterministic.
#include "sampled_common.hpp"   // temperature_ok
#include <math.h>

#define SS_STATS 0
#define SS_DU 1
#define SS_DV 2
#define SS_MAX_D 128
#define SS_WS_CAP_BYTES ((int64_t)256 << 20)      // the slices' partial products: at most 256 MiB

struct SharedParams {
    const float* R;            // resident rows [n_res, d]
    const float* T;            // streamed rows [n_str, d]
    int64_t n_res, n_str;
    int d;
    const float* r_bias;       // nullable [n_res]
    const float* t_bias;       // nullable [n_str]
    const float* cs;           // nullable [S]: the samples' constants (streamed side in SS_STATS / SS_DU, resident in SS_DV)
    const float* M;            // [n_users]  (SS_DU: resident, SS_DV: streamed)
    const float* tK;           // [n_users]
    float inv_t;
    int64_t slice_len;         // streamed rows per slice (multiple of 32)
    int n_rblocks;
    float* out;                // SS_DU: dU [n_users, d], added to; SS_DV: [n_slices, S, d]
    float* out_sum;            // SS_DV: [n_slices, S]
    float* out_M;              // SS_STATS: [n_users]
    float* out_Z;
};

__device__ __forceinline__ int ss_cd_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// (KT = 128 with the product accumulators needs more than 256 registers: one workgroup per CU there instead of spills)
template <int KT, int ROLE>
__global__ __launch_bounds__(256, (KT >= 128 && ROLE != SS_STATS) ? 1 : 2) void shared_tile_kernel(SharedParams p)
{
    constexpr int BN = 32;                  // streamed rows per tile = one 32 x 32 MFMA block
    constexpr int RB = KT * 4;              // bytes per LDS row
    constexpr int CH = RB / 16;             // 16-byte chunks per row
    constexpr int KS = KT / 2;              // MFMA k-steps of the score
    constexpr int CB = KT / 32;             // 32-column blocks of the product
    constexpr int TILE_BYTES = BN * RB;
    constexpr int NSLOT = BN * CH / 256;    // 16-byte staging slots per thread per tile
    constexpr int NSIDE = 3;                // per streamed row: bias, then c (samples) or M, tK (users)
    static_assert(NSLOT >= 1, "tile too small for 256 threads");
    extern __shared__ __attribute__((aligned(16))) char ssmem[];
    float* side = (float*)(ssmem + 2 * TILE_BYTES);        // [2][NSIDE][BN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int rblock = blockIdx.x % p.n_rblocks;
    const int slice = blockIdx.x / p.n_rblocks;
    const int64_t row = ((int64_t)rblock * 4 + wave) * 32 + l31;
    const bool row_ok = row < p.n_res;
    const int64_t src = row_ok ? row : 0;
    const int d = p.d;
    const int64_t t_begin = (int64_t)slice * p.slice_len;
    const int64_t t_end = (t_begin + p.slice_len < p.n_str) ? t_begin + p.slice_len : p.n_str;
    const int n_tiles = (int)((t_end - t_begin + BN - 1) / BN);
    const float inv_t = p.inv_t;

    float rff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int k = 2 * ks + half;
        rff[ks] = (k < d) ? p.R[src * d + k] : 0.f;
    }
    const float rb = p.r_bias ? p.r_bias[src] : 0.f;
    float rM = 0.f, rK = 0.f, rc = 0.f;
    if (ROLE == SS_DU) { rM = p.M[src]; rK = row_ok ? p.tK[src] : 0.f; }
    if (ROLE == SS_DV) rc = p.cs ? p.cs[src] : 0.f;

    // ---- staging: slot q = i * 256 + tid -> (row, physical 16-byte chunk), XOR-swizzled as in score_rank.hip; chunks past d are zeros
    int slot_row[NSLOT], slot_src[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int q = i * 256 + tid;
        const int r = q / CH, pc = q % CH;
        const int sw = (CH >= 16) ? (r & 15) : ((CH == 8) ? ((r >> 1) & 7) : 0);
        slot_row[i] = r;
        slot_src[i] = (pc ^ sw) * 16;
    }
    u32x4 stage[NSLOT];
    float side_v[NSIDE] = {0.f, 0.f, 0.f};
    auto stage_issue = [&](int tile) {
        const int64_t row0 = t_begin + (int64_t)tile * BN;
        if (tid < BN) {
            int64_t g = row0 + tid;
            if (g >= p.n_str) g = p.n_str - 1;              // clamped rows are masked below
            side_v[0] = p.t_bias ? p.t_bias[g] : 0.f;
            if (ROLE == SS_DV) { side_v[1] = p.M[g]; side_v[2] = p.tK[g]; }
            else side_v[1] = p.cs ? p.cs[g] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            int64_t g = row0 + slot_row[i];
            if (g >= p.n_str) g = p.n_str - 1;
            const u32x4 zero = {0u, 0u, 0u, 0u};
            stage[i] = (slot_src[i] < d * 4) ? *(const u32x4*)((const char*)p.T + g * (int64_t)d * 4 + slot_src[i]) : zero;
        }
    };
    auto stage_commit = [&](int buf) {
        if (tid < BN) {
#pragma unroll
            for (int j = 0; j < NSIDE; ++j) side[(buf * NSIDE + j) * BN + tid] = side_v[j];
        }
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) *(u32x4*)(ssmem + buf * TILE_BYTES + (i * 256 + tid) * 16) = stage[i];
    };

    f32x16 prod[ROLE == SS_STATS ? 1 : CB];
    if (ROLE != SS_STATS) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) prod[cb][r] = 0.f;
    }
    float run_m = -INFINITY, run_z = 0.f;    // SS_STATS
    float psum = 0.f;                        // SS_DV: this lane's share of d b_s

    stage_issue(0);
    stage_commit(0);
    __syncthreads();
    for (int t = 0; t < n_tiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < n_tiles) stage_issue(t + 1);
        const char* tile = ssmem + buf * TILE_BYTES;
        const char* rowp = tile + l31 * RB;
        const int sw = (CH >= 16) ? (l31 & 15) : ((CH == 8) ? ((l31 >> 1) & 7) : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (2 * ks < d) {                                                  // (uniform: the padded k-steps add exact zeros)
                const int k = 2 * ks + half;
                const float tf = *(const float*)(rowp + (((k >> 2) ^ sw) * 16) + (k & 3) * 4);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tf, rff[ks], acc, 0, 0, 0);
            }
        }
        const float* sd = side + buf * NSIDE * BN;
        const int64_t loc0 = t_begin + (int64_t)t * BN;
        const int rows_left = (int)((p.n_str - loc0 < BN) ? (p.n_str - loc0) : BN);
        // ---- w of my resident row against the streamed rows ss_cd_row(r, half): ((dot + b_u) + b_s) t + c_s in every role
        float tile_m = -INFINITY;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const f32x4 tb4 = *(const f32x4*)(sd + 8 * q4 + 4 * half);
            const f32x4 s14 = *(const f32x4*)(sd + BN + 8 * q4 + 4 * half);
            f32x4 s24 = {0.f, 0.f, 0.f, 0.f};
            if (ROLE == SS_DV) s24 = *(const f32x4*)(sd + 2 * BN + 8 * q4 + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool valid = 8 * q4 + 4 * half + e < rows_left;
                float v = acc[4 * q4 + e];
                if (ROLE == SS_DV) {
                    v = (v + tb4[e]) + rb;
                    v = fmaf(v, inv_t, rc);
                    v = valid ? s24[e] * expf(v - s14[e]) : 0.f;
                    psum += v;
                } else {
                    v = (v + rb) + tb4[e];
                    v = fmaf(v, inv_t, s14[e]);
                    if (ROLE == SS_DU) v = valid ? rK * expf(v - rM) : 0.f;
                    else {
                        v = valid ? v : -INFINITY;
                        tile_m = fmaxf(tile_m, v);
                    }
                }
                acc[4 * q4 + e] = v;
            }
        }
        if (ROLE == SS_STATS) {
            if (tile_m > -INFINITY) {                        // (a half-wave whose columns all lie past S adds nothing)
                if (tile_m > run_m) {
                    run_z = run_z * expf(run_m - tile_m);    // (first tile: 0 * exp(-inf) = 0)
                    run_m = tile_m;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) run_z += expf(acc[r] - run_m);
            }
        } else {
            // ---- product: C[column cb * 32 + i][resident j] += sum_r T[row ss_cd_row(r, k)][column] P[k][j], k = half
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                if (cb * 32 < d) {
                    const int k = cb * 32 + l31;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rr = ss_cd_row(r, half);
                        const int swr = (CH >= 16) ? (rr & 15) : ((CH == 8) ? ((rr >> 1) & 7) : 0);
                        const float a = *(const float*)(tile + rr * RB + (((k >> 2) ^ swr) * 16) + (k & 3) * 4);
                        prod[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, acc[r], prod[cb], 0, 0, 0);
                    }
                }
            }
        }
        if (t + 1 < n_tiles) stage_commit(buf ^ 1);
        __syncthreads();
    }

    if (ROLE == SS_STATS) {
        const float om = __shfl_xor(run_m, 32, 64), oz = __shfl_xor(run_z, 32, 64);
        // half 0 first, then half 1, in both lanes: M = max, Z = z0 exp(m0 - M) + z1 exp(m1 - M); an empty half adds an exact 0
        const float m0 = half ? om : run_m, z0 = half ? oz : run_z;
        const float m1 = half ? run_m : om, z1 = half ? run_z : oz;
        const float Mx = fmaxf(m0, m1);
        const float a0 = (m0 > -INFINITY) ? z0 * expf(m0 - Mx) : 0.f;
        const float a1 = (m1 > -INFINITY) ? z1 * expf(m1 - Mx) : 0.f;
        if (row_ok && half == 0) { p.out_M[row] = Mx; p.out_Z[row] = a0 + a1; }
        return;
    }
    // ---- the product of my resident row: prod[cb][4 q + e] is column cb * 32 + 8 q + 4 half + e
    float* orow = p.out + ((ROLE == SS_DV ? (int64_t)slice * p.n_res : 0) + src) * d;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int c0 = cb * 32 + 8 * q4 + 4 * half;
            if (row_ok && c0 < d) {
                f32x4 o = {prod[cb][4 * q4], prod[cb][4 * q4 + 1], prod[cb][4 * q4 + 2], prod[cb][4 * q4 + 3]};
                if (ROLE == SS_DU) {
                    const f32x4 have = *(const f32x4*)(orow + c0);
                    o = have + o;
                }
                *(f32x4*)(orow + c0) = o;
            }
        }
    }
    if (ROLE == SS_DV) {
        const float other = __shfl_xor(psum, 32, 64);
        if (row_ok && half == 0 && p.out_sum) p.out_sum[(int64_t)slice * p.n_res + row] = psum + other;
    }
}

// out[i] = the slices' partials added in slice order
__global__ __launch_bounds__(256) void shared_reduce_slices_kernel(const float* __restrict__ ws, int64_t n, int n_slices,
                                                                   float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = ws[i];
    for (int s = 1; s < n_slices; ++s) acc += ws[(int64_t)s * n + i];
    out[i] = acc;
}

// one thread per user: loss_p, d y_p, K_u in interaction order; the samples' share of d b_u is t K_u Z_u
__global__ __launch_bounds__(256) void shared_positives_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot,
                                                               const float* __restrict__ pred, const float* __restrict__ M,
                                                               const float* __restrict__ Z, int64_t n_users, float inv_t,
                                                               float* __restrict__ loss, float* __restrict__ d_pred,
                                                               float* __restrict__ tK, float* __restrict__ d_user_bias)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_users) return;
    const int64_t b = indptr[u], e = indptr[u + 1];
    const float Mu = M[u], Zu = Z[u];
    float K = 0.f, sdy = 0.f;
    for (int64_t q = b; q < e; ++q) {
        const int32_t slot = pos_slot[q];
        if (slot < 0) { d_pred[q] = 0.f; continue; }
        const float wp = pred[q] * inv_t;
        const float m = fmaxf(Mu, wp);
        const float a = expf(wp - m), bb = expf(Mu - m);
        const float bz = bb * Zu;
        const float D = a + bz;
        loss[slot] = (m - wp) + logf(D);
        const float dy = -inv_t * (bz / D);
        d_pred[q] = dy;
        sdy += dy;
        K += bb / D;
    }
    const float tk = inv_t * K;
    tK[u] = tk;
    if (d_user_bias) d_user_bias[u] = sdy + tk * Zu;
}

// The FULL softmax (the streamed matrix is the item representation itself, S = n_items): the positives are in the denominator, so
// (M_u, Z_u) already cover them.  One thread per user: loss_p = (M_u - w_p) + log Z_u with w_p = K3's score times t, d y_p = -t,
// tK_u = t n_u / Z_u with n_u the user's interactions of pos_slot >= 0 (upstream gradient 1: G_u = n_u).  The loss does not move
// when the row is shifted: d b_u is an exact 0.
__global__ __launch_bounds__(256) void full_positives_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot,
                                                             const float* __restrict__ pred, const float* __restrict__ M,
                                                             const float* __restrict__ Z, int64_t n_users, float inv_t,
                                                             float* __restrict__ loss, float* __restrict__ d_pred,
                                                             float* __restrict__ tK, float* __restrict__ d_user_bias)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_users) return;
    const int64_t b = indptr[u], e = indptr[u + 1];
    const float Mu = M[u], Zu = Z[u];
    const float lz = logf(Zu);
    int n = 0;
    for (int64_t q = b; q < e; ++q) {
        const int32_t slot = pos_slot[q];
        if (slot < 0) { d_pred[q] = 0.f; continue; }
        const float wp = pred[q] * inv_t;
        loss[slot] = (Mu - wp) + lz;
        d_pred[q] = -inv_t;
        ++n;
    }
    tK[u] = n ? (inv_t * (float)n) / Zu : 0.f;
    if (d_user_bias) d_user_bias[u] = 0.f;
}

// dV[id] += the rows of equal ids in slot order (ids sorted stably: `order` is the slot of sorted position j); one owner per id
__global__ __launch_bounds__(256) void shared_scatter_kernel(const int32_t* __restrict__ sorted_ids, const int64_t* __restrict__ order,
                                                             const float* __restrict__ dVs, const float* __restrict__ dbs, int S, int d,
                                                             int64_t n_items, float* __restrict__ dV, float* __restrict__ d_item_bias)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cols = d + 1;                                  // column d: the bias
    if (i >= (int64_t)S * cols) return;
    const int j = (int)(i / cols), c = (int)(i % cols);
    const int32_t id = sorted_ids[j];
    if (id < 0 || id >= n_items || (j > 0 && sorted_ids[j - 1] == id)) return;
    if (c == d && (!dbs || !d_item_bias)) return;
    float acc = 0.f;
    for (int k = j; k < S && sorted_ids[k] == id; ++k) {
        const int64_t s = order[k];
        acc += (c == d) ? dbs[s] : dVs[s * d + c];
    }
    if (c == d) d_item_bias[id] += acc;
    else dV[(int64_t)id * d + c] += acc;
}

static bool ss_shape_ok(int64_t S, int d) { return S >= 1 && S < ((int64_t)1 << 31) && d >= 4 && d % 4 == 0 && d <= SS_MAX_D; }

extern "C" int trec_softmax_shared_supported(int32_t n_sampled, int32_t d) { return ss_shape_ok(n_sampled, d) ? 1 : 0; }

extern "C" int trec_softmax_shared_slices(int64_t n_users, int32_t n_sampled, int32_t d)
{
    if (n_users < 1 || !ss_shape_ok(n_sampled, d)) return -1;
    const int64_t tiles = ceil_div64(n_users, 32);
    const int64_t n_rblocks = ceil_div64(n_sampled, 128);
    int64_t n = trec_get_tuning("softmax_shared_slices", 0);
    if (n < 1) n = ceil_div64(1024, n_rblocks);                  // about four workgroups per CU
    const int64_t cap = SS_WS_CAP_BYTES / ((int64_t)n_sampled * (d + 1) * 4);
    if (n > cap) n = cap;
    if (n > tiles) n = tiles;
    if (n < 1) n = 1;
    const int64_t slice_len = ceil_div64(tiles, n) * 32;
    return (int)ceil_div64(n_users, slice_len);
}

template <int KT, int ROLE>
static int ss_launch(const SharedParams& p, int n_slices, hipStream_t st)
{
    constexpr int LDS = 2 * 32 * KT * 4 + 2 * 3 * 32 * 4;
    auto kern = shared_tile_kernel<KT, ROLE>;
    if (LDS > 32 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    hipLaunchKernelGGL(kern, dim3((unsigned)p.n_rblocks * (unsigned)n_slices), dim3(256), LDS, st, p);
    return trec_check_launch("trec_softmax_shared");
}

template <int ROLE>
static int ss_dispatch(const SharedParams& p, int n_slices, hipStream_t st)
{
    if (p.d <= 32) return ss_launch<32, ROLE>(p, n_slices, st);
    if (p.d <= 64) return ss_launch<64, ROLE>(p, n_slices, st);
    return ss_launch<128, ROLE>(p, n_slices, st);
}


extern "C" int trec_softmax_shared_stats(const float* U, const float* Vs, const float* user_bias, const float* sample_bias,
                                         const float* sample_c, int64_t n_users, int32_t n_sampled, int32_t d,
                                         float inv_temperature, float* M, float* Z, void* stream)
{
    TREC_REQUIRE(U && Vs && M && Z, "trec_softmax_shared_stats: null pointer");
    TREC_REQUIRE(n_sampled >= 1, "trec_softmax_shared_stats: n_sampled must be >= 1");
    TREC_REQUIRE(ss_shape_ok(n_sampled, d), "trec_softmax_shared_stats: need d % 4 == 0 and 4 <= d <= 128");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_shared_stats: inv_temperature must be finite and > 0");
    TREC_REQUIRE(n_users >= 0 && n_users < ((int64_t)1 << 31), "trec_softmax_shared_stats: n_users must fit int32");
    if (n_users == 0) return TREC_OK;
    SharedParams p = {};
    p.R = U; p.T = Vs; p.n_res = n_users; p.n_str = n_sampled; p.d = d;
    p.r_bias = user_bias; p.t_bias = sample_bias; p.cs = sample_c; p.inv_t = inv_temperature;
    p.slice_len = ceil_div64(n_sampled, 32) * 32;
    p.n_rblocks = (int)ceil_div64(n_users, 128);
    p.out_M = M; p.out_Z = Z;
    return ss_dispatch<SS_STATS>(p, 1, (hipStream_t)stream);
}

extern "C" int trec_softmax_shared_positives(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial, const float* M,
                                             const float* Z, int64_t n_users, float inv_temperature, float* loss, float* d_pred,
                                             float* tK, float* d_user_bias, void* stream)
{
    TREC_REQUIRE(indptr && M && Z && tK, "trec_softmax_shared_positives: null pointer");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_shared_positives: inv_temperature must be finite and > 0");
    TREC_REQUIRE(n_users >= 0, "trec_softmax_shared_positives: n_users must be >= 0");
    if (n_users == 0) return TREC_OK;
    hipLaunchKernelGGL(shared_positives_kernel, dim3((unsigned)ceil_div64(n_users, 256)), dim3(256), 0, (hipStream_t)stream, indptr,
                       pos_slot, pred_serial, M, Z, n_users, inv_temperature, loss, d_pred, tK, d_user_bias);
    return trec_check_launch("trec_softmax_shared_positives");
}

extern "C" int trec_softmax_shared_grads(const float* U, const float* Vs, const float* user_bias, const float* sample_bias,
                                         const float* sample_c, const float* M, const float* tK, int64_t n_users, int32_t n_sampled,
                                         int32_t d, float inv_temperature, int32_t n_slices, float* workspace, float* dU, float* dVs,
                                         float* d_sample_bias, void* stream)
{
    TREC_REQUIRE(U && Vs && M && tK && dU && dVs, "trec_softmax_shared_grads: null pointer");
    TREC_REQUIRE(n_sampled >= 1, "trec_softmax_shared_grads: n_sampled must be >= 1");
    TREC_REQUIRE(ss_shape_ok(n_sampled, d), "trec_softmax_shared_grads: need d % 4 == 0 and 4 <= d <= 128");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_shared_grads: inv_temperature must be finite and > 0");
    TREC_REQUIRE(n_users >= 1 && n_users < ((int64_t)1 << 31), "trec_softmax_shared_grads: n_users must lie in [1, 2^31)");
    TREC_REQUIRE(n_slices == trec_softmax_shared_slices(n_users, n_sampled, d),
                 "trec_softmax_shared_grads: n_slices must be trec_softmax_shared_slices' answer");
    TREC_REQUIRE(n_slices == 1 || workspace, "trec_softmax_shared_grads: more than one slice needs the workspace");
    hipStream_t st = (hipStream_t)stream;
    SharedParams p = {};
    p.d = d; p.inv_t = inv_temperature; p.cs = sample_c; p.M = M; p.tK = tK;
    // dU: users resident, every sample streamed
    p.R = U; p.T = Vs; p.n_res = n_users; p.n_str = n_sampled; p.r_bias = user_bias; p.t_bias = sample_bias;
    p.slice_len = ceil_div64(n_sampled, 32) * 32;
    p.n_rblocks = (int)ceil_div64(n_users, 128);
    p.out = dU;
    int rc = ss_dispatch<SS_DU>(p, 1, st);
    if (rc != TREC_OK) return rc;
    // dV, d b_s: samples resident, the users streamed in slices
    const int64_t sd = (int64_t)n_sampled * d;
    p.R = Vs; p.T = U; p.n_res = n_sampled; p.n_str = n_users; p.r_bias = sample_bias; p.t_bias = user_bias;
    p.slice_len = ceil_div64(ceil_div64(n_users, 32), n_slices) * 32;
    p.n_rblocks = (int)ceil_div64(n_sampled, 128);
    p.out = n_slices == 1 ? dVs : workspace;
    p.out_sum = d_sample_bias ? (n_slices == 1 ? d_sample_bias : workspace + (int64_t)n_slices * sd) : nullptr;
    rc = ss_dispatch<SS_DV>(p, n_slices, st);
    if (rc != TREC_OK || n_slices == 1) return rc;
    hipLaunchKernelGGL(shared_reduce_slices_kernel, dim3((unsigned)ceil_div64(sd, 256)), dim3(256), 0, st, workspace, sd, n_slices, dVs);
    if (d_sample_bias)
        hipLaunchKernelGGL(shared_reduce_slices_kernel, dim3((unsigned)ceil_div64(n_sampled, 256)), dim3(256), 0, st,
                           workspace + (int64_t)n_slices * sd, (int64_t)n_sampled, n_slices, d_sample_bias);
    return trec_check_launch("trec_softmax_shared_grads");
}

extern "C" int trec_softmax_shared_scatter(const int32_t* sorted_ids, const int64_t* order, const float* dVs, const float* d_sample_bias,
                                           int32_t n_sampled, int32_t d, int64_t n_items, float* dV, float* d_item_bias, void* stream)
{
    TREC_REQUIRE(sorted_ids && order && dVs && dV, "trec_softmax_shared_scatter: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && d >= 1 && n_items >= 1, "trec_softmax_shared_scatter: need n_sampled, d, n_items >= 1");
    hipLaunchKernelGGL(shared_scatter_kernel, dim3((unsigned)ceil_div64((int64_t)n_sampled * (d + 1), 256)), dim3(256), 0,
                       (hipStream_t)stream, sorted_ids, order, dVs, d_sample_bias, n_sampled, d, n_items, dV, d_item_bias);
    return trec_check_launch("trec_softmax_shared_scatter");
}

// the positives of the full softmax (full_positives_kernel): pred_serial = K3's scores of the interactions, (M, Z) = _stats' answer
// with Vs = the whole item representation
extern "C" int trec_softmax_full_positives(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial, const float* M,
                                           const float* Z, int64_t n_users, float inv_temperature, float* loss, float* d_pred,
                                           float* tK, float* d_user_bias, void* stream)
{
    TREC_REQUIRE(indptr && M && Z && tK, "trec_softmax_full_positives: null pointer");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_full_positives: inv_temperature must be finite and > 0");
    TREC_REQUIRE(n_users >= 0, "trec_softmax_full_positives: n_users must be >= 0");
    if (n_users == 0) return TREC_OK;
    hipLaunchKernelGGL(full_positives_kernel, dim3((unsigned)ceil_div64(n_users, 256)), dim3(256), 0, (hipStream_t)stream, indptr,
                       pos_slot, pred_serial, M, Z, n_users, inv_temperature, loss, d_pred, tK, d_user_bias);
    return trec_check_launch("trec_softmax_full_positives");
}
