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
// shared_tile_hits_kernel<KT, ROLE> is the same kernel with accidental hits removed; the two share one body, softmax_shared_body.hpp.
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

// Accidental hits removed (HITS): the columns arrive SORTED by sample id, so the hits of a user are ascending, disjoint column ranges
// (shared_hit_ranges_kernel) and the users that have a sampled item as a positive are an ascending list (the transposed positives).
//   users resident    hit_rng [nnz][2] / hit_cnt [n_users]: user u's ranges [lo, hi) of sorted columns, compacted at indptr[u]
//   samples resident  sorted_ids [S], indptr_tp [n_items + 1], users_tp: the users, ascending, whose interaction with the item has
//                     pos_slot >= 0
struct SharedHits {
    const int64_t* indptr;
    const int32_t* hit_rng;
    const int32_t* hit_cnt;
    const int32_t* sorted_ids;
    const int64_t* indptr_tp;
    const int32_t* users_tp;
    int64_t n_items;
};

// (KT = 128 with the product accumulators needs more than 256 registers: one workgroup per CU there instead of spills)
template <int KT, int ROLE>
__global__ __launch_bounds__(256, (KT >= 128 && ROLE != SS_STATS) ? 1 : 2) void shared_tile_kernel(SharedParams p)
{
#define SS_HITS 0
#include "softmax_shared_body.hpp"
#undef SS_HITS
}

// the same with accidental hits removed
template <int KT, int ROLE>
__global__ __launch_bounds__(256, (KT >= 128 && ROLE != SS_STATS) ? 1 : 2) void shared_tile_hits_kernel(SharedParams p, SharedHits h)
{
#define SS_HITS 1
#include "softmax_shared_body.hpp"
#undef SS_HITS
}

// One thread per user: the sorted-column ranges [lo, hi) that hold the item of one of the user's interactions with pos_slot >= 0,
// written compacted, ascending and disjoint (x_item ascends within a row, without repeats) at hit_rng[indptr[u] + j], their number
// into hit_cnt[u].  An interaction with pos_slot < 0 is no hit; duplicate sample ids are one range.
__global__ __launch_bounds__(256) void shared_hit_ranges_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ x_item,
                                                                const int32_t* __restrict__ pos_slot,
                                                                const int32_t* __restrict__ sorted_ids, int64_t n_users, int S,
                                                                int32_t* __restrict__ hit_rng, int32_t* __restrict__ hit_cnt)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_users) return;
    const int64_t b = indptr[u], e = indptr[u + 1];
    int cnt = 0;
    for (int64_t q = b; q < e; ++q) {
        if (pos_slot[q] < 0) continue;
        const int32_t item = x_item[q];
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = (int)(((int64_t)lo + hi) >> 1);
            if (sorted_ids[mid] < item) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= S || sorted_ids[lo] != item) continue;
        int l2 = lo + 1;
        hi = S;
        while (l2 < hi) {
            const int mid = (int)(((int64_t)l2 + hi) >> 1);
            if (sorted_ids[mid] <= item) l2 = mid + 1;
            else hi = mid;
        }
        hit_rng[2 * (b + cnt)] = lo;
        hit_rng[2 * (b + cnt) + 1] = l2;
        ++cnt;
    }
    hit_cnt[u] = cnt;
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
static int ss_launch(const SharedParams& p, int n_slices, hipStream_t st, const SharedHits* h)
{
    constexpr int LDS = 2 * 32 * KT * 4 + 2 * 3 * 32 * 4;
    if (h) {                                                  // accidental hits removed
        auto kern = shared_tile_hits_kernel<KT, ROLE>;
        if (LDS > 32 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        hipLaunchKernelGGL(kern, dim3((unsigned)p.n_rblocks * (unsigned)n_slices), dim3(256), LDS, st, p, *h);
        return trec_check_launch("trec_softmax_shared_hits");
    }
    auto kern = shared_tile_kernel<KT, ROLE>;
    if (LDS > 32 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    hipLaunchKernelGGL(kern, dim3((unsigned)p.n_rblocks * (unsigned)n_slices), dim3(256), LDS, st, p);
    return trec_check_launch("trec_softmax_shared");
}

template <int ROLE>
static int ss_dispatch(const SharedParams& p, int n_slices, hipStream_t st, const SharedHits* h = nullptr)
{
    if (p.d <= 32) return ss_launch<32, ROLE>(p, n_slices, st, h);
    if (p.d <= 64) return ss_launch<64, ROLE>(p, n_slices, st, h);
    return ss_launch<128, ROLE>(p, n_slices, st, h);
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

// the launches of trec_softmax_shared_grads and trec_softmax_shared_hits_grads (h: accidental hits removed), arguments checked
static int ss_grads(const float* U, const float* Vs, const float* user_bias, const float* sample_bias, const float* sample_c,
                    const float* M, const float* tK, int64_t n_users, int32_t n_sampled, int32_t d, float inv_temperature,
                    int32_t n_slices, float* workspace, float* dU, float* dVs, float* d_sample_bias, const SharedHits* h, hipStream_t st)
{
    SharedParams p = {};
    p.d = d; p.inv_t = inv_temperature; p.cs = sample_c; p.M = M; p.tK = tK;
    // dU: users resident, every sample streamed
    p.R = U; p.T = Vs; p.n_res = n_users; p.n_str = n_sampled; p.r_bias = user_bias; p.t_bias = sample_bias;
    p.slice_len = ceil_div64(n_sampled, 32) * 32;
    p.n_rblocks = (int)ceil_div64(n_users, 128);
    p.out = dU;
    int rc = ss_dispatch<SS_DU>(p, 1, st, h);
    if (rc != TREC_OK) return rc;
    // dV, d b_s: samples resident, the users streamed in slices
    const int64_t sd = (int64_t)n_sampled * d;
    p.R = Vs; p.T = U; p.n_res = n_sampled; p.n_str = n_users; p.r_bias = sample_bias; p.t_bias = user_bias;
    p.slice_len = ceil_div64(ceil_div64(n_users, 32), n_slices) * 32;
    p.n_rblocks = (int)ceil_div64(n_sampled, 128);
    p.out = n_slices == 1 ? dVs : workspace;
    p.out_sum = d_sample_bias ? (n_slices == 1 ? d_sample_bias : workspace + (int64_t)n_slices * sd) : nullptr;
    rc = ss_dispatch<SS_DV>(p, n_slices, st, h);
    if (rc != TREC_OK || n_slices == 1) return rc;
    hipLaunchKernelGGL(shared_reduce_slices_kernel, dim3((unsigned)ceil_div64(sd, 256)), dim3(256), 0, st, workspace, sd, n_slices, dVs);
    if (d_sample_bias)
        hipLaunchKernelGGL(shared_reduce_slices_kernel, dim3((unsigned)ceil_div64(n_sampled, 256)), dim3(256), 0, st,
                           workspace + (int64_t)n_slices * sd, (int64_t)n_sampled, n_slices, d_sample_bias);
    return trec_check_launch("trec_softmax_shared_grads");
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
    return ss_grads(U, Vs, user_bias, sample_bias, sample_c, M, tK, n_users, n_sampled, d, inv_temperature, n_slices, workspace, dU, dVs,
                    d_sample_bias, nullptr, (hipStream_t)stream);
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

// ---- accidental hits removed: the columns (Vs, sample_bias, sample_c) in SORTED id order (include/tensorrec_hip.h)
extern "C" int trec_softmax_shared_hit_ranges(const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot,
                                              const int32_t* sorted_ids, int64_t n_users, int32_t n_sampled, int32_t* hit_rng,
                                              int32_t* hit_cnt, void* stream)
{
    TREC_REQUIRE(indptr && x_item && pos_slot && sorted_ids && hit_rng && hit_cnt, "trec_softmax_shared_hit_ranges: null pointer");
    TREC_REQUIRE(n_sampled >= 1, "trec_softmax_shared_hit_ranges: n_sampled must be >= 1");
    TREC_REQUIRE(n_users >= 0 && n_users < ((int64_t)1 << 31), "trec_softmax_shared_hit_ranges: n_users must fit int32");
    if (n_users == 0) return TREC_OK;
    hipLaunchKernelGGL(shared_hit_ranges_kernel, dim3((unsigned)ceil_div64(n_users, 256)), dim3(256), 0, (hipStream_t)stream, indptr,
                       x_item, pos_slot, sorted_ids, n_users, n_sampled, hit_rng, hit_cnt);
    return trec_check_launch("trec_softmax_shared_hit_ranges");
}

extern "C" int trec_softmax_shared_hits_stats(const float* U, const float* Vs, const float* user_bias, const float* sample_bias,
                                              const float* sample_c, const int64_t* indptr, const int32_t* hit_rng,
                                              const int32_t* hit_cnt, int64_t n_users, int32_t n_sampled, int32_t d,
                                              float inv_temperature, float* M, float* Z, void* stream)
{
    TREC_REQUIRE(U && Vs && M && Z && indptr && hit_rng && hit_cnt, "trec_softmax_shared_hits_stats: null pointer");
    TREC_REQUIRE(n_sampled >= 1, "trec_softmax_shared_hits_stats: n_sampled must be >= 1");
    TREC_REQUIRE(ss_shape_ok(n_sampled, d), "trec_softmax_shared_hits_stats: need d % 4 == 0 and 4 <= d <= 128");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_shared_hits_stats: inv_temperature must be finite and > 0");
    TREC_REQUIRE(n_users >= 0 && n_users < ((int64_t)1 << 31), "trec_softmax_shared_hits_stats: n_users must fit int32");
    if (n_users == 0) return TREC_OK;
    SharedParams p = {};
    p.R = U; p.T = Vs; p.n_res = n_users; p.n_str = n_sampled; p.d = d;
    p.r_bias = user_bias; p.t_bias = sample_bias; p.cs = sample_c; p.inv_t = inv_temperature;
    p.slice_len = ceil_div64(n_sampled, 32) * 32;
    p.n_rblocks = (int)ceil_div64(n_users, 128);
    p.out_M = M; p.out_Z = Z;
    SharedHits h = {};
    h.indptr = indptr; h.hit_rng = hit_rng; h.hit_cnt = hit_cnt;
    return ss_dispatch<SS_STATS>(p, 1, (hipStream_t)stream, &h);
}

extern "C" int trec_softmax_shared_hits_grads(const float* U, const float* Vs, const float* user_bias, const float* sample_bias,
                                              const float* sample_c, const float* M, const float* tK, const int64_t* indptr,
                                              const int32_t* hit_rng, const int32_t* hit_cnt, const int32_t* sorted_ids,
                                              const int64_t* indptr_tp, const int32_t* users_tp, int64_t n_items, int64_t n_users,
                                              int32_t n_sampled, int32_t d, float inv_temperature, int32_t n_slices, float* workspace,
                                              float* dU, float* dVs, float* d_sample_bias, void* stream)
{
    TREC_REQUIRE(U && Vs && M && tK && dU && dVs, "trec_softmax_shared_hits_grads: null pointer");
    TREC_REQUIRE(indptr && hit_rng && hit_cnt && sorted_ids && indptr_tp && users_tp, "trec_softmax_shared_hits_grads: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_items >= 1, "trec_softmax_shared_hits_grads: n_sampled and n_items must be >= 1");
    TREC_REQUIRE(ss_shape_ok(n_sampled, d), "trec_softmax_shared_hits_grads: need d % 4 == 0 and 4 <= d <= 128");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_shared_hits_grads: inv_temperature must be finite and > 0");
    TREC_REQUIRE(n_users >= 0 && n_users < ((int64_t)1 << 31), "trec_softmax_shared_hits_grads: n_users must fit int32");
    if (n_users == 0) return TREC_OK;
    TREC_REQUIRE(n_slices == trec_softmax_shared_slices(n_users, n_sampled, d),
                 "trec_softmax_shared_hits_grads: n_slices must be trec_softmax_shared_slices' answer");
    TREC_REQUIRE(n_slices == 1 || workspace, "trec_softmax_shared_hits_grads: more than one slice needs the workspace");
    SharedHits h = {};
    h.indptr = indptr; h.hit_rng = hit_rng; h.hit_cnt = hit_cnt;
    h.sorted_ids = sorted_ids; h.indptr_tp = indptr_tp; h.users_tp = users_tp; h.n_items = n_items;
    return ss_grads(U, Vs, user_bias, sample_bias, sample_c, M, tK, n_users, n_sampled, d, inv_temperature, n_slices, workspace, dU, dVs,
                    d_sample_bias, &h, (hipStream_t)stream);
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
