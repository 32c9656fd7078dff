// tensorrec_amd/csrc/loss_sampled.hip -- K6s: sampled softmax (InfoNCE) and BPR, forward + backward.
//
// Neither loss exists in the reference (tensorrec/loss_graphs.py has no such class): there is no TF op chain to restate, the
// formulas below are the definition.  Conventions and layout are K6's (loss.hip): interactions are CSR over users, pos_slot[p] is
// the slot of interaction p in the compact [P+] vector or -1 (ignored, d pred = 0), one wave (S <= 256) or one 256-thread workgroup
// (S <= 16384) owns a user, nothing of size P+ x S is ever stored, no atomics and a fixed summation order.
// t = 1 / temperature, y_p a positive's prediction, y_s a sample's prediction of the same user.
//
// Sampled softmax       loss_p = log(1 + sum_s exp((y_s - y_p) t))
//     per user          M = max_s y_s,  Z = sum_s exp((y_s - M) t)  (>= 1)              -- stored [n_users] for the backward pass
//     per positive      m = max(M, y_p),  a = exp((y_p - m) t),  b = exp((M - m) t),  D = a + b Z  (>= 1)
//                       loss_p = (m - y_p) t + log D                                    -- both terms >= 0, no overflow, no cancellation
//     backward          d y_p = -go_p t b Z / D,   d y_us = t exp((y_us - M) t) K_u,   K_u = sum_{p of u, positive} go_p b_p / D_p
//     The sums factor per user: O(S + n_u) work per user in both directions.
// BPR                   loss_p = (1/S) sum_s softplus(y_s - y_p),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
//     backward          d y_p = -(go_p / S) sum_s sigma(y_s - y_p),   d y_us = (1/S) sum_p go_p sigma(y_us - y_p)
//                       sigma(x) = x >= 0 ? 1 / (1 + e) : e / (1 + e),  e = exp(-|x|)
//     O(S n_u) like WMRB, and WMRB's loop structure: threads own samples and loop over the staged positives in order.
#include "sampled_common.hpp"   // the hit rule, ssm_terms, logq_correction, softplus_f / sigmoid_f, fill_samples, the reductions, the launch forms

#define SL_MAX_POS_LDS 1024        // positives of one user staged per pass (workgroup BPR backward)

// ---- the adjusted forms: accidental hits and the logQ correction ---------------------------------------------------------------
// A sample of user u is a HIT when its item is the column of one of the user's interactions with pos_slot >= 0 (a value <= 0 is no
// hit).  A row holds a column once and sorted (sparse.Interactions), so the thread that owns the sample does one binary search over
// x_item[b..e) and checks pos_slot of the match: once per sample per kernel, shared by all the user's positives.  A hit becomes
// padding (-inf): it never wins a maximum, adds exp(-inf) = 0 / softplus(-inf) = 0 / sigma(-inf) = 0, and its gradient is an exact 0.
// The correction of a kept sample is c = -(log S + log q(item)), log q from the [n_items] table or the scalar of the uniform case;
// an id outside [0, n_items) is not looked up (c = 0).  Both are recomputed by the backward pass: nothing of size [U, S] is stored.
#define SL_ADJ_LOGQ 1
#define SL_ADJ_HITS 2

struct SlAdj {
    const int32_t* x_item;      // CSR column ids (int32, sorted within a row); needed for SL_ADJ_HITS
    const int32_t* samples;     // [n_users, S] sampled item ids; needed when a flag is set
    const float* log_q;         // [n_items] log q, or NULL: log_q_uniform for every item
    float log_q_uniform;
    float log_s;                // log S
    int32_t n_items;
    int32_t flags;
};

// prediction y of the sample at flat position `at` of user row [b, e): -inf when it is a hit, else y with its correction in c
__device__ __forceinline__ float sl_adjust(const SlAdj& adj, const int32_t* __restrict__ pos_slot, int64_t b, int64_t e, int64_t at,
                                           float y, float& c)
{
    c = 0.f;
    if (adj.flags == 0) return y;
    const int32_t item = adj.samples[at];
    if ((adj.flags & SL_ADJ_HITS) && row_is_hit(adj.x_item, pos_slot, b, e, item)) return -INFINITY;
    if ((adj.flags & SL_ADJ_LOGQ) && (uint32_t)item < (uint32_t)adj.n_items)
        c = logq_correction(adj.log_s, adj.log_q ? adj.log_q[item] : adj.log_q_uniform);
    return y;
}

// The wave-per-user forms search a row of at most 64 interactions in registers (HitRow).  Every lane of the wave calls sl_adjust_wave
// (a lane without a sample passes live = false and gets its -inf padding back); longer rows take the binary search in memory.  The
// conditions on adj.flags and row.whole are wave-uniform.
__device__ __forceinline__ HitRow sl_row_wave(const SlAdj& adj, const int32_t* __restrict__ pos_slot, int64_t b, int64_t e, int lane)
{
    HitRow row;
    HIT_ROW_LOAD(row.whole, row.col, row.slot, adj.flags & SL_ADJ_HITS, adj.x_item, pos_slot, b, e, lane);
    return row;
}

__device__ __forceinline__ float sl_adjust_wave(const SlAdj& adj, const int32_t* __restrict__ pos_slot, int64_t b, int64_t e,
                                                const HitRow& row, bool live, int64_t at, float y, float& c)
{
    c = 0.f;
    if (adj.flags == 0) return y;
    const int32_t item = live ? adj.samples[at] : -1;
    if (adj.flags & SL_ADJ_HITS) {
        bool hit;
        if (row.whole) {
            HIT_ROW_TEST(hit, row.col, row.slot, item);
        } else {
            hit = live && row_is_hit(adj.x_item, pos_slot, b, e, item);
        }
        if (hit) return -INFINITY;
    }
    if (live && (adj.flags & SL_ADJ_LOGQ) && (uint32_t)item < (uint32_t)adj.n_items)
        c = logq_correction(adj.log_s, adj.log_q ? adj.log_q[item] : adj.log_q_uniform);
    return y;
}

// ---- sampled softmax: wave per user (S <= 256) ----------------------------------------------------------------
// Samples sit in <= 4 registers per lane (sample s = r * 64 + lane), padded with -inf: the padding never wins the maximum
// (S >= 1) and adds exp(-inf) = 0 to Z.  The positives are taken 64 per pass, one per lane: O(1) work each.
__global__ __launch_bounds__(256) void ssm_fwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int64_t n_users, int32_t S, float t, float* __restrict__ loss,
    float* __restrict__ Mu, float* __restrict__ Zu)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    float ys[SAMPLED_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
    float M = fmaxf(fmaxf(ys[0], ys[1]), fmaxf(ys[2], ys[3]));
    for (int off = 32; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
    float z = 0.f;
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) z += expf((ys[r] - M) * t);
    const float Z = wave_sum(z);
    if (lane == 0) { Mu[u] = M; Zu[u] = Z; }
    for (int64_t p = b + lane; p < e; p += 64) {
        const int32_t slot = pos_slot[p];
        if (slot < 0) continue;
        const float yp = pred[p];
        float m, bb, bz, D;
        ssm_terms(yp, M, Z, t, m, bb, bz, D);
        loss[slot] = (m - yp) * t + logf(D);
    }
}

__global__ __launch_bounds__(256) void ssm_bwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ Mu, const float* __restrict__ Zu,
    const float* __restrict__ grad_out, int64_t n_users, int32_t S, float t, float* __restrict__ d_pred,
    float* __restrict__ d_samp)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    float K = 0.f, M = 0.f;
    bool any = false;                                              // wave-uniform: does the user hold a positive?
    if (b != e) {                                                  // (M, Z are written for users with interactions only)
        M = Mu[u];
        const float Z = Zu[u];
        for (int64_t p0 = b; p0 < e; p0 += 64) {
            const int np = (int)((e - p0 < 64) ? (e - p0) : 64);
            float term = 0.f;
            bool is_pos = false;
            if (lane < np) {
                const int32_t slot = pos_slot[p0 + lane];
                float dp = 0.f;
                if (slot >= 0) {
                    const float go = grad_out[slot];
                    float m, bb, bz, D;
                    ssm_terms(pred[p0 + lane], M, Z, t, m, bb, bz, D);
                    dp = -(go * t) * (bz / D);
                    term = (go * bb) / D;
                    is_pos = true;
                }
                d_pred[p0 + lane] = dp;
            }
            any = any || (__builtin_amdgcn_ballot_w64(is_pos) != 0ull);
            for (int q = 0; q < np; ++q) K += __shfl(term, q, 64); // interaction order; a non-positive adds an exact 0
        }
    }
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
        const int s = r * 64 + lane;
        if (s < S) d_samp[u * S + s] = any ? (t * expf((samp[u * S + s] - M) * t)) * K : 0.f;
    }
}

// ---- sampled softmax: workgroup per user (S <= 16384) -----------------------------------------------------------
// Samples sit in LDS; M, Z and K are fixed-tree reductions over per-thread chains (thread i: s or p = i, i + 256, ...).
__global__ __launch_bounds__(256) void ssm_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int32_t S, float t, float* __restrict__ loss, float* __restrict__ Mu,
    float* __restrict__ Zu)
{
    extern __shared__ float lds[];           // [S] sampled predictions of this user
    __shared__ float red[256];
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    fill_samples(lds, samp, u, S);
    __syncthreads();
    float mx = -INFINITY;
    for (int s = threadIdx.x; s < S; s += 256) mx = fmaxf(mx, lds[s]);
    const float M = wg_max_halving(mx, red);
    float z = 0.f;
    for (int s = threadIdx.x; s < S; s += 256) z += expf((lds[s] - M) * t);
    const float Z = wg_sum_halving(z, red);
    if (threadIdx.x == 0) { Mu[u] = M; Zu[u] = Z; }
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int32_t slot = pos_slot[p];
        if (slot < 0) continue;
        const float yp = pred[p];
        float m, bb, bz, D;
        ssm_terms(yp, M, Z, t, m, bb, bz, D);
        loss[slot] = (m - yp) * t + logf(D);
    }
}

__global__ __launch_bounds__(256) void ssm_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ Mu, const float* __restrict__ Zu,
    const float* __restrict__ grad_out, int32_t S, float t, float* __restrict__ d_pred, float* __restrict__ d_samp)
{
    __shared__ float red[256];
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    float M = 0.f, Z = 1.f, k = 0.f, n_pos = 0.f;
    if (b != e) { M = Mu[u]; Z = Zu[u]; }
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int32_t slot = pos_slot[p];
        float dp = 0.f;
        if (slot >= 0) {
            const float go = grad_out[slot];
            float m, bb, bz, D;
            ssm_terms(pred[p], M, Z, t, m, bb, bz, D);
            dp = -(go * t) * (bz / D);
            k += (go * bb) / D;
            n_pos += 1.f;
        }
        d_pred[p] = dp;
    }
    const float K = wg_sum_halving(k, red);
    const bool any = wg_max_halving(n_pos, red) > 0.f;
    for (int s = threadIdx.x; s < S; s += 256)
        d_samp[u * S + s] = any ? (t * expf((samp[u * S + s] - M) * t)) * K : 0.f;
}

// ---- adjusted sampled softmax --------------------------------------------------------------------------------------------
//     loss_p = log(1 + sum_{s kept} exp((y_s - y_p) t + c_s)),   kept: not a hit;   c_s as in sl_adjust (0 without the correction)
//     per user          R = max_{kept} y_s;   w_s = (y_s - R) t + c_s;   M = max_{kept} w_s;   Z = sum_{kept} exp(w_s - M)  (>= 1)
//     per positive      w_p = (y_p - R) t;  the terms of ssm_terms on (w_p, M, Z) with t = 1:   loss_p = (m - w_p) + log D
//     backward          d y_p = -go_p t b Z / D,   d y_us = t exp(w_s - M) K_u for a kept sample, an exact 0 for a hit
// Only the negatives carry c.  R keeps every argument a difference of predictions as in the plain kernels (scores far from 0 lose
// nothing); M is the maximum of the corrected logits, so no exponential overflows.  (R, M, Z) are stored per user for the backward
// pass, which recomputes the mask and c.  A user whose samples are all hits has R = -inf: loss_p = 0, d y_p = 0, a zero d_samp row.
__global__ __launch_bounds__(256) void ssm_adj_fwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int64_t n_users, int32_t S, float t, float* __restrict__ loss, float* __restrict__ Ru,
    float* __restrict__ Mu, float* __restrict__ Zu, SlAdj adj)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    const HitRow row = sl_row_wave(adj, pos_slot, b, e, lane);
    float ys[SAMPLED_WAVE_SR], cs[SAMPLED_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
        const bool live = r * 64 + lane < S;
        ys[r] = sl_adjust_wave(adj, pos_slot, b, e, row, live, u * S + r * 64 + lane, live ? samp[u * S + r * 64 + lane] : -INFINITY, cs[r]);
    }
    float R = fmaxf(fmaxf(ys[0], ys[1]), fmaxf(ys[2], ys[3]));
    for (int off = 32; off > 0; off >>= 1) R = fmaxf(R, __shfl_xor(R, off, 64));
    const bool none = R == -INFINITY;                              // wave-uniform: every sample is a hit
    float M = 0.f, Z = 0.f;
    if (!none) {
        float w[SAMPLED_WAVE_SR];
#pragma unroll
        for (int r = 0; r < SAMPLED_WAVE_SR; ++r) w[r] = (ys[r] - R) * t + cs[r];      // -inf for a hit or padding
        M = fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
        for (int off = 32; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
        float z = 0.f;
#pragma unroll
        for (int r = 0; r < SAMPLED_WAVE_SR; ++r) z += expf(w[r] - M);
        Z = wave_sum(z);
    }
    if (lane == 0) { Ru[u] = R; Mu[u] = M; Zu[u] = Z; }
    for (int64_t p = b + lane; p < e; p += 64) {
        const int32_t slot = pos_slot[p];
        if (slot < 0) continue;
        float lo = 0.f;
        if (!none) {
            const float wp = (pred[p] - R) * t;
            float m, bb, bz, D;
            ssm_terms(wp, M, Z, 1.0f, m, bb, bz, D);
            lo = (m - wp) + logf(D);
        }
        loss[slot] = lo;
    }
}

__global__ __launch_bounds__(256) void ssm_adj_bwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ Ru, const float* __restrict__ Mu, const float* __restrict__ Zu,
    const float* __restrict__ grad_out, int64_t n_users, int32_t S, float t, float* __restrict__ d_pred,
    float* __restrict__ d_samp, SlAdj adj)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    float K = 0.f, M = 0.f, R = 0.f;
    bool any = false;                                              // wave-uniform: a positive and a kept sample
    if (b != e) {
        R = Ru[u];
        M = Mu[u];
        const float Z = Zu[u];
        const bool none = R == -INFINITY;
        for (int64_t p0 = b; p0 < e; p0 += 64) {
            const int np = (int)((e - p0 < 64) ? (e - p0) : 64);
            float term = 0.f;
            bool is_pos = false;
            if (lane < np) {
                const int32_t slot = pos_slot[p0 + lane];
                float dp = 0.f;
                if (slot >= 0 && !none) {
                    const float go = grad_out[slot];
                    float m, bb, bz, D;
                    ssm_terms((pred[p0 + lane] - R) * t, M, Z, 1.0f, m, bb, bz, D);
                    dp = -(go * t) * (bz / D);
                    term = (go * bb) / D;
                    is_pos = true;
                }
                d_pred[p0 + lane] = dp;
            }
            any = any || (__builtin_amdgcn_ballot_w64(is_pos) != 0ull);
            for (int q = 0; q < np; ++q) K += __shfl(term, q, 64); // interaction order; a non-positive adds an exact 0
        }
    }
    const HitRow row = sl_row_wave(adj, pos_slot, b, e, lane);
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
        const int s = r * 64 + lane;
        if (r * 64 >= S) continue;                                 // (wave-uniform)
        float d = 0.f;
        if (any) {                                                 // (wave-uniform: every lane takes part in the row search)
            float c;
            const float y = sl_adjust_wave(adj, pos_slot, b, e, row, s < S, u * S + s, s < S ? samp[u * S + s] : -INFINITY, c);
            if (y != -INFINITY) d = (t * expf(((y - R) * t + c) - M)) * K;
        }
        if (s < S) d_samp[u * S + s] = d;
    }
}

// workgroup per user: LDS holds the samples' (masked) predictions, then their corrected logits w in place, and the corrections
__global__ __launch_bounds__(256) void ssm_adj_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int32_t S, float t, float* __restrict__ loss, float* __restrict__ Ru, float* __restrict__ Mu,
    float* __restrict__ Zu, SlAdj adj)
{
    extern __shared__ float lds[];           // [S] y, then w | [S] c
    __shared__ float red[256];
    float* l_w = lds;
    float* l_c = lds + S;
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    float mx = -INFINITY;
    for (int s = threadIdx.x; s < S; s += 256) {                   // (a thread reads back only the slots it wrote)
        float c;
        const float y = sl_adjust(adj, pos_slot, b, e, u * S + s, samp[u * S + s], c);
        l_w[s] = y;
        l_c[s] = c;
        mx = fmaxf(mx, y);
    }
    const float R = wg_max_halving(mx, red);
    const bool none = R == -INFINITY;
    float M = 0.f, Z = 0.f;
    if (!none) {
        mx = -INFINITY;
        for (int s = threadIdx.x; s < S; s += 256) {
            const float w = (l_w[s] - R) * t + l_c[s];
            l_w[s] = w;
            mx = fmaxf(mx, w);
        }
        M = wg_max_halving(mx, red);
        float z = 0.f;
        for (int s = threadIdx.x; s < S; s += 256) z += expf(l_w[s] - M);
        Z = wg_sum_halving(z, red);
    }
    if (threadIdx.x == 0) { Ru[u] = R; Mu[u] = M; Zu[u] = Z; }
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int32_t slot = pos_slot[p];
        if (slot < 0) continue;
        float lo = 0.f;
        if (!none) {
            const float wp = (pred[p] - R) * t;
            float m, bb, bz, D;
            ssm_terms(wp, M, Z, 1.0f, m, bb, bz, D);
            lo = (m - wp) + logf(D);
        }
        loss[slot] = lo;
    }
}

__global__ __launch_bounds__(256) void ssm_adj_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ Ru, const float* __restrict__ Mu, const float* __restrict__ Zu,
    const float* __restrict__ grad_out, int32_t S, float t, float* __restrict__ d_pred, float* __restrict__ d_samp, SlAdj adj)
{
    __shared__ float red[256];
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    float R = -INFINITY, M = 0.f, Z = 1.f, k = 0.f, n_pos = 0.f;
    if (b != e) { R = Ru[u]; M = Mu[u]; Z = Zu[u]; }
    const bool none = R == -INFINITY;
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const int32_t slot = pos_slot[p];
        float dp = 0.f;
        if (slot >= 0 && !none) {
            const float go = grad_out[slot];
            float m, bb, bz, D;
            ssm_terms((pred[p] - R) * t, M, Z, 1.0f, m, bb, bz, D);
            dp = -(go * t) * (bz / D);
            k += (go * bb) / D;
            n_pos += 1.f;
        }
        d_pred[p] = dp;
    }
    const float K = wg_sum_halving(k, red);
    const bool any = wg_max_halving(n_pos, red) > 0.f;
    for (int s = threadIdx.x; s < S; s += 256) {
        float d = 0.f;
        if (any) {
            float c;
            const float y = sl_adjust(adj, pos_slot, b, e, u * S + s, samp[u * S + s], c);
            if (y != -INFINITY) d = (t * expf(((y - R) * t + c) - M)) * K;
        }
        d_samp[u * S + s] = d;
    }
}

// ---- BPR ---------------------------------------------------------------------------------------------------------------
// The kernels live in loss_sampled_bpr_body.hpp and are compiled twice: the plain ones, and the ones that drop accidental hits.
#define SL_ADJ 0
#include "loss_sampled_bpr_body.hpp"
#undef SL_ADJ
#define SL_ADJ 1
#include "loss_sampled_bpr_body.hpp"
#undef SL_ADJ

// ---- entry points ------------------------------------------------------------------------------------------------
extern "C" int trec_sampled_softmax_fwd(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial,
                                        const float* sample_pred, int64_t n_users, int32_t n_sampled, float inv_temperature,
                                        float* loss, float* row_max, float* row_sum, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && loss && row_max && row_sum,
                 "trec_sampled_softmax_fwd: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, "trec_sampled_softmax_fwd: n_sampled must be in [1, 16384]");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_sampled_softmax_fwd: inv_temperature must be finite and > 0");
    if (n_users == 0) return TREC_OK;
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(ssm_fwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, n_users, n_sampled, inv_temperature, loss, row_max, row_sum);
        return trec_check_launch("trec_sampled_softmax_fwd");
    }
    const size_t lds = sizeof(float) * (size_t)n_sampled;
    allow_lds(ssm_fwd_kernel, lds + 1024);
    hipLaunchKernelGGL(ssm_fwd_kernel, dim3((unsigned)n_users), dim3(256), lds, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, n_sampled, inv_temperature, loss, row_max, row_sum);
    return trec_check_launch("trec_sampled_softmax_fwd");
}

extern "C" int trec_sampled_softmax_bwd(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial,
                                        const float* sample_pred, const float* row_max, const float* row_sum,
                                        const float* grad_loss, int64_t n_users, int32_t n_sampled, float inv_temperature,
                                        float* d_pred_serial, float* d_sample_pred, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && row_max && row_sum && grad_loss && d_pred_serial && d_sample_pred,
                 "trec_sampled_softmax_bwd: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, "trec_sampled_softmax_bwd: n_sampled must be in [1, 16384]");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_sampled_softmax_bwd: inv_temperature must be finite and > 0");
    if (n_users == 0) return TREC_OK;
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(ssm_bwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, row_max, row_sum, grad_loss, n_users, n_sampled,
                           inv_temperature, d_pred_serial, d_sample_pred);
        return trec_check_launch("trec_sampled_softmax_bwd");
    }
    hipLaunchKernelGGL(ssm_bwd_kernel, dim3((unsigned)n_users), dim3(256), 0, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, row_max, row_sum, grad_loss, n_sampled, inv_temperature, d_pred_serial, d_sample_pred);
    return trec_check_launch("trec_sampled_softmax_bwd");
}

extern "C" int trec_bpr_fwd(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial, const float* sample_pred,
                            int64_t n_users, int32_t n_sampled, float* loss, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && loss, "trec_bpr_fwd: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, "trec_bpr_fwd: n_sampled must be in [1, 16384]");
    if (n_users == 0) return TREC_OK;
    const float inv_s = 1.0f / (float)n_sampled;
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(bpr_fwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, n_users, n_sampled, inv_s, loss);
        return trec_check_launch("trec_bpr_fwd");
    }
    const size_t lds = sizeof(float) * (size_t)n_sampled;
    allow_lds(bpr_fwd_kernel, lds);
    hipLaunchKernelGGL(bpr_fwd_kernel, dim3((unsigned)n_users), dim3(256), lds, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, n_sampled, inv_s, loss);
    return trec_check_launch("trec_bpr_fwd");
}

extern "C" int trec_bpr_bwd(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial, const float* sample_pred,
                            const float* grad_loss, int64_t n_users, int32_t n_sampled, float* d_pred_serial,
                            float* d_sample_pred, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && grad_loss && d_pred_serial && d_sample_pred,
                 "trec_bpr_bwd: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, "trec_bpr_bwd: n_sampled must be in [1, 16384]");
    if (n_users == 0) return TREC_OK;
    const float inv_s = 1.0f / (float)n_sampled;
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(bpr_bwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, grad_loss, n_users, n_sampled, inv_s, d_pred_serial,
                           d_sample_pred);
        return trec_check_launch("trec_bpr_bwd");
    }
    const size_t lds = sizeof(float) * ((size_t)n_sampled + 2 * SL_MAX_POS_LDS);
    allow_lds(bpr_bwd_kernel, lds);
    hipLaunchKernelGGL(bpr_bwd_kernel, dim3((unsigned)n_users), dim3(256), lds, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, grad_loss, n_sampled, inv_s, d_pred_serial, d_sample_pred);
    return trec_check_launch("trec_bpr_bwd");
}

// ---- entry points of the adjusted forms ---------------------------------------------------------------------------------
static inline SlAdj make_adj(const int32_t* x_item, const int32_t* samples, const float* log_q, float log_q_uniform, int64_t n_items,
                             int32_t n_sampled, int32_t log_q_correction, int32_t remove_hits)
{
    SlAdj adj;
    adj.x_item = x_item;
    adj.samples = samples;
    adj.log_q = log_q;
    adj.log_q_uniform = log_q_uniform;
    adj.log_s = (float)log((double)n_sampled);
    adj.n_items = (int32_t)n_items;
    adj.flags = (log_q_correction ? SL_ADJ_LOGQ : 0) | (remove_hits ? SL_ADJ_HITS : 0);
    return adj;
}

#define SL_ADJ_REQUIRE(name)                                                                                                            \
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, name ": n_sampled must be in [1, 16384]");                                       \
    TREC_REQUIRE(!(log_q_correction || remove_hits) || samples, name ": null samples with an option that needs them");                  \
    TREC_REQUIRE(!remove_hits || x_item, name ": null x_item with remove_hits");                                                        \
    TREC_REQUIRE(!log_q_correction || (n_items >= 1 && n_items <= 2147483647), name ": n_items must be in [1, 2^31) with log_q_correction")

extern "C" int trec_sampled_softmax_adj_fwd(const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot,
                                            const float* pred_serial, const float* sample_pred, const int32_t* samples,
                                            const float* log_q, float log_q_uniform, int64_t n_users, int64_t n_items,
                                            int32_t n_sampled, float inv_temperature, int32_t log_q_correction, int32_t remove_hits,
                                            float* loss, float* row_ref, float* row_max, float* row_sum, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && loss && row_ref && row_max && row_sum,
                 "trec_sampled_softmax_adj_fwd: null pointer");
    SL_ADJ_REQUIRE("trec_sampled_softmax_adj_fwd");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_sampled_softmax_adj_fwd: inv_temperature must be finite and > 0");
    if (n_users == 0) return TREC_OK;
    const SlAdj adj = make_adj(x_item, samples, log_q, log_q_uniform, n_items, n_sampled, log_q_correction, remove_hits);
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(ssm_adj_fwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, n_users, n_sampled, inv_temperature, loss, row_ref, row_max,
                           row_sum, adj);
        return trec_check_launch("trec_sampled_softmax_adj_fwd");
    }
    const size_t lds = sizeof(float) * 2 * (size_t)n_sampled;
    allow_lds(ssm_adj_fwd_kernel, lds + 1024);
    hipLaunchKernelGGL(ssm_adj_fwd_kernel, dim3((unsigned)n_users), dim3(256), lds, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, n_sampled, inv_temperature, loss, row_ref, row_max, row_sum, adj);
    return trec_check_launch("trec_sampled_softmax_adj_fwd");
}

extern "C" int trec_sampled_softmax_adj_bwd(const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot,
                                            const float* pred_serial, const float* sample_pred, const int32_t* samples,
                                            const float* log_q, float log_q_uniform, const float* row_ref, const float* row_max,
                                            const float* row_sum, const float* grad_loss, int64_t n_users, int64_t n_items,
                                            int32_t n_sampled, float inv_temperature, int32_t log_q_correction, int32_t remove_hits,
                                            float* d_pred_serial, float* d_sample_pred, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && row_ref && row_max && row_sum && grad_loss && d_pred_serial &&
                     d_sample_pred,
                 "trec_sampled_softmax_adj_bwd: null pointer");
    SL_ADJ_REQUIRE("trec_sampled_softmax_adj_bwd");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_sampled_softmax_adj_bwd: inv_temperature must be finite and > 0");
    if (n_users == 0) return TREC_OK;
    const SlAdj adj = make_adj(x_item, samples, log_q, log_q_uniform, n_items, n_sampled, log_q_correction, remove_hits);
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(ssm_adj_bwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, row_ref, row_max, row_sum, grad_loss, n_users, n_sampled,
                           inv_temperature, d_pred_serial, d_sample_pred, adj);
        return trec_check_launch("trec_sampled_softmax_adj_bwd");
    }
    hipLaunchKernelGGL(ssm_adj_bwd_kernel, dim3((unsigned)n_users), dim3(256), 0, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, row_ref, row_max, row_sum, grad_loss, n_sampled, inv_temperature, d_pred_serial, d_sample_pred, adj);
    return trec_check_launch("trec_sampled_softmax_adj_bwd");
}

// BPR has no logQ term: the adjusted pair takes the ids for the hit test only
extern "C" int trec_bpr_adj_fwd(const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot, const float* pred_serial,
                                const float* sample_pred, const int32_t* samples, int64_t n_users, int32_t n_sampled,
                                int32_t remove_hits, float* loss, void* stream)
{
    const int32_t log_q_correction = 0;
    const int64_t n_items = 0;
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && loss, "trec_bpr_adj_fwd: null pointer");
    SL_ADJ_REQUIRE("trec_bpr_adj_fwd");
    if (n_users == 0) return TREC_OK;
    const SlAdj adj = make_adj(x_item, samples, nullptr, 0.f, n_items, n_sampled, 0, remove_hits);
    const float inv_s = 1.0f / (float)n_sampled;
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(bpr_fwd_wave_adj_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, n_users, n_sampled, inv_s, loss, adj);
        return trec_check_launch("trec_bpr_adj_fwd");
    }
    const size_t lds = sizeof(float) * (size_t)n_sampled;
    allow_lds(bpr_fwd_adj_kernel, lds);
    hipLaunchKernelGGL(bpr_fwd_adj_kernel, dim3((unsigned)n_users), dim3(256), lds, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, n_sampled, inv_s, loss, adj);
    return trec_check_launch("trec_bpr_adj_fwd");
}

extern "C" int trec_bpr_adj_bwd(const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot, const float* pred_serial,
                                const float* sample_pred, const int32_t* samples, const float* grad_loss, int64_t n_users,
                                int32_t n_sampled, int32_t remove_hits, float* d_pred_serial, float* d_sample_pred, void* stream)
{
    const int32_t log_q_correction = 0;
    const int64_t n_items = 0;
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && grad_loss && d_pred_serial && d_sample_pred,
                 "trec_bpr_adj_bwd: null pointer");
    SL_ADJ_REQUIRE("trec_bpr_adj_bwd");
    if (n_users == 0) return TREC_OK;
    const SlAdj adj = make_adj(x_item, samples, nullptr, 0.f, n_items, n_sampled, 0, remove_hits);
    const float inv_s = 1.0f / (float)n_sampled;
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(bpr_bwd_wave_adj_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, pred_serial, sample_pred, grad_loss, n_users, n_sampled, inv_s, d_pred_serial,
                           d_sample_pred, adj);
        return trec_check_launch("trec_bpr_adj_bwd");
    }
    const size_t lds = sizeof(float) * ((size_t)n_sampled + 2 * SL_MAX_POS_LDS);
    allow_lds(bpr_bwd_adj_kernel, lds);
    hipLaunchKernelGGL(bpr_bwd_adj_kernel, dim3((unsigned)n_users), dim3(256), lds, (hipStream_t)stream, indptr, pos_slot, pred_serial,
                       sample_pred, grad_loss, n_sampled, inv_s, d_pred_serial, d_sample_pred, adj);
    return trec_check_launch("trec_bpr_adj_bwd");
}
