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
#include "common.hpp"

#define SL_MAX_POS_LDS 1024        // positives of one user staged per pass (workgroup BPR backward)
#define SL_WAVE_SR 4               // samples per lane of the wave-per-user forms: S <= 64 * SL_WAVE_SR

// ---- shared pieces ------------------------------------------------------------------------------------------
// fixed-tree workgroup reductions over 256 threads (every thread gets the result)
__device__ __forceinline__ float wg_sum(float v, float* red)
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

__device__ __forceinline__ float wg_max(float v, float* red)
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

__device__ __forceinline__ float wave_sum(float v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one user's samples into LDS (four loads per thread in flight, then the four LDS stores, as loss.hip fills)
__device__ __forceinline__ void fill_samples(float* l_s, const float* __restrict__ samp, int64_t u, int32_t S)
{
    for (int s0 = threadIdx.x; s0 < S; s0 += 1024) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int s = s0 + 256 * k; t[k] = samp[u * S + (s < S ? s : S - 1)]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int s = s0 + 256 * k; if (s < S) l_s[s] = t[k]; }
    }
}

// the per-positive terms of the sampled softmax from the user's (M, Z): bz = b Z, D = a + b Z; forward and backward share the code
__device__ __forceinline__ void ssm_terms(float yp, float M, float Z, float t, float& m, float& b, float& bz, float& D)
{
    m = fmaxf(M, yp);
    const float a = expf((yp - m) * t);
    b = expf((M - m) * t);
    bz = b * Z;
    D = a + bz;
}

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float sigmoid_f(float x)
{
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
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
    float ys[SL_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SL_WAVE_SR; ++r) ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
    float M = fmaxf(fmaxf(ys[0], ys[1]), fmaxf(ys[2], ys[3]));
    for (int off = 32; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
    float z = 0.f;
#pragma unroll
    for (int r = 0; r < SL_WAVE_SR; ++r) z += expf((ys[r] - M) * t);
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
    for (int r = 0; r < SL_WAVE_SR; ++r) {
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
    const float M = wg_max(mx, red);
    float z = 0.f;
    for (int s = threadIdx.x; s < S; s += 256) z += expf((lds[s] - M) * t);
    const float Z = wg_sum(z, red);
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
    const float K = wg_sum(k, red);
    const bool any = wg_max(n_pos, red) > 0.f;
    for (int s = threadIdx.x; s < S; s += 256)
        d_samp[u * S + s] = any ? (t * expf((samp[u * S + s] - M) * t)) * K : 0.f;
}

// ---- BPR: wave per user (S <= 256) --------------------------------------------------------------------------------
// The loop structure of wmrb_*_wave_kernel: 64 positives loaded per pass and broadcast.  The -inf padding gives x = -inf:
// softplus = max(-inf, 0) + log1p(exp(-inf)) = 0 and sigma = exp(-inf) / (1 + exp(-inf)) = 0, so a padded lane adds nothing.
// Every cell costs an expf and a log1pf or a division, so registers that hold padding only (S = 100: two of the four) are skipped.
__global__ __launch_bounds__(256) void bpr_fwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int64_t n_users, int32_t S, float inv_s, float* __restrict__ loss)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    float ys[SL_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SL_WAVE_SR; ++r) ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
    for (int64_t p0 = b; p0 < e; p0 += 64) {
        const int np = (int)((e - p0 < 64) ? (e - p0) : 64);
        int32_t slot = -1;
        float yp = 0.f;
        if (lane < np) {
            slot = pos_slot[p0 + lane];
            yp = pred[p0 + lane];
        }
        float mine = 0.f;
        for (int q = 0; q < np; ++q) {
            if (__shfl(slot, q, 64) < 0) continue;                 // wave-uniform
            const float ypq = __shfl(yp, q, 64);
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < SL_WAVE_SR; ++r)
                if (r * 64 < S) acc += softplus_f(ys[r] - ypq);    // (wave-uniform: a register of padding only costs nothing)
            acc = wave_sum(acc);
            if (lane == q) mine = acc * inv_s;
        }
        if (lane < np && slot >= 0) loss[slot] = mine;
    }
}

__global__ __launch_bounds__(256) void bpr_bwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ grad_out, int64_t n_users, int32_t S, float inv_s,
    float* __restrict__ d_pred, float* __restrict__ d_samp)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    float ys[SL_WAVE_SR], acc[SL_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SL_WAVE_SR; ++r) {
        ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
        acc[r] = 0.f;
    }
    for (int64_t p0 = b; p0 < e; p0 += 64) {
        const int np = (int)((e - p0 < 64) ? (e - p0) : 64);
        float c = 0.f, yp = 0.f;
        if (lane < np) {
            const int32_t slot = pos_slot[p0 + lane];
            yp = pred[p0 + lane];
            if (slot >= 0) c = grad_out[slot] * inv_s;
        }
        float my_dp = 0.f;
        for (int q = 0; q < np; ++q) {
            const float cq = __shfl(c, q, 64);
            if (cq == 0.f) continue;                               // wave-uniform; d_pred stays 0
            const float ypq = __shfl(yp, q, 64);
            float sg = 0.f;
#pragma unroll
            for (int r = 0; r < SL_WAVE_SR; ++r) {
                if (r * 64 >= S) continue;                         // (wave-uniform: a register of padding only costs nothing)
                const float sig = sigmoid_f(ys[r] - ypq);
                sg += sig;
                acc[r] += cq * sig;
            }
            sg = wave_sum(sg);
            if (lane == q) my_dp = -cq * sg;
        }
        if (lane < np) d_pred[p0 + lane] = my_dp;
    }
#pragma unroll
    for (int r = 0; r < SL_WAVE_SR; ++r)
        if (r * 64 + lane < S) d_samp[u * S + r * 64 + lane] = acc[r];
}

// ---- BPR: workgroup per user (S <= 16384) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bpr_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int32_t S, float inv_s, float* __restrict__ loss)
{
    extern __shared__ float lds[];           // [S] sampled predictions of this user
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    fill_samples(lds, samp, u, S);
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (int64_t p = b + wave; p < e; p += 4) {
        const int32_t slot = pos_slot[p];
        if (slot < 0) continue;
        const float yp = pred[p];
        float acc = 0.f;
        for (int s = lane; s < S; s += 64) acc += softplus_f(lds[s] - yp);
        acc = wave_sum(acc);
        if (lane == 0) loss[slot] = acc * inv_s;
    }
}

__global__ __launch_bounds__(256) void bpr_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ grad_out, int32_t S, float inv_s,
    float* __restrict__ d_pred, float* __restrict__ d_samp)
{
    extern __shared__ float lds[];           // [S] samples | [SL_MAX_POS_LDS] yp | [SL_MAX_POS_LDS] c
    float* l_s = lds;
    float* l_yp = lds + S;
    float* l_c = l_yp + SL_MAX_POS_LDS;
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    fill_samples(l_s, samp, u, S);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (int64_t p0 = b; p0 < e || p0 == b; p0 += SL_MAX_POS_LDS) {
        const int np = (int)((e - p0 < SL_MAX_POS_LDS) ? (e - p0) : SL_MAX_POS_LDS);
        __syncthreads();
        for (int q = threadIdx.x; q < np; q += 256) {
            const int32_t slot = pos_slot[p0 + q];
            l_yp[q] = pred[p0 + q];
            l_c[q] = slot >= 0 ? grad_out[slot] * inv_s : 0.f;
        }
        __syncthreads();
        // (1) gradient w.r.t. the positive's own prediction: waves over positives, lanes over samples
        for (int q = wave; q < np; q += 4) {
            const float c = l_c[q];
            if (c == 0.f) { if (lane == 0) d_pred[p0 + q] = 0.f; continue; }
            const float yp = l_yp[q];
            float sg = 0.f;
            for (int s = lane; s < S; s += 64) sg += sigmoid_f(l_s[s] - yp);
            sg = wave_sum(sg);
            if (lane == 0) d_pred[p0 + q] = -c * sg;
        }
        // (2) gradient w.r.t. the shared samples: threads own s, loop over this pass's positives in order
        for (int s = threadIdx.x; s < S; s += 256) {
            const float ys = l_s[s];
            float acc = (p0 == b) ? 0.f : d_samp[u * S + s];
            for (int q = 0; q < np; ++q) {
                const float c = l_c[q];
                if (c != 0.f) acc += c * sigmoid_f(ys - l_yp[q]);   // (uniform over the workgroup)
            }
            d_samp[u * S + s] = acc;
        }
        if (e == b) break;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------
// dynamic LDS above 64 KB (S close to 16384) has to be asked for
template <typename K>
static inline void allow_lds(K kernel, size_t lds)
{
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

static inline bool use_wave_form(int32_t n_sampled)
{
    return n_sampled <= 64 * SL_WAVE_SR && trec_get_tuning("wmrb_wave", 1);
}

static inline bool temperature_ok(float inv_temperature) { return inv_temperature > 0.f && inv_temperature <= 3.402823466e+38f; }

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
        hipLaunchKernelGGL(ssm_fwd_wave_kernel, dim3((unsigned)ceil_div64(n_users * 64, 256)), dim3(256), 0, (hipStream_t)stream,
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
        hipLaunchKernelGGL(ssm_bwd_wave_kernel, dim3((unsigned)ceil_div64(n_users * 64, 256)), dim3(256), 0, (hipStream_t)stream,
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
        hipLaunchKernelGGL(bpr_fwd_wave_kernel, dim3((unsigned)ceil_div64(n_users * 64, 256)), dim3(256), 0, (hipStream_t)stream,
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
        hipLaunchKernelGGL(bpr_bwd_wave_kernel, dim3((unsigned)ceil_div64(n_users * 64, 256)), dim3(256), 0, (hipStream_t)stream,
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
