// tensorrec_amd/csrc/loss_warp.hip -- K6w: WARP (Weston et al., "WSABIE"), forward + backward.
//
// The reference has no such loss (tensorrec/loss_graphs.py): there is no TF op chain to restate, the formulas below are the definition.
// Conventions and layout are K6s' (loss_sampled.hip): interactions are CSR over users, pos_slot[p] is the slot of interaction p in the
// compact [P+] vector or -1 (ignored, d pred = 0), one wave (S <= 256) or one 256-thread workgroup (S <= 16384) owns a user, no atomics
// and a fixed summation order.  y_p a positive's prediction, y_s the prediction of sample s of the same user; the samples are tried in
// table order.
//
//     v_s    = (1.0f - y_p) + y_s            float32, in this order (loss.hip's hinge); sample s VIOLATES iff v_s > 0, strictly
//     kept   every sample, or (remove_hits) every sample that is no hit: its item is not the column of an interaction of the user with
//            pos_slot >= 0; the mask is per user
//     f_p    the smallest kept s that violates;   N_p = number of kept samples with index <= f_p   (f_p + 1 without hit removal)
//     r_p    = (n_items - 1) div N_p;   L_p = logf((float)max(r_p, 1))   (r_p <= 1: an exact 0)
//     loss_p = L_p v_{f_p};   no kept violator: loss_p = 0, f_p = -1, L_p = 0
//     backward (L is piecewise constant and not differentiated):   d y_p = -go_p L_p,   d y_us = sum_{p of u, f_p = s} go_p L_p,
//            the sum in interaction order
// The forward pass stores f_p (first) and L_p (weight) per interaction; the backward pass reads those and no prediction.
// No expf / log1pf / division per cell: a compare and a ballot per 64 samples, one integer division and one logf per positive.
#include "warp_common.hpp"       // wp_weight, wp_upto: shared with csrc/warp_fused.hip; the hit rule and the launch forms of sampled_common.hpp

#define WP_STAGE 256               // positives staged per pass of the workgroup backward kernel

// ---- shared pieces ------------------------------------------------------------------------------------------
struct WpHits {
    const int32_t* x_item;      // CSR column ids (int32, sorted within a row)
    const int32_t* samples;     // [n_users, S] sampled item ids
};

// ---- wave per user (S <= 256) ---------------------------------------------------------------------------------
// Samples sit in <= 4 registers per lane (sample s = r * 64 + lane), padded with -inf: v = (1 - y_p) + -inf never violates.  The
// positives are loaded 64 per pass and taken in turn; everything per positive is wave-uniform: a compare and a ballot per register,
// the first set bit, a popcount of the kept ballots up to it.  Lane q keeps positive q's result, so the pass ends in coalesced stores.
// HITS: a row of <= 64 interactions is held and searched in registers (HIT_ROW_LOAD / HIT_ROW_TEST); longer rows take the binary search in memory.
template <bool HITS>
__global__ __launch_bounds__(256) void warp_fwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int64_t n_users, int32_t S, int32_t n_items_m1, float* __restrict__ loss,
    int32_t* __restrict__ first, float* __restrict__ weight, WpHits h)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    float ys[SAMPLED_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
    uint64_t kept[SAMPLED_WAVE_SR];
    if (HITS) {
        bool whole;                                                // (wave-uniform)
        int32_t col, col_slot;
        HIT_ROW_LOAD(whole, col, col_slot, true, h.x_item, pos_slot, b, e, lane);
#pragma unroll
        for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
            kept[r] = 0ull;
            if (r * 64 >= S) continue;                             // (wave-uniform)
            const bool live = r * 64 + lane < S;
            const int32_t item = live ? h.samples[u * S + r * 64 + lane] : -1;
            bool hit;
            if (whole) {
                HIT_ROW_TEST(hit, col, col_slot, item);
            } else {
                hit = live && row_is_hit(h.x_item, pos_slot, b, e, item);
            }
            kept[r] = __builtin_amdgcn_ballot_w64(live && !hit);
        }
    }
    for (int64_t p0 = b; p0 < e; p0 += 64) {
        const int np = (int)((e - p0 < 64) ? (e - p0) : 64);
        int32_t slot = -1;
        float yp = 0.f;
        if (lane < np) {
            slot = pos_slot[p0 + lane];
            yp = pred[p0 + lane];
        }
        int32_t my_f = -1, my_n = 1;
        float my_v = 0.f;
        for (int q = 0; q < np; ++q) {
            if (__shfl(slot, q, 64) < 0) continue;                 // wave-uniform
            const float base = 1.0f - __shfl(yp, q, 64);
            int32_t f = -1, n = 1, before = 0;
            float vf = 0.f;
#pragma unroll
            for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
                if (r * 64 >= S || f >= 0) continue;               // (wave-uniform)
                const float v = base + ys[r];
                uint64_t m = __builtin_amdgcn_ballot_w64(v > 0.f);
                if (HITS) m &= kept[r];
                if (m != 0ull) {
                    const int k = __builtin_ctzll(m);
                    f = r * 64 + k;
                    vf = __shfl(v, k, 64);
                    n = HITS ? before + __builtin_popcountll(kept[r] & wp_upto(k)) : f + 1;
                } else if (HITS) {
                    before += __builtin_popcountll(kept[r]);
                }
            }
            if (lane == q) { my_f = f; my_n = n; my_v = vf; }
        }
        if (lane < np) {
            float L = 0.f, lo = 0.f;
            if (my_f >= 0) {
                L = wp_weight(n_items_m1, my_n);
                lo = L * my_v;
            }
            first[p0 + lane] = my_f;
            weight[p0 + lane] = L;
            if (slot >= 0) loss[slot] = lo;
        }
    }
}

// Lane s % 64 owns the user's slots s, s + 64, ... in registers; the positives are taken in interaction order, so each slot's sum has
// that order.  A user without interactions gets its zero row here too.
__global__ __launch_bounds__(256) void warp_bwd_wave_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const int32_t* __restrict__ first,
    const float* __restrict__ weight, const float* __restrict__ grad_out, int64_t n_users, int32_t S,
    float* __restrict__ d_pred, float* __restrict__ d_samp)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    float acc[SAMPLED_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) acc[r] = 0.f;
    for (int64_t p0 = b; p0 < e; p0 += 64) {
        const int np = (int)((e - p0 < 64) ? (e - p0) : 64);
        int32_t f = -1;
        float c = 0.f;
        if (lane < np) {
            const int32_t slot = pos_slot[p0 + lane];
            f = slot >= 0 ? first[p0 + lane] : -1;
            if (f >= 0) c = grad_out[slot] * weight[p0 + lane];
            d_pred[p0 + lane] = f >= 0 ? -c : 0.f;
        }
        uint64_t todo = __builtin_amdgcn_ballot_w64(f >= 0);       // the positives of this pass that hold a violator, lowest first
        while (todo != 0ull) {
            const int q = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const int32_t fq = __shfl(f, q, 64);
            const float cq = __shfl(c, q, 64);
#pragma unroll
            for (int r = 0; r < SAMPLED_WAVE_SR; ++r)
                if ((fq >> 6) == r && (fq & 63) == lane) acc[r] += cq;
        }
    }
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r)
        if (r * 64 + lane < S) d_samp[u * S + r * 64 + lane] = acc[r];
}

// ---- workgroup per user (S <= 16384) ----------------------------------------------------------------------------
// Samples sit in LDS, the kept mask as one bit per sample (a 64-bit word per chunk of 64 samples, built once per user).  Waves take
// positives; a positive scans the samples 64 at a time and stops at the first chunk with a kept violator.
template <bool HITS>
__global__ __launch_bounds__(256) void warp_fwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int32_t S, int32_t n_items_m1, float* __restrict__ loss, int32_t* __restrict__ first,
    float* __restrict__ weight, WpHits h)
{
    extern __shared__ uint64_t lds64[];      // HITS: [ceil(S / 64)] kept words | [S] sampled predictions of this user
    const int n_chunks = (S + 63) >> 6;
    uint64_t* l_kept = lds64;
    float* l_s = (float*)(lds64 + (HITS ? n_chunks : 0));
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    fill_samples(l_s, samp, u, S);
    if (HITS) {
        for (int c = wave; c < n_chunks; c += 4) {
            const int s = c * 64 + lane;
            const bool keep = s < S && !row_is_hit(h.x_item, pos_slot, b, e, h.samples[u * S + (s < S ? s : S - 1)]);
            const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
            if (lane == 0) l_kept[c] = m;
        }
    }
    __syncthreads();
    for (int64_t p = b + wave; p < e; p += 4) {
        int32_t f = -1, n = 1, before = 0;
        float vf = 0.f;
        const int32_t slot = pos_slot[p];
        if (slot >= 0) {
            const float base = 1.0f - pred[p];
            for (int c = 0; c < n_chunks; ++c) {
                const int s = c * 64 + lane;
                const float v = s < S ? base + l_s[s] : -INFINITY;
                uint64_t m = __builtin_amdgcn_ballot_w64(v > 0.f);
                const uint64_t kc = HITS ? l_kept[c] : ~0ull;
                m &= kc;
                if (m != 0ull) {
                    const int k = __builtin_ctzll(m);
                    f = c * 64 + k;
                    vf = __shfl(v, k, 64);
                    n = HITS ? before + __builtin_popcountll(kc & wp_upto(k)) : f + 1;
                    break;
                }
                if (HITS) before += __builtin_popcountll(kc);
            }
        }
        if (lane == 0) {
            float L = 0.f, lo = 0.f;
            if (f >= 0) {
                L = wp_weight(n_items_m1, n);
                lo = L * vf;
            }
            first[p] = f;
            weight[p] = L;
            if (slot >= 0) loss[slot] = lo;
        }
    }
}

// Thread s % 256 owns the user's slots s, s + 256, ...: it zeroes them, then adds the terms of the positives whose first violator is
// one of them.  The positives are staged WP_STAGE per pass and every thread walks the stage in order, so each slot's sum has the
// interaction order; a slot is read and written by its one owner only.
__global__ __launch_bounds__(256) void warp_bwd_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const int32_t* __restrict__ first,
    const float* __restrict__ weight, const float* __restrict__ grad_out, int32_t S, float* __restrict__ d_pred,
    float* __restrict__ d_samp)
{
    __shared__ int32_t l_f[WP_STAGE];
    __shared__ float l_c[WP_STAGE];
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    for (int s = threadIdx.x; s < S; s += 256) d_samp[u * S + s] = 0.f;
    for (int64_t p0 = b; p0 < e; p0 += WP_STAGE) {
        const int np = (int)((e - p0 < WP_STAGE) ? (e - p0) : WP_STAGE);
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int64_t p = p0 + threadIdx.x;
            const int32_t slot = pos_slot[p];
            const int32_t f = slot >= 0 ? first[p] : -1;
            float c = 0.f;
            if (f >= 0) c = grad_out[slot] * weight[p];
            d_pred[p] = f >= 0 ? -c : 0.f;
            l_f[threadIdx.x] = f;
            l_c[threadIdx.x] = c;
        }
        __syncthreads();
        for (int q = 0; q < np; ++q) {
            const int32_t f = l_f[q];
            if ((uint32_t)f < (uint32_t)S && (f & 255) == (int)threadIdx.x) d_samp[u * S + f] += l_c[q];
        }
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------
template <bool HITS>
static void launch_fwd(const int64_t* indptr, const int32_t* pos_slot, const float* pred_serial, const float* sample_pred,
                       int64_t n_users, int32_t n_items_m1, int32_t n_sampled, float* loss, int32_t* first, float* weight, WpHits h,
                       hipStream_t stream)
{
    if (use_wave_form(n_sampled)) {
        hipLaunchKernelGGL(warp_fwd_wave_kernel<HITS>, wave_form_grid(n_users), dim3(256), 0, stream, indptr,
                           pos_slot, pred_serial, sample_pred, n_users, n_sampled, n_items_m1, loss, first, weight, h);
        return;
    }
    const size_t lds = sizeof(float) * (size_t)n_sampled + (HITS ? sizeof(uint64_t) * (size_t)((n_sampled + 63) / 64) : 0);
    allow_lds(warp_fwd_kernel<HITS>, lds);
    hipLaunchKernelGGL(warp_fwd_kernel<HITS>, dim3((unsigned)n_users), dim3(256), lds, stream, indptr, pos_slot, pred_serial,
                       sample_pred, n_sampled, n_items_m1, loss, first, weight, h);
}

extern "C" int trec_warp_fwd(const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot, const float* pred_serial,
                             const float* sample_pred, const int32_t* samples, int64_t n_users, int64_t n_items, int32_t n_sampled,
                             int32_t remove_hits, float* loss, int32_t* first, float* weight, void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && pred_serial && sample_pred && loss && first && weight, "trec_warp_fwd: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, "trec_warp_fwd: n_sampled must be in [1, 16384]");
    TREC_REQUIRE(n_items >= 1 && n_items <= 2147483647, "trec_warp_fwd: n_items must be in [1, 2^31)");
    TREC_REQUIRE(!remove_hits || samples, "trec_warp_fwd: null samples with remove_hits");
    TREC_REQUIRE(!remove_hits || x_item, "trec_warp_fwd: null x_item with remove_hits");
    if (n_users == 0) return TREC_OK;
    WpHits h;
    h.x_item = x_item;
    h.samples = samples;
    const int32_t n_items_m1 = (int32_t)(n_items - 1);
    if (remove_hits)
        launch_fwd<true>(indptr, pos_slot, pred_serial, sample_pred, n_users, n_items_m1, n_sampled, loss, first, weight, h,
                         (hipStream_t)stream);
    else
        launch_fwd<false>(indptr, pos_slot, pred_serial, sample_pred, n_users, n_items_m1, n_sampled, loss, first, weight, h,
                          (hipStream_t)stream);
    return trec_check_launch("trec_warp_fwd");
}

extern "C" int trec_warp_bwd(const int64_t* indptr, const int32_t* pos_slot, const int32_t* first, const float* weight,
                             const float* grad_loss, int64_t n_users, int32_t n_sampled, float* d_pred_serial, float* d_sample_pred,
                             void* stream)
{
    TREC_REQUIRE(indptr && pos_slot && first && weight && grad_loss && d_pred_serial && d_sample_pred, "trec_warp_bwd: null pointer");
    TREC_REQUIRE(n_sampled >= 1 && n_sampled <= 16384, "trec_warp_bwd: n_sampled must be in [1, 16384]");
    if (n_users == 0) return TREC_OK;
    if (use_wave_form(n_sampled))
        hipLaunchKernelGGL(warp_bwd_wave_kernel, wave_form_grid(n_users), dim3(256), 0, (hipStream_t)stream,
                           indptr, pos_slot, first, weight, grad_loss, n_users, n_sampled, d_pred_serial, d_sample_pred);
    else
        hipLaunchKernelGGL(warp_bwd_kernel, dim3((unsigned)n_users), dim3(256), 0, (hipStream_t)stream, indptr, pos_slot, first,
                           weight, grad_loss, n_sampled, d_pred_serial, d_sample_pred);
    return trec_check_launch("trec_warp_bwd");
}
