// tensorrec_amd/csrc/loss_sampled_bpr_body.hpp -- the four BPR kernels of csrc/loss_sampled.hip, included twice: with SL_ADJ 0 it is the
// text of the plain kernels (bpr_*_kernel), unchanged; with SL_ADJ 1 it gives bpr_*_adj_kernel, which take an SlAdj and turn every
// accidental hit into padding right after the samples are loaded.  No include guard on purpose.
#if SL_ADJ
#define SL_KERNEL(name) name##_adj_kernel
#define SL_ADJ_PARAM , SlAdj adj
#else
#define SL_KERNEL(name) name##_kernel
#define SL_ADJ_PARAM
#endif

// ---- BPR: wave per user (S <= 256) --------------------------------------------------------------------------------
// The loop structure of wmrb_*_wave_kernel: 64 positives loaded per pass and broadcast.  The -inf padding gives x = -inf:
// softplus = max(-inf, 0) + log1p(exp(-inf)) = 0 and sigma = exp(-inf) / (1 + exp(-inf)) = 0, so a padded lane adds nothing.
// Every cell costs an expf and a log1pf or a division, so registers that hold padding only (S = 100: two of the four) are skipped.
__global__ __launch_bounds__(256) void SL_KERNEL(bpr_fwd_wave)(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int64_t n_users, int32_t S, float inv_s, float* __restrict__ loss SL_ADJ_PARAM)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    float ys[SAMPLED_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
#if SL_ADJ
    {                                                              // a hit becomes padding
        const HitRow row = sl_row_wave(adj, pos_slot, b, e, lane);
#pragma unroll
        for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
            float c;
            ys[r] = sl_adjust_wave(adj, pos_slot, b, e, row, r * 64 + lane < S, u * S + r * 64 + lane, ys[r], c);
        }
    }
#endif
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
            for (int r = 0; r < SAMPLED_WAVE_SR; ++r)
                if (r * 64 < S) acc += softplus_f(ys[r] - ypq);    // (wave-uniform: a register of padding only costs nothing)
            acc = wave_sum(acc);
            if (lane == q) mine = acc * inv_s;
        }
        if (lane < np && slot >= 0) loss[slot] = mine;
    }
}

__global__ __launch_bounds__(256) void SL_KERNEL(bpr_bwd_wave)(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ grad_out, int64_t n_users, int32_t S, float inv_s,
    float* __restrict__ d_pred, float* __restrict__ d_samp SL_ADJ_PARAM)
{
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (u >= n_users) return;
    const int lane = lane_id();
    const int64_t b = indptr[u], e = indptr[u + 1];
    float ys[SAMPLED_WAVE_SR], acc[SAMPLED_WAVE_SR];
#pragma unroll
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
        ys[r] = (r * 64 + lane < S) ? samp[u * S + r * 64 + lane] : -INFINITY;
        acc[r] = 0.f;
    }
#if SL_ADJ
    {                                                              // a hit becomes padding
        const HitRow row = sl_row_wave(adj, pos_slot, b, e, lane);
#pragma unroll
        for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
            float c;
            ys[r] = sl_adjust_wave(adj, pos_slot, b, e, row, r * 64 + lane < S, u * S + r * 64 + lane, ys[r], c);
        }
    }
#endif
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
            for (int r = 0; r < SAMPLED_WAVE_SR; ++r) {
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
    for (int r = 0; r < SAMPLED_WAVE_SR; ++r)
        if (r * 64 + lane < S) d_samp[u * S + r * 64 + lane] = acc[r];
}

// ---- BPR: workgroup per user (S <= 16384) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void SL_KERNEL(bpr_fwd)(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, int32_t S, float inv_s, float* __restrict__ loss SL_ADJ_PARAM)
{
    extern __shared__ float lds[];           // [S] sampled predictions of this user
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b == e) return;
    fill_samples(lds, samp, u, S);
#if SL_ADJ
    for (int s = threadIdx.x; s < S; s += 256) {                   // a hit becomes padding (a thread masks the slots it filled)
        float c;
        lds[s] = sl_adjust(adj, pos_slot, b, e, u * S + s, lds[s], c);
    }
#endif
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

__global__ __launch_bounds__(256) void SL_KERNEL(bpr_bwd)(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ pos_slot, const float* __restrict__ pred,
    const float* __restrict__ samp, const float* __restrict__ grad_out, int32_t S, float inv_s,
    float* __restrict__ d_pred, float* __restrict__ d_samp SL_ADJ_PARAM)
{
    extern __shared__ float lds[];           // [S] samples | [SL_MAX_POS_LDS] yp | [SL_MAX_POS_LDS] c
    float* l_s = lds;
    float* l_yp = lds + S;
    float* l_c = l_yp + SL_MAX_POS_LDS;
    const int64_t u = blockIdx.x;
    const int64_t b = indptr[u], e = indptr[u + 1];
    fill_samples(l_s, samp, u, S);
#if SL_ADJ
    for (int s = threadIdx.x; s < S; s += 256) {                   // a hit becomes padding (a thread masks the slots it filled)
        float c;
        l_s[s] = sl_adjust(adj, pos_slot, b, e, u * S + s, l_s[s], c);
    }
#endif
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

#undef SL_KERNEL
#undef SL_ADJ_PARAM
