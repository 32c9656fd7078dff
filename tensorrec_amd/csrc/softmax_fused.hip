// tensorrec_amd/csrc/softmax_fused.hip -- one training step of the sampled softmax loss in ONE pass per user: K3 on the interactions
// and on the [U, S] samples, the loss (csrc/loss_sampled.hip: plain, or with the logQ correction and / or accidental hits removed)
// and the user side of their backward.
//
// The step of wmrb_fused.hip with another loss phase.  A workgroup owns a user: its S + n_u item rows are gathered once into the
// registers of the 8 subgroups, predictions, loss and coefficients stay on chip, dU_u is the coefficient-weighted sum of the rows
// still in the registers, and one coefficient per pair goes back to HBM for the item side.  The gather, dU and the rank epilogue ARE
// wmrb_fused.hip's (the parts of csrc/user_fused_body.hpp).  The upstream gradient is the constant 1 (the trainer differentiates the SUM of the
// loss vector).  With t = 1 / temperature:
//     plain      per user  M = max_s y_s, Z = sum_s exp((y_s - M) t);  per positive  m = max(M, y_p), a = exp((y_p - m) t),
//                b = exp((M - m) t), D = a + b Z:  loss_p = (m - y_p) t + log D,  coef_p = -t b Z / D,  K_u = sum_p b_p / D_p,
//                coef_s = t exp((y_s - M) t) K_u
//     adjusted   kept = not a hit;  c_s = -(log S + log q(item_s)) with the correction, else 0;  R = max_kept y_s,
//                w_s = (y_s - R) t + c_s, M = max_kept w_s, Z = sum_kept exp(w_s - M), w_p = (y_p - R) t, then the terms above on
//                (w_p, M, Z) with t = 1;  coef_p = -t b Z / D, coef_s = t exp(w_s - M) K_u for a kept sample and exactly 0 for a hit;
//                no kept sample: loss_p = 0 and every coefficient of the user is 0 (docs/sampled_losses.md)
// The sums factor per user: the loss phase is O(S + n_u) where WMRB's is O(S n_u).  M, Z and K_u are reduced over the 256 threads
// in a fixed order (xor butterfly inside a wave, the four waves' partials added as (0 + 1) + (2 + 3)): a call is deterministic.
// expf / logf are the library's (no fast-math): the error bars of tests/sampled_loss_reference.py apply as they stand.
#include "user_fused_body.hpp"
#include "sampled_common.hpp"   // hit_column, HIT_SCAN4, ssm_terms, logq_correction, the butterfly reductions, temperature_ok

namespace {

// ITERS, RMAX, SURE: as in wmrb_user_fused_kernel.  ADJ: the adjusted loss phase (use_q: the logQ correction, no_hits: accidental
// hits leave the sums); the plain instantiations carry none of it -- no id reload, no log q gather, no hit test.
template <int ITERS, int RMAX, int SURE, bool ADJ>
__global__ __launch_bounds__(256, (ITERS == 1 && RMAX == 16) ? 4 : 1) void softmax_user_fused_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ ub, const float* __restrict__ ib,
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ xi, const int32_t* __restrict__ pos_slot,
    const int32_t* __restrict__ samples, const float* __restrict__ log_q, int64_t n_users, int32_t S, int d, float t, float log_s,
    float log_uniform, int use_q, int no_hits, int32_t max_rows, float* __restrict__ loss, float* __restrict__ pred_serial,
    float* __restrict__ dU, float* __restrict__ dub, float* __restrict__ coef_samples, float* __restrict__ coef_pairs,
    int32_t* __restrict__ sample_hist, int32_t* __restrict__ sample_rank)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // y [max_rows4] | coef [max_rows4] | log q of the samples [max_rows4] | hit ids [max_rows4] | reductions [16] | partial dU [8][d]
    const int mr4 = (max_rows + 3) & ~3;
    float* l_y = lds;
    float* l_coef = l_y + mr4;
    float* l_lq = l_coef + mr4;
    int32_t* l_xid = (int32_t*)(l_lq + mr4);
    float* l_red = (float*)(l_xid + mr4);
    float* l_part = l_red + 16;
    constexpr int ablate = 0;                                    // (the ablation build is wmrb_fused.hip's alone)
    const float* __restrict__ side = log_q;
    const float side_uniform = log_uniform;
    float* l_side = l_lq;
#define USER_FUSED_SIDE ADJ                                      // log q of the sampled items, fetched with the item biases

#define USER_FUSED_PART 1
#include "user_fused_body.hpp"
#undef USER_FUSED_PART

    // interaction `tid` of this user (n_pos <= 256): its slot (and, for the hit test, its item) are fetched now, used in phase (c);
    // the adjusted loss phase has thread s look at sample s: its id again, in the layout of that phase (an L1 / L2 hit)
    const int qi = tid < n_pos ? tid : n_pos - 1;
    const int32_t slot_ld = pos_slot[b + qi];
    const int32_t xi_ld = (ADJ && no_hits) ? xi[b + qi] : 0;      // (uniform branch)
    const int32_t my_sample = ADJ ? samples[u * S + (tid < S ? tid : S - 1)] : 0;
    const int32_t my_slot = (tid < n_pos) ? slot_ld : -1;

#define USER_FUSED_PART 2
#include "user_fused_body.hpp"
#undef USER_FUSED_PART
    // the columns a sample is tested against: the user's interactions with pos_slot >= 0, -1 (no item) for the others and
    // for the padding up to a multiple of four
    const int np4 = (n_pos + 3) & ~3;
    if (ADJ && no_hits && tid < np4) l_xid[tid] = hit_column(xi_ld, my_slot);
    __syncthreads();

    // ---- (c) loss terms and coefficients: thread s owns sample s, thread q interaction q ----
    const bool is_sample = tid < S;
    const float ys = is_sample ? l_y[tid] : -INFINITY;           // padding never wins a maximum and adds exp(-inf) = 0
    const float yp = l_y[S + qi];
    float dp = 0.f, term = 0.f, cs = 0.f;
    if (!ADJ) {
        const float M = wg_max_butterfly(ys, l_red);
        const float E = expf((ys - M) * t);
        const float Z = wg_sum_butterfly(E, l_red + 4);
        if (my_slot >= 0) {
            float m, bb, bz, D;
            ssm_terms(yp, M, Z, t, m, bb, bz, D);
            loss[my_slot] = (m - yp) * t + logf(D);
            dp = -t * (bz / D);
            term = bb / D;
        }
        const float K = wg_sum_butterfly(term, l_red + 8);              // a non-positive interaction or an idle thread adds an exact 0
        cs = (t * E) * K;
    } else {
        bool kept = is_sample;
        if (no_hits) {                                           // (uniform branch)
            bool hit;
            HIT_SCAN4(hit, l_xid, np4, my_sample);
            kept = kept && !hit;
        }
        const float c = (use_q && is_sample) ? logq_correction(log_s, l_lq[tid]) : 0.f;
        const float Rm = wg_max_butterfly(kept ? ys : -INFINITY, l_red);
        if (Rm != -INFINITY) {                                   // (uniform) -inf: every sample of this user is a hit
            const float w = kept ? (ys - Rm) * t + c : -INFINITY;
            const float M = wg_max_butterfly(w, l_red + 4);
            const float E = expf(w - M);                          // 0 for a hit and for padding
            const float Z = wg_sum_butterfly(E, l_red + 8);
            if (my_slot >= 0) {
                const float wp = (yp - Rm) * t;
                float m, bb, bz, D;
                ssm_terms(wp, M, Z, 1.0f, m, bb, bz, D);
                loss[my_slot] = (m - wp) + logf(D);
                dp = -t * (bz / D);
                term = bb / D;
            }
            const float K = wg_sum_butterfly(term, l_red + 12);
            cs = kept ? (t * E) * K : 0.f;                        // a hit's coefficient is exactly 0
        } else if (my_slot >= 0) {
            loss[my_slot] = 0.f;
        }
    }
    if (tid < n_pos) {
        l_coef[S + tid] = dp;
        coef_pairs[b + tid] = dp;
    }
    if (is_sample) {
        l_coef[tid] = cs;
        coef_samples[u * S + tid] = cs;
    }
    __syncthreads();

#define USER_FUSED_PART 3
#include "user_fused_body.hpp"
#undef USER_FUSED_PART
#undef USER_FUSED_SIDE
}

}  // namespace

// Dynamic LDS the fused softmax step needs, or -1 if the configuration is not covered (the host then runs the generic step): the
// coverage of trec_wmrb_fused_lds_bytes -- 1 <= n_sampled <= 256, d % 4 == 0, 4 <= d <= 256, n_sampled + the longest interaction
// row <= 256 (128 for d > 128).
extern "C" int trec_softmax_fused_lds_bytes(int32_t n_sampled, int32_t max_interactions_per_user, int32_t d)
{
    return fused_lds_bytes(n_sampled, max_interactions_per_user, d);
}

extern "C" int trec_softmax_fused_step(const float* U, const float* V, const float* user_bias, const float* item_bias,
                                       const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot,
                                       const int32_t* samples, int64_t n_users, int64_t n_items, int32_t n_sampled, int32_t d,
                                       int32_t max_interactions_per_user, float inv_temperature, const float* log_q,
                                       float log_uniform, int32_t log_q_correction, int32_t remove_hits, float* loss,
                                       float* pred_serial, float* dU, float* d_user_bias, float* coef_samples, float* coef_pairs,
                                       int32_t* sample_hist, int32_t* sample_rank, void* stream)
{
    USER_FUSED_REQUIRE_POINTERS("trec_softmax_fused_step");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_fused_step: inv_temperature must be finite and > 0");
    USER_FUSED_REQUIRE_PAIRS("trec_softmax_fused_step");
    TREC_REQUIRE(!log_q_correction || (n_items >= 1 && n_items < ((int64_t)1 << 31)),
                 "trec_softmax_fused_step: n_items must lie in [1, 2^31) with the logQ correction");
    TREC_REQUIRE(!remove_hits || (x_item && pos_slot), "trec_softmax_fused_step: remove_hits needs the interaction arrays");
    USER_FUSED_COVERED("trec_softmax_fused_step", trec_softmax_fused_lds_bytes);
    const float log_s = (float)log((double)n_sampled);
    const int use_q = log_q_correction ? 1 : 0, no_hits = remove_hits ? 1 : 0;
    const bool adj = use_q || no_hits;
#define TREC_FUSED_K(IT, RM, SU, ADJ)                                                                                          \
    hipLaunchKernelGGL((softmax_user_fused_kernel<IT, RM, SU, ADJ>), dim3((unsigned)n_users), dim3(256), lds, st, U, V,         \
                       user_bias, item_bias, indptr, x_item, pos_slot, samples, use_q ? log_q : (const float*)nullptr, n_users, \
                       n_sampled, d, inv_temperature, log_s, log_uniform, use_q, no_hits, max_rows, loss, pred_serial, dU,      \
                       d_user_bias, coef_samples, coef_pairs, sample_hist, sample_rank)
#define TREC_FUSED(IT, RM, SU)                                                                                                 \
    do {                                                                                                                       \
        if (adj) TREC_FUSED_K(IT, RM, SU, true);                                                                               \
        else TREC_FUSED_K(IT, RM, SU, false);                                                                                  \
    } while (0)
    USER_FUSED_LAUNCH("trec_softmax_fused_step");
#undef TREC_FUSED
#undef TREC_FUSED_K
}
