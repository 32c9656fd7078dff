// tensorrec_amd/csrc/warp_fused.hip -- one training step of the WARP loss in ONE pass per user: K3 on the interactions and on the
// [U, S] samples, the loss (csrc/loss_warp.hip: plain, or with accidental hits removed) and the user side of their backward.
//
// The step of softmax_fused.hip with another loss phase.  A workgroup owns a user: its S + n_u item rows are gathered once into the
// registers of the 8 subgroups, predictions, loss and coefficients stay on chip, dU_u is the coefficient-weighted sum of the rows
// still in the registers, and one coefficient per pair goes back to HBM for the item side.  The gather, dU and the rank epilogue ARE
// wmrb_fused.hip's (the parts of csrc/user_fused_body.hpp).  The upstream gradient is the constant 1 (the trainer differentiates the
// SUM of the loss vector).  The definitions are loss_warp.hip's, through the one copy of csrc/warp_common.hpp:
//     v_s    = (1.0f - y_p) + y_s, in this order;  s violates iff v_s > 0, strictly;  kept = not a hit (HITS), the mask per user
//     f_p    the first kept violator in table order;  N_p = the kept samples with index <= f_p;  L_p = wp_weight(n_items - 1, N_p)
//     loss_p = L_p v_f,  coef_p = -L_p,  coef_s = sum_{p of u, f_p = s} L_p in interaction order;  everything an exact 0 for an
//     interaction that is no positive or has no kept violator
// Thread q owns interaction q (n_u <= 255): it walks the predictions in LDS as broadcast reads up to its first kept violator -- one
// compare per cell, no expf and no division --, then one integer division, one logf and one product.  Thread s owns sample s: it adds
// the L_q of the interactions that stopped at s, in interaction order.  At most n_u of a user's S sample coefficients are not 0.
// No float atomics and no cross-lane float reduction in the loss phase: a call is deterministic.
#include "user_fused_body.hpp"
#include "warp_common.hpp"

namespace {

// ITERS, RMAX, SURE: as in wmrb_user_fused_kernel.  HITS: accidental hits leave the scan; the plain instantiations carry none of it --
// no id reload, no hit test, no kept mask.
template <int ITERS, int RMAX, int SURE, bool HITS>
__global__ __launch_bounds__(256, (ITERS == 1 && RMAX == 16) ? 4 : 1) void warp_user_fused_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ ub, const float* __restrict__ ib,
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ xi, const int32_t* __restrict__ pos_slot,
    const int32_t* __restrict__ samples, int64_t n_users, int32_t S, int d, int32_t n_items_m1, int32_t max_rows,
    float* __restrict__ loss, float* __restrict__ pred_serial, float* __restrict__ dU, float* __restrict__ dub,
    float* __restrict__ coef_samples, float* __restrict__ coef_pairs, int32_t* __restrict__ first,
    int32_t* __restrict__ sample_hist, int32_t* __restrict__ sample_rank)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // softmax_fused.hip's layout: y [max_rows4] | coef [max_rows4] | f of the interactions [max_rows4] | hit ids [max_rows4] |
    // the kept mask, 4 words of 64 bits, in the reduction area [16] | partial dU [8][d]
    const int mr4 = (max_rows + 3) & ~3;
    float* l_y = lds;
    float* l_coef = l_y + mr4;
    int32_t* l_f = (int32_t*)(l_coef + mr4);
    int32_t* l_xid = l_f + mr4;
    uint64_t* l_kept = (uint64_t*)(l_xid + mr4);
    float* l_part = (float*)(l_xid + mr4) + 16;
    constexpr int ablate = 0;                                    // (the ablation build is wmrb_fused.hip's alone)

#define USER_FUSED_PART 1
#include "user_fused_body.hpp"
#undef USER_FUSED_PART

    // interaction `tid` of this user (n_pos <= 255): its slot (and, for the hit test, its item) are fetched now, used in phase (c);
    // with HITS thread s looks at sample s: its id again, in the layout of that phase (an L1 / L2 hit)
    const int qi = tid < n_pos ? tid : n_pos - 1;
    const int32_t slot_ld = pos_slot[b + qi];
    const int32_t xi_ld = HITS ? xi[b + qi] : 0;
    const int32_t my_sample = HITS ? samples[u * S + (tid < S ? tid : S - 1)] : 0;
    const int32_t my_slot = (tid < n_pos) ? slot_ld : -1;

#define USER_FUSED_PART 2
#include "user_fused_body.hpp"
#undef USER_FUSED_PART
    // the columns a sample is tested against: the user's interactions with pos_slot >= 0, -1 (no item) for the others and
    // for the padding up to a multiple of four
    const int np4 = (n_pos + 3) & ~3;
    if (HITS && tid < np4) l_xid[tid] = hit_column(xi_ld, my_slot);
    __syncthreads();

    // ---- (c) loss terms and coefficients: thread s owns sample s, thread q interaction q ----
    const bool is_sample = tid < S;
    if (HITS) {
        bool hit;
        HIT_SCAN4(hit, l_xid, np4, my_sample);
        const uint64_t m = __builtin_amdgcn_ballot_w64(is_sample && !hit);       // the kept samples 64 wave .. 64 wave + 63
        if (lane == 0) l_kept[wave] = m;
        __syncthreads();
    }
    // the scan: v in table order up to the first kept violator; a wave leaves once all its interactions have stopped (there is no
    // barrier inside the walk)
    const float base = 1.0f - l_y[S + qi];
    int32_t f = -1;
    float vf = 0.f;
    bool open = my_slot >= 0;
    for (int s4 = 0; s4 < S; s4 += 4) {
        if (__builtin_amdgcn_ballot_w64(open) == 0ull) break;
        const f32x4 y4 = *(const f32x4*)(l_y + s4);              // (s4 + 3 < max_rows4; cells past S are never taken)
        const uint32_t k4 = HITS ? (uint32_t)(l_kept[s4 >> 6] >> (s4 & 63)) & 0xfu : 0xfu;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = base + y4[k];
            if (open && s4 + k < S && v > 0.f && ((k4 >> k) & 1u)) {
                f = s4 + k;
                vf = v;
                open = false;
            }
        }
    }
    float L = 0.f, lo = 0.f;
    if (f >= 0) {
        int32_t n = f + 1;
        if (HITS) {
            n = __builtin_popcountll(l_kept[f >> 6] & wp_upto(f & 63));
            for (int c = 0; c < (f >> 6); ++c) n += __builtin_popcountll(l_kept[c]);
        }
        L = wp_weight(n_items_m1, n);
        lo = L * vf;
    }
    if (my_slot >= 0) loss[my_slot] = lo;
    if (tid < n_pos) {
        const float dp = f >= 0 ? -L : 0.f;
        l_coef[S + tid] = dp;
        coef_pairs[b + tid] = dp;
        if (first) first[b + tid] = f;
    }
    if (tid < np4) l_f[tid] = f;                                 // (-1 for an interaction without a violator and for the padding)
    __syncthreads();
    if (is_sample) {
        float cs = 0.f;
        for (int q4 = 0; q4 < np4; q4 += 4) {                    // broadcast reads again; the terms in interaction order
            const int32_t f0 = l_f[q4], f1 = l_f[q4 + 1], f2 = l_f[q4 + 2], f3 = l_f[q4 + 3];
            if (f0 == tid) cs += -l_coef[S + q4];                // (L_q = -coef_q, exactly)
            if (f1 == tid) cs += -l_coef[S + q4 + 1];
            if (f2 == tid) cs += -l_coef[S + q4 + 2];
            if (f3 == tid) cs += -l_coef[S + q4 + 3];
        }
        l_coef[tid] = cs;
        coef_samples[u * S + tid] = cs;
    }
    __syncthreads();

#define USER_FUSED_PART 3
#include "user_fused_body.hpp"
#undef USER_FUSED_PART
}

}  // namespace

// Dynamic LDS the fused WARP step needs, or -1 if the configuration is not covered (the host then runs the generic step): the
// coverage and the number of trec_softmax_fused_lds_bytes -- 1 <= n_sampled <= 256, d % 4 == 0, 4 <= d <= 256, n_sampled + the
// longest interaction row <= 256 (128 for d > 128).
extern "C" int trec_warp_fused_lds_bytes(int32_t n_sampled, int32_t max_interactions_per_user, int32_t d)
{
    return fused_lds_bytes(n_sampled, max_interactions_per_user, d);
}

extern "C" int trec_warp_fused_step(const float* U, const float* V, const float* user_bias, const float* item_bias,
                                    const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot, const int32_t* samples,
                                    int64_t n_users, int64_t n_items, int32_t n_sampled, int32_t d,
                                    int32_t max_interactions_per_user, int32_t remove_hits, float* loss, float* pred_serial,
                                    float* dU, float* d_user_bias, float* coef_samples, float* coef_pairs, int32_t* first,
                                    int32_t* sample_hist, int32_t* sample_rank, void* stream)
{
    USER_FUSED_REQUIRE_POINTERS("trec_warp_fused_step");
    USER_FUSED_REQUIRE_PAIRS("trec_warp_fused_step");
    TREC_REQUIRE(n_items >= 1 && n_items < ((int64_t)1 << 31), "trec_warp_fused_step: n_items must lie in [1, 2^31)");
    TREC_REQUIRE(!remove_hits || (x_item && pos_slot), "trec_warp_fused_step: remove_hits needs the interaction arrays");
    USER_FUSED_COVERED("trec_warp_fused_step", trec_warp_fused_lds_bytes);
    const int32_t n_items_m1 = (int32_t)(n_items - 1);
#define TREC_FUSED_K(IT, RM, SU, HITS)                                                                                         \
    hipLaunchKernelGGL((warp_user_fused_kernel<IT, RM, SU, HITS>), dim3((unsigned)n_users), dim3(256), lds, st, U, V, user_bias, \
                       item_bias, indptr, x_item, pos_slot, samples, n_users, n_sampled, d, n_items_m1, max_rows, loss,        \
                       pred_serial, dU, d_user_bias, coef_samples, coef_pairs, first, sample_hist, sample_rank)
#define TREC_FUSED(IT, RM, SU)                                                                                                 \
    do {                                                                                                                       \
        if (remove_hits) TREC_FUSED_K(IT, RM, SU, true);                                                                       \
        else TREC_FUSED_K(IT, RM, SU, false);                                                                                  \
    } while (0)
    USER_FUSED_LAUNCH("trec_warp_fused_step");
#undef TREC_FUSED
#undef TREC_FUSED_K
}
