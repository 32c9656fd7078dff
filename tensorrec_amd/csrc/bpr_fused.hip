// tensorrec_amd/csrc/bpr_fused.hip -- one training step of the BPR loss in ONE pass per user: K3 on the interactions and on the
// [U, S] samples, the loss (csrc/loss_sampled.hip, trec_bpr_fwd / _bwd: plain, or with accidental hits removed) and the user side
// of their backward.
//
// The step of warp_fused.hip with another loss phase.  A workgroup owns a user: its S + n_u item rows are gathered once into the
// registers of the 8 subgroups, predictions, loss and coefficients stay on chip, dU_u is the coefficient-weighted sum of the rows
// still in the registers, and one coefficient per pair goes back to HBM for the item side.  The gather, dU and the rank epilogue ARE
// wmrb_fused.hip's (the parts of csrc/user_fused_body.hpp).  The upstream gradient is the constant 1 (the trainer differentiates the
// SUM of the loss vector).  The definitions are loss_sampled.hip's, through the one copy of the cell in csrc/sampled_common.hpp:
//     x_ps   = y_s - y_p;  kept = not a hit (HITS), the mask per user;  the divisor is S, also with hits removed
//     loss_p = (1/S) sum_{s kept} softplus(x_ps),  coef_p = -(1/S) sum_{s kept} sigma(x_ps),  coef_s = (1/S) sum_{p of u} sigma(x_ps);
//     an interaction with pos_slot < 0 gets coef_p = 0 exactly and adds nothing; a hit gets coef_s = 0 exactly and adds nothing
// The phase is O(S n_u) cells of one expf, one log1pf and one division each (softplus_sigmoid_f: both values from one e), so it uses
// the whole workgroup.  W = the waves the samples need, a power of two (1: S <= 64, 2: S <= 128, 4); group g = wave / W of the
// G = 4 / W groups takes the interactions q = g, g + G, ... in interaction order; lane l of the group's wave w = wave % W owns
// sample 64 w + l.  Per interaction a wave reduces its 64 softplus and its 64 sigma values (xor butterfly) and leaves the two sums in
// LDS; a lane keeps the sigma values of ITS sample, summed over its group's interactions, and leaves that partial in LDS too.  After
// ONE barrier thread q adds the wave sums of interaction q in the order w = 0, 1, ..., thread s the group partials of sample s in
// the order g = 0, 1, ..., and both multiply by 1 / S.  A wave whose 64 sample slots are all past S (S = 129 .. 192: the fourth)
// skips the loop and its sums are not read.  No float atomics, a fixed summation order, no barrier inside the loop: a call is
// deterministic.
// Dynamic LDS, in 4-byte words (tests/bpr_step_reference.py mirrors it):
//     y [rows4] | coef [rows4] | pos_slot of the interactions [rows4] | hit ids [rows4] | softplus sums, then sigma sums, [n_u max][W]
//     each: 2 W max_interactions_per_user rounded up to 4 | sample partials [G][64 W] = 256 | partial dU [8][d]
//     bytes = 4 (4 rows4 + round4(2 W max_interactions_per_user) + 256 + 8 d),  rows4 = n_sampled + max_interactions_per_user rounded up to 4
#include "user_fused_body.hpp"
#include "sampled_common.hpp"

namespace {

static int bpr_sample_waves(int32_t n_sampled) { return n_sampled <= 64 ? 1 : (n_sampled <= 128 ? 2 : 4); }

// ITERS, RMAX, SURE: as in wmrb_user_fused_kernel.  HITS: accidental hits leave the sums; the plain instantiations carry none of it --
// no id reload, no hit test, no kept flag.
template <int ITERS, int RMAX, int SURE, bool HITS>
__global__ __launch_bounds__(256, (ITERS == 1 && RMAX == 16) ? 4 : 1) void bpr_user_fused_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ ub, const float* __restrict__ ib,
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ xi, const int32_t* __restrict__ pos_slot,
    const int32_t* __restrict__ samples, int64_t n_users, int32_t S, int d, int32_t max_rows,
    float* __restrict__ loss, float* __restrict__ pred_serial, float* __restrict__ dU, float* __restrict__ dub,
    float* __restrict__ coef_samples, float* __restrict__ coef_pairs, int32_t* __restrict__ sample_hist,
    int32_t* __restrict__ sample_rank)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int mr4 = (max_rows + 3) & ~3;
    const int W = S <= 64 ? 1 : (S <= 128 ? 2 : 4);              // (bpr_sample_waves)
    const int G = 4 / W;
    const int wsum = W * (max_rows - S);                         // entries of one array of wave sums
    float* l_y = lds;
    float* l_coef = l_y + mr4;
    int32_t* l_slot = (int32_t*)(l_coef + mr4);
    int32_t* l_xid = l_slot + mr4;
    float* l_sp = (float*)(l_xid + mr4);                         // [n_pos][W] softplus sums of the waves
    float* l_sg = l_sp + wsum;                                   // [n_pos][W] sigma sums of the waves
    float* l_cs = l_sp + ((2 * wsum + 3) & ~3);                  // [G][64 W] sigma sums per sample and group
    float* l_part = l_cs + 256;
    constexpr int ablate = 0;                                    // (the ablation build is wmrb_fused.hip's alone)

#define USER_FUSED_PART 1
#include "user_fused_body.hpp"
#undef USER_FUSED_PART

    // interaction `tid` of this user (n_pos <= 255): its slot (and, for the hit test, its item) are fetched now, used in phase (c);
    // with HITS a lane looks at the sample it owns in that phase: its id again (an L1 / L2 hit)
    const int grp = wave / W, wg = wave - grp * W;
    const int my_s = 64 * wg + lane;                             // the sample this lane owns in phase (c)
    const int qi = tid < n_pos ? tid : n_pos - 1;
    const int32_t slot_ld = pos_slot[b + qi];
    const int32_t xi_ld = HITS ? xi[b + qi] : 0;
    const int32_t my_sample = HITS ? samples[u * S + (my_s < S ? my_s : S - 1)] : 0;
    const int32_t my_slot = (tid < n_pos) ? slot_ld : -1;

#define USER_FUSED_PART 2
#include "user_fused_body.hpp"
#undef USER_FUSED_PART
    // the slots the groups walk, and the columns a sample is tested against: the user's interactions with pos_slot >= 0, -1 (no
    // item) for the others and for the padding up to a multiple of four
    const int np4 = (n_pos + 3) & ~3;
    if (tid < np4) {
        l_slot[tid] = my_slot;
        if (HITS) l_xid[tid] = hit_column(xi_ld, my_slot);
    }
    __syncthreads();

    // ---- (c) loss terms and coefficients: group grp walks the interactions q = grp (mod G), lane my_s % 64 of its wave wg owns sample my_s ----
    const float inv_s = 1.0f / (float)S;
    bool mine = my_s < S;                                        // this lane's sample is kept
    if (HITS) {
        bool hit;
        HIT_SCAN4(hit, l_xid, np4, my_sample);
        mine = mine && !hit;
    }
    if (64 * wg < S) {                                           // (wave-uniform: a wave of padding only has nothing to add; no barrier inside)
        const float ys = l_y[my_s < S ? my_s : S - 1];
        float cs = 0.f;
        for (int q = grp; q < n_pos; q += G) {
            if (l_slot[q] < 0) continue;                         // (uniform over the workgroup: broadcast reads)
            const float x = ys - l_y[S + q];
            float sp, sg;
            softplus_sigmoid_f(x, sp, sg);
            sp = mine ? sp : 0.f;
            sg = mine ? sg : 0.f;
            cs += sg;                                            // interaction order inside the group
            const float tp = wave_sum(sp), tg = wave_sum(sg);
            if (lane == 0) {
                l_sp[q * W + wg] = tp;
                l_sg[q * W + wg] = tg;
            }
        }
        l_cs[grp * (64 * W) + my_s] = cs;
    }
    __syncthreads();
    if (tid < n_pos) {
        float lo = 0.f, dp = 0.f;
        if (my_slot >= 0) {
            const int nw = (S + 63) >> 6;                        // the waves that hold samples
            float tp = l_sp[tid * W], tg = l_sg[tid * W];
            for (int w = 1; w < nw; ++w) {
                tp += l_sp[tid * W + w];
                tg += l_sg[tid * W + w];
            }
            lo = tp * inv_s;
            dp = -(tg * inv_s);
            loss[my_slot] = lo;
        }
        l_coef[S + tid] = dp;
        coef_pairs[b + tid] = dp;
    }
    if (tid < S) {
        float cs = l_cs[tid];
        for (int g = 1; g < G; ++g) cs += l_cs[g * (64 * W) + tid];
        cs = cs * inv_s;
        l_coef[tid] = cs;
        coef_samples[u * S + tid] = cs;
    }
    __syncthreads();

#define USER_FUSED_PART 3
#include "user_fused_body.hpp"
#undef USER_FUSED_PART
}

}  // namespace

// Dynamic LDS the fused BPR step needs, or -1 if the configuration is not covered (the host then runs the generic step): the
// coverage of trec_softmax_fused_lds_bytes -- 1 <= n_sampled <= 256, d % 4 == 0, 4 <= d <= 256, n_sampled + the longest interaction
// row <= 256 (128 for d > 128) --, the bytes of the layout in the header comment (more than the softmax step's: the wave sums and
// the sample partials of the loss phase).
extern "C" int trec_bpr_fused_lds_bytes(int32_t n_sampled, int32_t max_interactions_per_user, int32_t d)
{
    const int64_t r4 = covered_rows4(n_sampled, max_interactions_per_user, d);
    if (r4 < 0) return -1;
    const int64_t sums = (2 * (int64_t)bpr_sample_waves(n_sampled) * max_interactions_per_user + 3) & ~(int64_t)3;
    return (int)((4 * r4 + sums + 256 + 8 * (int64_t)d) * 4);
}

extern "C" int trec_bpr_fused_step(const float* U, const float* V, const float* user_bias, const float* item_bias,
                                   const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot, const int32_t* samples,
                                   int64_t n_users, int64_t n_items, int32_t n_sampled, int32_t d,
                                   int32_t max_interactions_per_user, int32_t remove_hits, float* loss, float* pred_serial,
                                   float* dU, float* d_user_bias, float* coef_samples, float* coef_pairs, int32_t* sample_hist,
                                   int32_t* sample_rank, void* stream)
{
    (void)n_items;
    USER_FUSED_REQUIRE_POINTERS("trec_bpr_fused_step");
    USER_FUSED_REQUIRE_PAIRS("trec_bpr_fused_step");
    TREC_REQUIRE(!remove_hits || (x_item && pos_slot), "trec_bpr_fused_step: remove_hits needs the interaction arrays");
    USER_FUSED_COVERED("trec_bpr_fused_step", trec_bpr_fused_lds_bytes);
#define TREC_FUSED_K(IT, RM, SU, HITS)                                                                                        \
    hipLaunchKernelGGL((bpr_user_fused_kernel<IT, RM, SU, HITS>), dim3((unsigned)n_users), dim3(256), lds, st, U, V, user_bias, \
                       item_bias, indptr, x_item, pos_slot, samples, n_users, n_sampled, d, max_rows, loss, pred_serial, dU,  \
                       d_user_bias, coef_samples, coef_pairs, sample_hist, sample_rank)
#define TREC_FUSED(IT, RM, SU)                                                                                                 \
    do {                                                                                                                       \
        if (remove_hits) TREC_FUSED_K(IT, RM, SU, true);                                                                       \
        else TREC_FUSED_K(IT, RM, SU, false);                                                                                  \
    } while (0)
    USER_FUSED_LAUNCH("trec_bpr_fused_step");
#undef TREC_FUSED
#undef TREC_FUSED_K
}
