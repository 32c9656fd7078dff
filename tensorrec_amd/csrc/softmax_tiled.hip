// tensorrec_amd/csrc/softmax_tiled.hip -- the one-pass sampled-softmax step for users whose rows do NOT fit in registers, for S in the
// thousands and for Euclidean scores: the step of csrc/softmax_fused.hip on the frame of csrc/wmrb_tiled.hip.
//
// A 256-thread workgroup owns a user.  Pass 1 keeps the user's row in registers and streams its S + n_u item rows in tiles; every
// score stays in LDS.  The loss phase runs from LDS; pass 2 streams the rows once more and sums them with their values into dU.
// Both passes ARE wmrb_tiled_user's (the text parts of csrc/tiled_pass_parts.hpp), and so are the outputs (TiledOut): loss, serial
// predictions, dU or the row sum, d b_u, per pair the value the item side sums (dot: the coefficient g; Euclidean: c = -g / sqrt(D),
// 0 where D < 1e-16 -- the convention of pair_score.hip), the raw g for Euclidean scores with item biases, the optional dense G.
//
// The loss phase (docs/sampled_losses.md, "Formulas" and "Definitions"; upstream gradient 1; t = 1 / temperature) is O(S + n_u):
//     plain      M = max_s y_s, Z = sum_s exp((y_s - M) t);  per positive  ssm_terms: m = max(M, y_p), a = exp((y_p - m) t),
//                b = exp((M - m) t), D = a + b Z:  loss_p = (m - y_p) t + log D,  g_p = -t b Z / D,  K_u = sum_p b_p / D_p,
//                g_s = t exp((y_s - M) t) K_u
//     adjusted   kept = not a hit;  c_s = -(log S + log q(item_s)) with the correction, else 0;  R = max_kept y_s,
//                w_s = (y_s - R) t + c_s, M = max_kept w_s, Z = sum_kept exp(w_s - M), w_p = (y_p - R) t, then ssm_terms on
//                (w_p, M, Z) with t = 1;  g_p = -t b Z / D, g_s = t exp(w_s - M) K_u for a kept sample and exactly 0 for a hit;
//                no kept sample: loss_p = 0 and every coefficient of the user is 0
// Thread tid owns the samples tid, tid + 256, ... and the interactions tid, tid + 256, ..., each walked in ascending order; the
// threads' partials of M, Z, K_u (and R) are joined by the butterfly pair of csrc/sampled_common.hpp (xor butterfly inside a wave,
// the four waves as (0 + 1) + (2 + 3)).  No float atomics except the adds into dense_g: everything else a call writes is
// bit-identical between two calls.  expf / logf are the library's (no fast-math).
//
// One more LDS array than the scores and values, l_w [S]: exp((y_s - M) t) between the Z sweep and the coefficient sweep; adjusted:
// first c_s, or -inf for a hit (decided ONCE per sample by its owner: row_is_hit's binary search through x_item[b..e) and one
// log_q gather), then w_s, then exp(w_s - M) -- a hit stays -inf / 0 through all three.  Recomputing mask and c_s instead would
// save 4 S bytes of LDS and repeat the search and the gather in three sweeps (R, M, Z / coefficients).
#include "wmrb_tiled_body.hpp"  // dpp_add, TiledOut, tiled_subgroups, EUCLID_EPS
#include "sampled_common.hpp"   // row_is_hit, ssm_terms, logq_correction, the butterfly reductions, temperature_ok

namespace {

// floats of dynamic LDS: y [mr4] | cf [mr4] | w [ms4] | partial dU [subgroups][d] | red [24]
__host__ __device__ inline int64_t softmax_tiled_lds_floats(int64_t n_sampled, int64_t max_pos, int d)
{
    const int64_t mr4 = (n_sampled + max_pos + 3) & ~(int64_t)3, ms4 = (n_sampled + 3) & ~(int64_t)3;
    return 2 * mr4 + ms4 + (int64_t)tiled_subgroups(d) * d + 24;
}

// ITERS, RB, MODE, LPR: as in wmrb_user_tiled_kernel.  ADJ: the adjusted loss phase (use_q: the logQ correction, no_hits: accidental
// hits leave the sums); the plain instantiations carry none of it -- no id reload, no log q gather, no hit test.
template <int ITERS, int RB, int MODE, int LPR, bool ADJ>
__global__ __launch_bounds__(256, ITERS <= 2 ? 4 : 2) void softmax_user_tiled_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ ub, const float* __restrict__ ib,
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ xi, const int32_t* __restrict__ pos_slot,
    const int32_t* __restrict__ samples, const float* __restrict__ log_q, int64_t n_users, int32_t S, int d, float t, float log_s,
    float log_uniform, int use_q, int no_hits, int32_t max_rows, TiledOut o)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t u = blockIdx.x;
    const int32_t* samp = samples + u * S;
    const int mr4 = (max_rows + 3) & ~3, ms4 = (S + 3) & ~3;
    float* l_y = lds;
    float* l_cf = l_y + mr4;
    float* l_w = l_cf + mr4;
    float* l_part = l_w + ms4;
    constexpr int NSG = 256 / LPR;                       // subgroups of the workgroup
    float* l_red = l_part + NSG * d;                     // [0, 8): part 2's; [8, 24): R, M, Z, K of the loss phase

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int sub = tid & (LPR - 1), sg = tid / LPR;
    const int64_t b = indptr[u], e = indptr[u + 1];
    const int n_pos = (int)(e - b);
    const int R = S + n_pos;

#define TILED_PASS_PART 1
#include "tiled_pass_parts.hpp"
#undef TILED_PASS_PART

    // ---- the loss phase: (R,) M, Z over the samples; the interactions; the samples' coefficients ----
    float Rm = 0.f, M, Z;
    bool dead = false;                                       // (uniform) every sample of this user is a hit
    if (!ADJ) {
        float mx = -INFINITY;
        for (int s = tid; s < S; s += 256) mx = fmaxf(mx, l_y[s]);
        M = wg_max_butterfly(mx, l_red + 12);
        float z = 0.f;
        for (int s = tid; s < S; s += 256) {
            const float E = expf((l_y[s] - M) * t);
            l_w[s] = E;
            z += E;
        }
        Z = wg_sum_butterfly(z, l_red + 16);
    } else {
        float rx = -INFINITY;
        for (int s = tid; s < S; s += 256) {
            const int32_t item = samp[s];
            const bool hit = no_hits && row_is_hit(xi, pos_slot, b, e, item);      // (no_hits: uniform)
            const float c = use_q ? logq_correction(log_s, log_q ? log_q[item] : log_uniform) : 0.f;
            l_w[s] = hit ? -INFINITY : c;
            rx = hit ? rx : fmaxf(rx, l_y[s]);
        }
        Rm = wg_max_butterfly(rx, l_red + 8);
        dead = Rm == -INFINITY;
        M = 0.f;
        Z = 0.f;
        if (!dead) {
            float mx = -INFINITY;
            for (int s = tid; s < S; s += 256) {
                const float w = (l_y[s] - Rm) * t + l_w[s];  // (a hit: finite + -inf = -inf)
                l_w[s] = w;
                mx = fmaxf(mx, w);
            }
            M = wg_max_butterfly(mx, l_red + 12);
            float z = 0.f;
            for (int s = tid; s < S; s += 256) {
                const float E = expf(l_w[s] - M);            // 0 for a hit
                l_w[s] = E;
                z += E;
            }
            Z = wg_sum_butterfly(z, l_red + 16);
        }
    }
    float raw_sum = 0.f;                                     // this thread's share of d b_u = sum of every pair's g
    float val_sum = 0.f;                                     // ... and of the sum of the values (euclidean: dU = val_sum U - G . V)
    float term = 0.f;                                        // ... and of K_u
    for (int q = tid; q < n_pos; q += 256) {
        const int32_t slot = pos_slot[b + q];
        const int32_t xi_ld = xi[b + q];
        const float yp = l_y[S + q];
        float dp = 0.f;
        if (slot >= 0) {
            if (dead) {
                o.loss[slot] = 0.f;
            } else {
                float m, bb, bz, D;
                if (!ADJ) {
                    ssm_terms(yp, M, Z, t, m, bb, bz, D);
                    o.loss[slot] = (m - yp) * t + logf(D);
                } else {
                    const float wp = (yp - Rm) * t;
                    ssm_terms(wp, M, Z, 1.0f, m, bb, bz, D);
                    o.loss[slot] = (m - wp) + logf(D);
                }
                dp = -t * (bz / D);
                term += bb / D;
            }
        }
        float val = dp;
        if (MODE == 1) { const float D = l_cf[S + q]; val = (D >= EUCLID_EPS) ? -dp / sqrtf(D) : 0.f; }
        l_cf[S + q] = val;
        if (o.val_pairs) o.val_pairs[b + q] = val;
        if (o.raw_pairs) o.raw_pairs[b + q] = dp;
        if (o.dense_g) unsafeAtomicAdd(o.dense_g + u * o.ldg + xi_ld, val);
        raw_sum += dp;
        val_sum += val;
    }
    const float K = wg_sum_butterfly(term, l_red + 20);      // a non-positive interaction or an idle thread adds an exact 0
    for (int s = tid; s < S; s += 256) {
        const float g = dead ? 0.f : (t * l_w[s]) * K;       // a hit: l_w = 0, an exact 0
        float val = g;
        if (MODE == 1) { const float D = l_cf[s]; val = (D >= EUCLID_EPS) ? -g / sqrtf(D) : 0.f; }
        l_cf[s] = val;
        if (o.val_samples) o.val_samples[u * S + s] = val;
        if (o.raw_samples) o.raw_samples[u * S + s] = g;
        if (o.dense_g) unsafeAtomicAdd(o.dense_g + u * o.ldg + samp[s], val);
        raw_sum += g;
        val_sum += val;
    }
    __syncthreads();

#define TILED_PASS_PART 2
#include "tiled_pass_parts.hpp"
#undef TILED_PASS_PART
}

constexpr int64_t SOFTMAX_TILED_MAX_LDS = 128 * 1024;

}  // namespace

// Dynamic LDS of trec_softmax_tiled_step, or -1 when the configuration is not covered: d % 4 == 0, 4 <= d <= 512, n_sampled >= 1, and
// 2 * (n_sampled + longest interaction row) + n_sampled + 8 * d (16 * d for d <= 64) + 24 floats within 128 KB (one layout for the
// plain and the adjusted loss phase).
extern "C" int trec_softmax_tiled_lds_bytes(int32_t n_sampled, int32_t max_interactions_per_user, int32_t d)
{
    if (n_sampled < 1 || d < 4 || d % 4 != 0 || d > 512 || max_interactions_per_user < 0) return -1;
    const int64_t bytes = softmax_tiled_lds_floats(n_sampled, max_interactions_per_user, d) * 4;
    return bytes <= SOFTMAX_TILED_MAX_LDS ? (int)bytes : -1;
}

extern "C" int trec_softmax_tiled_step(const float* U, const float* V, const float* user_bias, const float* item_bias,
                                       const int64_t* indptr, const int32_t* x_item, const int32_t* pos_slot,
                                       const int32_t* samples, int64_t n_users, int64_t n_items, int32_t n_sampled, int32_t d,
                                       int32_t mode, int32_t max_interactions_per_user, float inv_temperature, const float* log_q,
                                       float log_uniform, int32_t log_q_correction, int32_t remove_hits, float* loss,
                                       float* pred_serial, float* dU, float* d_user_bias, float* val_samples, float* val_pairs,
                                       float* raw_samples, float* raw_pairs, float* dense_g, int64_t ldg, float* val_rowsum,
                                       void* stream)
{
    TREC_REQUIRE(U && V && indptr && samples && loss && pred_serial && val_samples && val_pairs,
                 "trec_softmax_tiled_step: null pointer");
    TREC_REQUIRE(dU || (dense_g && val_rowsum), "trec_softmax_tiled_step: without dU the caller needs dense_g and val_rowsum");
    TREC_REQUIRE(mode == 0 || mode == 1, "trec_softmax_tiled_step: mode must be 0 (dot) or 1 (euclidean)");
    TREC_REQUIRE(temperature_ok(inv_temperature), "trec_softmax_tiled_step: inv_temperature must be finite and > 0");
    TREC_REQUIRE(!user_bias == !d_user_bias, "trec_softmax_tiled_step: user_bias and d_user_bias go together");
    TREC_REQUIRE(!raw_samples == !raw_pairs, "trec_softmax_tiled_step: raw_samples and raw_pairs go together");
    TREC_REQUIRE(!dense_g || ldg >= n_items, "trec_softmax_tiled_step: ldg must cover the items");
    TREC_REQUIRE(!log_q_correction || (n_items >= 1 && n_items < ((int64_t)1 << 31)),
                 "trec_softmax_tiled_step: n_items must lie in [1, 2^31) with the logQ correction");
    TREC_REQUIRE(!remove_hits || (x_item && pos_slot), "trec_softmax_tiled_step: remove_hits needs the interaction arrays");
    const int lds = trec_softmax_tiled_lds_bytes(n_sampled, max_interactions_per_user, d);
    if (lds < 0) {
        trec_set_last_error("trec_softmax_tiled_step: configuration not covered (see trec_softmax_tiled_lds_bytes)");
        return TREC_ERR_UNSUPPORTED;
    }
    if (n_users == 0) return TREC_OK;
    TREC_REQUIRE(max_interactions_per_user == 0 || (x_item && pos_slot), "trec_softmax_tiled_step: null interaction arrays");
    const float log_s = (float)log((double)n_sampled);
    const int use_q = log_q_correction ? 1 : 0, no_hits = remove_hits ? 1 : 0;
    const bool adj = use_q || no_hits;
    const int32_t max_rows = n_sampled + max_interactions_per_user;
    hipStream_t st = (hipStream_t)stream;
    TiledOut o = {loss, pred_serial, dU, d_user_bias, val_samples, val_pairs, raw_samples, raw_pairs, dense_g, ldg, val_rowsum};
#define TREC_TILED_K(IT, RB, MD, LP, ADJ)                                                                                          \
    do {                                                                                                                           \
        if (lds > 64 * 1024)                                                                                                       \
            (void)hipFuncSetAttribute((const void*)softmax_user_tiled_kernel<IT, RB, MD, LP, ADJ>,                                 \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)SOFTMAX_TILED_MAX_LDS);                     \
        hipLaunchKernelGGL((softmax_user_tiled_kernel<IT, RB, MD, LP, ADJ>), dim3((unsigned)n_users), dim3(256), lds, st, U, V,    \
                           user_bias, item_bias, indptr, x_item, pos_slot, samples, use_q ? log_q : (const float*)nullptr, n_users, \
                           n_sampled, d, inv_temperature, log_s, log_uniform, use_q, no_hits, max_rows, o);                        \
    } while (0)
#define TREC_TILED(IT, RB, MD, LP)                                                                                                 \
    do {                                                                                                                           \
        if (adj) TREC_TILED_K(IT, RB, MD, LP, true);                                                                               \
        else TREC_TILED_K(IT, RB, MD, LP, false);                                                                                  \
    } while (0)
    if (mode == 0) {
        if (d <= 64) TREC_TILED(1, 12, 0, 16);
        else if (d <= 128) TREC_TILED(1, 12, 0, 32);
        else if (d <= 256) TREC_TILED(2, 8, 0, 32);
        else TREC_TILED(4, 4, 0, 32);
    } else {
        if (d <= 64) TREC_TILED(1, 12, 1, 16);
        else if (d <= 128) TREC_TILED(1, 12, 1, 32);
        else if (d <= 256) TREC_TILED(2, 8, 1, 32);
        else TREC_TILED(4, 4, 1, 32);
    }
#undef TREC_TILED
#undef TREC_TILED_K
    return trec_check_launch("trec_softmax_tiled_step");
}
