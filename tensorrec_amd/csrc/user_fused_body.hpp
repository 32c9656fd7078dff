// tensorrec_amd/csrc/user_fused_body.hpp -- what the one-pass per-user training steps share, as TEXT: csrc/wmrb_fused.hip,
// csrc/softmax_fused.hip, csrc/warp_fused.hip and csrc/bpr_fused.hip include it once at file scope for the helpers and the host section (the entry
// checks, the coverage and the instantiation ladder of their entry points) and three times inside their kernel
// (template <int ITERS, int RMAX, int SURE, ...>), each time with one USER_FUSED_PART defined:
//     USER_FUSED_PART 1   the prologue: thread indices, the sample ids, the user's interaction range, the user without interactions
//     USER_FUSED_PART 2   phases (a), (b): the user's row and its R = S + n_pos item rows into registers, predictions into l_y (and
//                         pred_serial), the histogram atomics
//     USER_FUSED_PART 3   phase (d) and the epilogue: dU from the registers through 8 LDS partials, d b_u = the sum of l_coef, the ranks
// The kernel puts its own loads between parts 1 and 2 and its loss phase (c), framed by __syncthreads(), between parts 2 and 3.  The
// parts are the text wmrb_user_fused_kernel held before the softmax step existed, so that kernel compiles to the code it always did
// (a version with forced-inline functions allocated registers differently).  No include guard on purpose.
// Names the parts expect in scope: the kernel parameters U, V, ub, ib, indptr, xi, samples, n_users, S, d, pred_serial, dU, dub,
// coef_samples, sample_hist, sample_rank, ablate; the LDS arrays l_y [R], l_coef [R] (complete before part 3), l_part [8][d].
// USER_FUSED_SIDE (optional, a compile-time condition): the owner lane of a SAMPLE row also fetches side[item] (side == null:
// side_uniform) in the batch of the item bias and leaves it in l_side[j], j < S -- log q of the sampled softmax.
#ifndef USER_FUSED_PART
#include "common.hpp"
#include <math.h>

namespace {

// sum over the 32 lanes of a subgroup with DPP adds (one VALU instruction each, no LDS crossbar): four rotations
// inside the 16-lane rows, then row_bcast15 carries row 0's total into row 1 -- the full sum is valid in lanes 16..31
// of the subgroup (read it from lane 31).  ds_bpermute-based __shfl_xor costs ~5x more issue slots and latency here.
__device__ __forceinline__ float dpp_add(float x, const int ctrl_tag)
{
    int v = __float_as_int(x), r;
    switch (ctrl_tag) {
        case 8: r = __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false); break;    // row_ror:8
        case 4: r = __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false); break;    // row_ror:4
        case 2: r = __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false); break;    // row_ror:2
        case 1: r = __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false); break;    // row_ror:1
        default: r = __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); break;   // row_bcast15 into rows 1, 3
    }
    return x + __int_as_float(r);
}

// A/B switches of the gather (variant libraries: -DTREC_WMRB_NT / -DTREC_WMRB_NO_EARLY).  Non-temporal row loads were MEASURED
// slower (13.5 ms against 11.4 for the whole kernel at 1M x 1M, profiles/r05_wmrb_fused_ab.txt): the rows are read once per pair,
// but `nt` loads of 16 B per lane did not stream past the L2 any cheaper -- plain loads stay the default.
#ifdef TREC_WMRB_NT
#define TREC_ROW_LOAD(p) __builtin_nontemporal_load(p)
#else
#define TREC_ROW_LOAD(p) (*(p))
#endif

// The ablation switches of scripts/bench_fused_ablate.py (histogram atomics / loss phases / dU off: WRONG results, only the
// time is read) exist only in a build with -DTREC_WMRB_ABLATE; the shipped kernel has none of the branches and no tuning
// lookup per launch (a knob left set would train wrong gradients silently).
#ifdef TREC_WMRB_ABLATE
#define TREC_ABLATED(bit) (ablate & (bit))
#else
#define TREC_ABLATED(bit) false
#endif

static int rows_capacity(int d) { return d <= 128 ? 256 : 128; }      // 8 subgroups x RMAX rows

// n_sampled <= 256, d % 4 == 0, 4 <= d <= 256, n_sampled + the longest interaction row <= 256 (128 for d > 128): the rows of a user
// live in the registers of its workgroup.  Returns the rows rounded up to 4, or -1 where the shape is not covered.
static int64_t covered_rows4(int32_t n_sampled, int32_t max_interactions_per_user, int32_t d)
{
    if (n_sampled < 1 || n_sampled > 256 || d < 4 || d % 4 != 0 || d > 256 || max_interactions_per_user < 0) return -1;
    const int64_t rows = (int64_t)n_sampled + max_interactions_per_user;
    if (rows > rows_capacity(d)) return -1;
    return (rows + 3) & ~(int64_t)3;
}

// dynamic LDS of the softmax and WARP steps (one layout: four arrays of rows4, 16 words of reductions / kept mask, partial dU [8][d])
static int fused_lds_bytes(int32_t n_sampled, int32_t max_interactions_per_user, int32_t d)
{
    const int64_t r4 = covered_rows4(n_sampled, max_interactions_per_user, d);
    return r4 < 0 ? -1 : (int)((4 * r4 + 16 + 8 * (int64_t)d) * 4);
}

}  // namespace

// ---- host: what the entry points trec_<loss>_fused_step share, as macros over the parameter names all three use.  An entry point is
//     USER_FUSED_REQUIRE_POINTERS(name);  USER_FUSED_REQUIRE_PAIRS(name);  its own TREC_REQUIREs, in the order it always had them (the
//     softmax step's temperature check stands between the two);  USER_FUSED_COVERED(name, lds_bytes);  its constants and
//     #define TREC_FUSED(IT, RM, SU) <launch of that instantiation>;  USER_FUSED_LAUNCH(name);  #undef TREC_FUSED
#define USER_FUSED_REQUIRE_POINTERS(name) \
    TREC_REQUIRE(U && V && indptr && samples && loss && pred_serial && dU && coef_samples && coef_pairs, name ": null pointer")
#define USER_FUSED_REQUIRE_PAIRS(name)                                                                                         \
    TREC_REQUIRE(!user_bias == !d_user_bias, name ": user_bias and d_user_bias go together");                                  \
    TREC_REQUIRE(sample_hist || !sample_rank, name ": sample_rank needs sample_hist")

// defines lds, max_rows and st; leaves with TREC_ERR_UNSUPPORTED where the shape is not covered (the host then runs the generic step)
#define USER_FUSED_COVERED(name, lds_bytes)                                                                                    \
    const int lds = lds_bytes(n_sampled, max_interactions_per_user, d);                                                        \
    if (lds < 0) {                                                                                                             \
        trec_set_last_error(name ": configuration not covered (see " #lds_bytes ")");                                          \
        return TREC_ERR_UNSUPPORTED;                                                                                           \
    }                                                                                                                          \
    if (n_users == 0) return TREC_OK;                                                                                          \
    TREC_REQUIRE(max_interactions_per_user == 0 || (x_item && pos_slot), name ": null interaction arrays");                    \
    const int32_t max_rows = n_sampled + max_interactions_per_user;                                                            \
    hipStream_t st = (hipStream_t)stream

// register rows r < sure hold samples in every subgroup (8 r + 7 < S)
#ifdef TREC_WMRB_NO_EARLY
#define USER_FUSED_SURE(n_sampled) 0
#else
#define USER_FUSED_SURE(n_sampled) ((n_sampled) / 8)
#endif

// the <ITERS, RMAX, SURE> instantiations (tests/softmax_step_reference.py mirrors this ladder)
#define USER_FUSED_LAUNCH(name)                                                                                                \
    const int sure = USER_FUSED_SURE(n_sampled);                                                                               \
    if (d <= 128 && max_rows <= 128) {                                                                                         \
        if (sure >= 12) TREC_FUSED(1, 16, 12);                                                                                 \
        else if (sure >= 8) TREC_FUSED(1, 16, 8);                                                                              \
        else if (sure >= 4) TREC_FUSED(1, 16, 4);                                                                              \
        else TREC_FUSED(1, 16, 0);                                                                                             \
    } else if (d <= 128) {                                                                                                     \
        if (sure >= 16) TREC_FUSED(1, 32, 16);                                                                                 \
        else TREC_FUSED(1, 32, 0);                                                                                             \
    } else {                                                                                                                   \
        if (sure >= 8) TREC_FUSED(2, 16, 8);                                                                                   \
        else TREC_FUSED(2, 16, 0);                                                                                             \
    }                                                                                                                          \
    return trec_check_launch(name)

#elif USER_FUSED_PART == 1
    const int64_t u = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int sub = tid & 31, sg = tid >> 5;             // 8 subgroups of 32 lanes
    // Every load of the gather phase is UNCONDITIONAL, from a clamped (always valid) address, and selected afterwards: written
    // as `cond ? load : 0` the compiler wraps each load in an exec-masked block that ends in s_waitcnt vmcnt(0) -- the 16 loads
    // of the interaction ids, the biases, the user row and the histogram atomic became ~10 SERIAL round trips per user where
    // three dependent ones are needed (ids -> rows / biases -> atomics; the refining launch of the top-k cascade had the same
    // disease).  Rows past R read item 0 and are never used unguarded (predictions not written, dU sum guarded).
    // The sampled item ids do not depend on the user's interaction range: their loads leave together with indptr's.
    int32_t item[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int j = sg + 8 * r;
        item[r] = samples[u * S + (j < S ? j : S - 1)];
    }
    const int64_t b = indptr[u], e = indptr[u + 1];
    const int n_pos = (int)(e - b);
    const int R = S + n_pos;                             // rows of this user: samples first, then interactions

    if (n_pos == 0) {
        // no interactions: no loss terms, every coefficient is 0 (the samples of this user are never used)
        for (int s = tid; s < S; s += 256) {
            coef_samples[u * S + s] = 0.f;
            if (sample_hist) {                                                   // the sort still sees these pairs
                const int32_t rk = atomicAdd(sample_hist + samples[u * S + s], 1);
                if (sample_rank) sample_rank[u * S + s] = rk;
            }
        }
        for (int c = tid; c < d; c += 256) dU[u * d + c] = 0.f;
        if (dub && tid == 0) dub[u] = 0.f;
        return;
    }

#elif USER_FUSED_PART == 2
    // ---- (a) the user's row, in the registers of every subgroup ----
    f32x4 x[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * 32 + sub) * 4;
        const f32x4 v = TREC_ROW_LOAD((const f32x4*)(U + u * d + (c < d ? c : 0)));
        x[it] = (c < d) ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const float bu = ub ? ub[u] : 0.f;

    // ---- (b) every subgroup gathers its rows j = sg + 8 r (r < RMAX) in ONE batch and keeps them ----
    f32x4 y[RMAX][ITERS];
    // the rows that are samples for certain first: their addresses need nothing but the sample ids
#pragma unroll
    for (int r = 0; r < SURE; ++r) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * 32 + sub) * 4;
            y[r][it] = TREC_ROW_LOAD((const f32x4*)(V + (int64_t)item[r] * d + (c < d ? c : 0)));
        }
    }
    {
        int32_t xid[RMAX];                               // the interaction item of row j >= S (n_pos >= 1 here)
#pragma unroll
        for (int r = SURE; r < RMAX; ++r) {
            const int q = sg + 8 * r - S;
            xid[r] = xi[b + (q < 0 ? 0 : (q < n_pos ? q : n_pos - 1))];
        }
#pragma unroll
        for (int r = SURE; r < RMAX; ++r) {
            const int j = sg + 8 * r;
            item[r] = (j < S) ? item[r] : ((j < R) ? xid[r] : 0);
        }
    }
    // Lane 16 + (r & 15) of a subgroup OWNS the subgroup's row r (lanes 16..31 are where the DPP reduction leaves the
    // 32-lane dot product): it fetches the row's item bias -- in the same batch of loads as the rows --, issues the row's
    // histogram atomic and writes its prediction; none of that costs RMAX registers in every lane.
    constexpr int H = RMAX / 16;
    const int own = sub - 16;
    float my_bi[H];
#ifdef USER_FUSED_SIDE
    float my_side[H];
#endif
    int32_t my_item[H];                                  // the item of the owned row: picked from the ids every lane holds
    // (16 v_cndmask per owned row instead of two more loads: written as loads -- samples / xi again at the owner's index -- the
    // compiler sank the xi one into an exec-masked block ending in s_waitcnt vmcnt(0), one more dependent round trip in front of
    // the bias load and, with the early rows above, a wait for ALL of them before the last rows could leave)
#pragma unroll
    for (int h = 0; h < H; ++h) {
        int32_t mine = 0;
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) mine = (own == r16) ? item[r16 + 16 * h] : mine;
        my_item[h] = mine;                               // (rows past R hold item 0: a valid address, never used unguarded)
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int j = sg + 8 * (own + 16 * h);
        const float v = ib ? ib[my_item[h]] : 0.f;           // (uniform branch)
        my_bi[h] = (own >= 0 && j < R) ? v : 0.f;
#ifdef USER_FUSED_SIDE
        if (USER_FUSED_SIDE) my_side[h] = side ? side[my_item[h]] : side_uniform;     // (uniform branch; item 0 past R: a valid address)
#endif
    }
#pragma unroll
    for (int r = SURE; r < RMAX; ++r) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * 32 + sub) * 4;
            y[r][it] = TREC_ROW_LOAD((const f32x4*)(V + (int64_t)item[r] * d + (c < d ? c : 0)));
        }
    }
    if (d < ITERS * 128) {                               // (uniform: columns past d contribute zeros)
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
                if ((it * 32 + sub) * 4 >= d) y[r][it] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    // predictions: no per-row branch (a wave holds two subgroups with different rows), so the RMAX reduction chains
    // interleave; rows past R are zeros and are simply not written
    float dot[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            acc = fmaf(x[it].x, y[r][it].x, acc); acc = fmaf(x[it].y, y[r][it].y, acc);
            acc = fmaf(x[it].z, y[r][it].z, acc); acc = fmaf(x[it].w, y[r][it].w, acc);
        }
        dot[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        float t = dot[r];
        t = dpp_add(t, 8); t = dpp_add(t, 4); t = dpp_add(t, 2); t = dpp_add(t, 1);
        dot[r] = dpp_add(t, 0);                            // lanes 16..31 of the subgroup: the 32-lane total
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        float mine = 0.f;
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) mine = (own == r16) ? dot[r16 + 16 * h] : mine;
        const int j = sg + 8 * (own + 16 * h);
        if (own >= 0 && j < R) {
            float s = mine;
            if (ub) s = s + bu;
            if (ib) s = s + my_bi[h];
            l_y[j] = s;
            if (j >= S) pred_serial[b + (j - S)] = s;
#ifdef USER_FUSED_SIDE
            if (USER_FUSED_SIDE && j < S) l_side[j] = my_side[h];
#endif
        }
    }
    // histogram of the counting sort to come, by the owner lanes: ONE atomic instruction per subgroup and 16 rows instead
    // of RMAX from lane 0.  The value an atomic returns is the pair's rank inside its item's bucket, which makes the sort's
    // fill pass atomic-free; it is stored at the very end of the kernel.  Issued AFTER the rows have been consumed: returning
    // atomics and loads come back in order, so an atomic issued between the row loads and their first use is waited for first
    // (rk stays UNDEFINED for lanes that issue none: merging it with a constant would put the wait right here).
    int32_t rk[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int j = sg + 8 * (own + 16 * h);
        if (sample_hist && own >= 0 && j < S && !TREC_ABLATED(1))
            rk[h] = __hip_atomic_fetch_add(sample_hist + my_item[h], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

#elif USER_FUSED_PART == 3
    // ---- (d) dU_u = sum_j coef_j * V_row_j: every subgroup sums ITS rows from registers, 8 partials meet in LDS ----
    {
        f32x4 part[ITERS];
#pragma unroll
        for (int it = 0; it < ITERS; ++it) part[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const int j = sg + 8 * r;
            if (j < R && !TREC_ABLATED(4)) {
                const float cf = l_coef[j];
#pragma unroll
                for (int it = 0; it < ITERS; ++it) {
                    part[it].x = fmaf(cf, y[r][it].x, part[it].x); part[it].y = fmaf(cf, y[r][it].y, part[it].y);
                    part[it].z = fmaf(cf, y[r][it].z, part[it].z); part[it].w = fmaf(cf, y[r][it].w, part[it].w);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * 32 + sub) * 4;
            if (c < d) *(f32x4*)(l_part + sg * d + c) = part[it];
        }
    }
    __syncthreads();
    for (int c = tid; c < d; c += 256) {
        float acc = l_part[c];
#pragma unroll
        for (int g8 = 1; g8 < 8; ++g8) acc += l_part[g8 * d + c];
        dU[u * d + c] = acc;
    }
    if (dub && wave == 0) {
        float acc = 0.f;
        for (int j = lane; j < R; j += 64) acc += l_coef[j];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) dub[u] = acc;
    }
    if (sample_hist && sample_rank && own >= 0 && !TREC_ABLATED(1)) {
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int j = sg + 8 * (own + 16 * h);
            if (j < S) sample_rank[u * S + j] = rk[h];
        }
    }
#endif
