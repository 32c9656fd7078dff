// tensorrec_amd/csrc/candidate_sets.hip -- scores, exact top-k and pair ranks restricted to per-user candidate sets
// (docs/candidate_sets.md).
//
// The candidates of a call arrive as one CSR in the convention of exclude.hip: ptr int64 [n_rows + 1] (absolute positions into idx),
// idx int32 sorted ascending and de-duplicated within a row, `rows` (nullable) mapping the call's row r to its CSR row rows[r].
//
// A. trec_candset_scores.  out[p] = the exact score of (user of p's segment, idx[p]) for every listed pair, in CSR order: bit for bit
//    the chain of pair_score_exact_kernel (score_rank.hip) -- one __fmaf_rn chain in k order over kdim, the Euclidean transform,
//    + b_u, + b_i.  That kernel gives a pair to a thread, which walks two rows alone: 64 lanes touch 64 rows per load.  Here a wave
//    owns tiles of 64 consecutive pairs.  The item rows of a tile are fetched 64 columns at a time with a row across 16 consecutive
//    lanes (one dwordx4 each, 256 contiguous bytes per row), staged through registers into the wave's LDS tile (row stride 68
//    dwords: ds_read_b128 by lane = row puts the 16 lanes of a read group on 16 different 4-bank slots; the ds_write_b128 of a
//    row's 16 lanes covers 64 consecutive banks), and each lane then walks ITS row in k order.  The loads of the next column block
//    -- or of the next tile's first -- are in flight while a block is computed; eight waves per CU keep eight such blocks (128 KB)
//    in flight.  Users with few candidates share a tile: the segment of a lane is found from ptr (a galloping search from the
//    tile's first segment).  The rows of a tile's first two users are held in LDS (one address for all their lanes: a broadcast);
//    the lanes of further users of the same tile -- segments shorter than 32 -- read their user row from global memory.
//    With `rows` a tile never spans two users (the call's rows are not consecutive in the CSR).
//
// B. trec_candset_topk.  The exact top-k of every segment by (value desc, id asc), padded with -inf / -1, on the uint32 key of
//    csr_select.hpp (-0.0 ties +0.0, a NaN ranks behind -inf).  Segments of at most 256 entries take a wave each: every entry's
//    place is the number of 64-bit (key, ~position) words above it -- idx is sorted, so position order is id order.  Longer
//    segments take one 1,024-thread workgroup each, listed by the host (ptr is a host array there), through the streaming body of
//    trec_topk_rows_excluded (select_row_topk).
//
// C. trec_candset_rank_count.  counts[t] = #{x in C_u, x != t : s_x > s_t or (s_x == s_t and x < t)} for targets grouped by user:
//    trec_exclude_rank_adjust's comparison (listed_ahead), set instead of subtracted.
#include "csr_select.hpp"
#include "exact_finish.hpp"

namespace {

constexpr int CS_KC = 64;                  // columns per staged block
constexpr int CS_LDW = CS_KC + 4;          // LDS row stride in dwords
constexpr int CS_ULDS = 2;                 // users of a tile whose rows are held in LDS
constexpr int CS_KMAX = 256;               // longest chain (the operands of score_prep: d <= 256)
constexpr int CS_WAVES = 4;
constexpr int CS_SHORT = 256;              // longest segment of the wave-per-segment top-k

struct CandScoreArgs {
    const float* U;
    const float* V;
    int64_t ld;
    int kdim;
    const int64_t* ptr;
    const int32_t* idx;
    const int32_t* rows;
    int64_t n_rows;
    int64_t n_items;
    const float* u_bias;
    const float* t_bias;
    int euclid;
    const float* u_sq;
    const float* t_sq;
    float* out;
};

// largest r in [lo, n_rows) with ptr[r] <= p, given ptr[lo] <= p < ptr[n_rows]
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ ptr, int64_t lo, int64_t n_rows, int64_t p)
{
    int64_t step = 1, hi = lo + 1;
    while (hi < n_rows && ptr[hi] <= p) {
        lo = hi;
        step <<= 1;
        hi = lo + step;
    }
    if (hi > n_rows) hi = n_rows;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// what a lane knows of its pair of a tile (lane = row of the LDS tile)
struct CandTile {
    int64_t p;          // position in idx / out
    int64_t u;          // user operand row
    int32_t item;       // item operand row (0 when the lane has no pair)
    int slot;           // rank of the lane's user among the tile's users
    bool ok;            // the lane has a pair with an item id inside the catalogue
    bool has;           // the lane has a pair at all (an id outside the catalogue scores NaN)
    bool head;          // ... and it is the first of its user in the tile
};

__device__ __forceinline__ void cand_tile_finish(const CandScoreArgs& a, CandTile& t, int lane)
{
    int32_t it = t.has ? a.idx[t.p] : 0;
    t.ok = t.has && it >= 0 && (int64_t)it < a.n_items;
    t.item = t.ok ? it : 0;
    const int64_t up = __shfl_up(t.u, 1, TREC_WAVE);
    t.head = t.has && (lane == 0 || up != t.u);
    const unsigned long long heads = __ballot(t.head);
    t.slot = (int)__popcll(heads & ((2ull << lane) - 1ull)) - 1;
    if (t.slot < 0) t.slot = 0;
}

// issue the loads of one column block of a tile: instruction j fetches rows 4j .. 4j + 3, a row across 16 lanes
__device__ __forceinline__ void cand_issue(const CandScoreArgs& a, const CandTile& t, int c0, int kq, int lane, f32x4 (&st)[16])
{
    const int col = c0 + (lane & 15) * 4;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int src = j * 4 + (lane >> 4);
        const int32_t item = __shfl(t.item, src, TREC_WAVE);
        const bool ok = __shfl((int)t.ok, src, TREC_WAVE) != 0;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (ok && col < kq) x = *(const f32x4*)(a.V + (int64_t)item * a.ld + col);
        st[j] = x;
    }
}

template <bool U_LDS>
__device__ __forceinline__ float cand_chain(float acc, const float* __restrict__ tile_row, const float* __restrict__ urow, int c0, int kdim)
{
    const int cend = (kdim - c0) < CS_KC ? (kdim - c0) : CS_KC;        // columns of this block that belong to the chain
    return exact_chain(acc, urow + c0, tile_row, cend, true);
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// PACKED (rows == NULL): tile t of the wave covers positions ptr[0] + 64 t ... of the CSR, whatever users they belong to.
// !PACKED: the wave walks the call's rows w, w + n_waves, ...; a tile is 64 consecutive entries of one row's segment.
template <bool PACKED>
__global__ __launch_bounds__(64 * CS_WAVES, 2) void candset_scores_kernel(const CandScoreArgs a, int64_t tiles_per_wave)
{
    __shared__ __attribute__((aligned(16))) float s_tile[CS_WAVES][64 * CS_LDW];
    __shared__ __attribute__((aligned(16))) float s_user[CS_WAVES][CS_ULDS][CS_KMAX];
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wave = (int64_t)blockIdx.x * CS_WAVES + w;
    const int64_t n_waves = (int64_t)gridDim.x * CS_WAVES;
    float* tile = s_tile[w];
    const int kq = (a.kdim + 3) & ~3;                                   // columns fetched (ld is a multiple of 4)
    const int n_blocks = (a.kdim + CS_KC - 1) / CS_KC;

    // ---- the wave's tile sequence
    const int64_t base = PACKED ? a.ptr[0] : 0, end = PACKED ? a.ptr[a.n_rows] : 0;
    int64_t t_idx = PACKED ? wave * tiles_per_wave : 0;                 // PACKED: tile number
    const int64_t t_end = PACKED ? min((wave + 1) * tiles_per_wave, (end - base + 63) >> 6) : 0;
    int64_t seg_lo = 0;                                                 // PACKED: a segment at or before the next tile's first
    int64_t row = wave, off = 0, rb = 0, re = 0;                        // !PACKED: the call row, the offset inside its segment
    if (!PACKED) {
        while (row < a.n_rows) {
            const int64_t r = (int64_t)a.rows[row];
            rb = a.ptr[r];
            re = a.ptr[r + 1];
            if (re > rb) break;
            row += n_waves;
        }
    }
    auto next_tile = [&](CandTile& t) -> bool {
        if (PACKED) {
            if (t_idx >= t_end) return false;
            const int64_t p0 = base + (t_idx << 6);
            const int64_t first = segment_of(a.ptr, seg_lo, a.n_rows, p0);
            t.p = p0 + lane;
            t.has = t.p < end;
            if (!t.has) t.p = end - 1;
            t.u = segment_of(a.ptr, first, a.n_rows, t.p);
            seg_lo = first;
            ++t_idx;
        } else {
            if (row >= a.n_rows) return false;
            t.p = rb + off + lane;
            t.has = t.p < re;
            if (!t.has) t.p = re - 1;
            t.u = row;
            off += 64;
            if (rb + off >= re) {
                off = 0;
                row += n_waves;
                while (row < a.n_rows) {
                    const int64_t r = (int64_t)a.rows[row];
                    rb = a.ptr[r];
                    re = a.ptr[r + 1];
                    if (re > rb) break;
                    row += n_waves;
                }
            }
        }
        cand_tile_finish(a, t, lane);
        return true;
    };
    // the rows of the tile's first CS_ULDS users, a row across the wave (lane: 4 columns)
    auto issue_users = [&](const CandTile& t, f32x4 (&ur)[CS_ULDS]) {
        unsigned long long m = __ballot(t.head && t.slot < CS_ULDS);
#pragma unroll
        for (int s = 0; s < CS_ULDS; ++s) {
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (m != 0ull) {
                const int src = (int)__builtin_ctzll(m);
                m &= m - 1ull;
                const int64_t u = __shfl(t.u, src, TREC_WAVE);
                if (lane * 4 < kq) x = *(const f32x4*)(a.U + u * a.ld + lane * 4);
            }
            ur[s] = x;
        }
    };

    CandTile cur, nxt;
    f32x4 st[16], ur[CS_ULDS];
    if (!next_tile(cur)) return;
    issue_users(cur, ur);
    cand_issue(a, cur, 0, kq, lane, st);
    for (;;) {
        float acc = 0.0f;
        bool more = false;
        for (int blk = 0; blk < n_blocks; ++blk) {
            // the block that was in flight: registers -> LDS
            if (blk == 0) {
#pragma unroll
                for (int s = 0; s < CS_ULDS; ++s) *(f32x4*)(&s_user[w][s][lane * 4]) = ur[s];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) *(f32x4*)(tile + (j * 4 + (lane >> 4)) * CS_LDW + (lane & 15) * 4) = st[j];
            wave_lds_sync();
            // the next block, or the next tile's first, goes in flight
            if (blk + 1 < n_blocks) {
                cand_issue(a, cur, (blk + 1) * CS_KC, kq, lane, st);
            } else {
                more = next_tile(nxt);
                if (more) {
                    issue_users(nxt, ur);
                    cand_issue(a, nxt, 0, kq, lane, st);
                }
            }
            if (cur.slot < CS_ULDS) acc = cand_chain<true>(acc, tile + lane * CS_LDW, s_user[w][cur.slot], blk * CS_KC, a.kdim);
            else acc = cand_chain<false>(acc, tile + lane * CS_LDW, a.U + cur.u * a.ld, blk * CS_KC, a.kdim);
            wave_lds_sync();
        }
        if (cur.has) {
            float s = acc;
            if (a.euclid) {
                float dist = (a.u_sq[cur.u] - 2.0f * s) + a.t_sq[cur.item];
                dist = fmaxf(dist, 1e-16f);
                s = -1.0f * sqrtf(dist);
            }
            if (a.u_bias) s = s + a.u_bias[cur.u];
            if (a.t_bias) s = s + a.t_bias[cur.item];
            a.out[cur.p] = cur.ok ? s : __uint_as_float(0x7fc00000u);
        }
        if (!more) break;
        cur = nxt;
    }
}

// one wave per segment of at most CS_SHORT entries: place = number of (key, ~position) words above the entry's own
__global__ __launch_bounds__(64 * CS_WAVES) void candset_topk_short_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ptr,
                                                                           const int32_t* __restrict__ idx, const int32_t* __restrict__ rows,
                                                                           int64_t n_rows, int k, float* __restrict__ out_vals,
                                                                           int32_t* __restrict__ out_idx)
{
    __shared__ unsigned long long s_key[CS_WAVES][CS_SHORT];
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * CS_WAVES + w;
    if (r >= n_rows) return;
    const int64_t cr = rows ? (int64_t)rows[r] : r;
    const int64_t b = ptr[cr];
    const int64_t len = ptr[cr + 1] - b;
    if (len > CS_SHORT) return;                                         // (a long segment: the workgroup kernel's)
    const int n = (int)len;
    unsigned long long* keys = s_key[w];
    constexpr int PER = CS_SHORT / 64;
    unsigned long long mine[PER];
    float val[PER];
    int n_absent = 0;                                                   // entries with the sentinel's bits: the lowest keys, never placed
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int pos = q * 64 + lane;
        val[q] = pos < n ? scores[b + pos] : 0.f;
        mine[q] = cand_key(sel_key(val[q]), pos);
        if (pos < n) keys[pos] = mine[q];
        n_absent += (int)__popcll(__ballot(pos < n && (mine[q] >> 32) == 0ull));
    }
    wave_lds_sync();
    int place[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) place[q] = 0;
    for (int x = 0; x < n; ++x) {
        const unsigned long long other = keys[x];                       // (one address for the wave: a broadcast)
#pragma unroll
        for (int q = 0; q < PER; ++q) place[q] += other > mine[q] ? 1 : 0;
    }
    float* ov = out_vals + r * k;
    int32_t* oi = out_idx + r * k;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int pos = q * 64 + lane;
        if (pos < n && place[q] < k && (mine[q] >> 32) != 0ull) {
            ov[place[q]] = val[q];
            oi[place[q]] = idx[b + pos];
        }
    }
    for (int p = n - n_absent + lane; p < k; p += TREC_WAVE) {
        ov[p] = -INFINITY;
        oi[p] = -1;
    }
}

// one workgroup per listed row (long: int32 [n_long] rows of the call)
__global__ __launch_bounds__(SEL_THREADS) void candset_topk_long_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ptr,
                                                                        const int32_t* __restrict__ idx, const int32_t* __restrict__ rows,
                                                                        const int32_t* __restrict__ long_rows, int k,
                                                                        float* __restrict__ out_vals, int32_t* __restrict__ out_idx)
{
    const int64_t r = (int64_t)long_rows[blockIdx.x];
    const int64_t cr = rows ? (int64_t)rows[r] : r;
    const int64_t b = ptr[cr];
    select_row_topk(scores + b, ptr[cr + 1] - b, idx + b, k, out_vals + r * k, out_idx + r * k);
}

__global__ __launch_bounds__(256) void candset_rank_count_kernel(const int64_t* __restrict__ pair_ptr, const int32_t* __restrict__ t_idx,
                                                                 const float* __restrict__ t_score, const int64_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ score,
                                                                 int64_t n_users, int32_t* __restrict__ counts)
{
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    const int64_t p0 = pair_ptr[u], p1 = pair_ptr[u + 1], e0 = ptr[u], e1 = ptr[u + 1];
    for (int64_t p = p0 + lane_id(); p < p1; p += TREC_WAVE)
        counts[p] = listed_ahead<true>(idx, score, e0, e1, t_idx[p], t_score[p]);
}

}  // namespace

extern "C" int trec_candset_scores(const float* users_f32, const float* items_f32, int64_t ld, int32_t kdim, const int64_t* ptr,
                                   const int32_t* idx, const int32_t* rows, int64_t n_rows, int64_t nnz, int64_t n_items,
                                   const float* user_bias, const float* item_bias, int32_t mode, const float* user_sqnorm,
                                   const float* item_sqnorm, float* out, void* stream)
{
    TREC_REQUIRE(users_f32 && items_f32 && ptr, "trec_candset_scores: null pointer");
    TREC_REQUIRE(kdim >= 1 && kdim <= CS_KMAX && ld >= kdim, "trec_candset_scores: need 1 <= kdim <= 256 and kdim <= ld");
    TREC_REQUIRE((ld & 3) == 0 && (((uintptr_t)users_f32 | (uintptr_t)items_f32) & 15u) == 0,
                 "trec_candset_scores: operands must be 16-byte aligned with ld a multiple of 4 (score_prep's)");
    TREC_REQUIRE(mode == 0 || (user_sqnorm && item_sqnorm), "trec_candset_scores: euclidean mode needs squared norms");
    TREC_REQUIRE(n_rows >= 0 && nnz >= 0 && n_items >= 0 && n_items <= 0x7fffffffLL, "trec_candset_scores: bad sizes");
    if (n_rows == 0 || nnz == 0) return TREC_OK;
    TREC_REQUIRE(idx && out, "trec_candset_scores: null pointer");
    TREC_REQUIRE(n_items >= 1, "trec_candset_scores: candidates without items");
    const CandScoreArgs a = {users_f32, items_f32, ld, kdim, ptr, idx, rows, n_rows, n_items, user_bias, item_bias,
                             mode, user_sqnorm, item_sqnorm, out};
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int64_t max_waves = (int64_t)cus * 2 * CS_WAVES;             // two resident workgroups per CU
    if (rows) {
        const int64_t waves = n_rows < max_waves ? n_rows : max_waves;
        hipLaunchKernelGGL(candset_scores_kernel<false>, dim3((unsigned)ceil_div64(waves, CS_WAVES)), dim3(64 * CS_WAVES), 0,
                           (hipStream_t)stream, a, (int64_t)0);
    } else {
        // (the call's nnz = ptr[n_rows] - ptr[0]: the host knows it, the kernel reads both ends itself)
        const int64_t tiles = ceil_div64(nnz, 64);
        const int64_t waves = tiles < max_waves ? tiles : max_waves;
        const int64_t per_wave = ceil_div64(tiles, waves);
        hipLaunchKernelGGL(candset_scores_kernel<true>, dim3((unsigned)ceil_div64(ceil_div64(tiles, per_wave), CS_WAVES)),
                           dim3(64 * CS_WAVES), 0, (hipStream_t)stream, a, per_wave);
    }
    return trec_check_launch("trec_candset_scores");
}

extern "C" int trec_candset_topk(const float* scores, const int64_t* ptr, const int32_t* idx, const int32_t* rows, int64_t n_rows,
                                 int32_t k, const int32_t* long_rows, int64_t n_long, float* out_vals, int32_t* out_idx, void* stream)
{
    TREC_REQUIRE(ptr && out_vals && out_idx, "trec_candset_topk: null pointer");
    TREC_REQUIRE(k >= 1 && k <= SEL_THREADS, "trec_candset_topk: need 1 <= k <= 1024");
    TREC_REQUIRE(n_rows >= 0 && n_rows <= 0x7fffffffLL && n_long >= 0 && n_long <= n_rows, "trec_candset_topk: bad row counts");
    TREC_REQUIRE(n_long == 0 || (long_rows && scores && idx), "trec_candset_topk: null pointer");
    if (n_rows == 0) return TREC_OK;
    hipLaunchKernelGGL(candset_topk_short_kernel, dim3((unsigned)ceil_div64(n_rows, CS_WAVES)), dim3(64 * CS_WAVES), 0,
                       (hipStream_t)stream, scores, ptr, idx, rows, n_rows, k, out_vals, out_idx);
    int rc = trec_check_launch("trec_candset_topk (short)");
    if (rc != TREC_OK || n_long == 0) return rc;
    hipLaunchKernelGGL(candset_topk_long_kernel, dim3((unsigned)n_long), dim3(SEL_THREADS), 0, (hipStream_t)stream, scores, ptr, idx,
                       rows, long_rows, k, out_vals, out_idx);
    return trec_check_launch("trec_candset_topk (long)");
}

extern "C" int trec_candset_rank_count(const int64_t* pair_ptr, const int32_t* t_idx, const float* t_score, const int64_t* ptr,
                                       const int32_t* idx, const float* score, int64_t n_users, int32_t* counts, void* stream)
{
    TREC_REQUIRE(pair_ptr && ptr && counts, "trec_candset_rank_count: null pointer");
    if (n_users == 0) return TREC_OK;
    hipLaunchKernelGGL(candset_rank_count_kernel, dim3((unsigned)ceil_div64(n_users, 4)), dim3(256), 0, (hipStream_t)stream, pair_ptr,
                       t_idx, t_score, ptr, idx, score, n_users, counts);
    return trec_check_launch("trec_candset_rank_count");
}
