// tensorrec_amd/csrc/softmax_shared_body.hpp -- the body of shared_tile_kernel<KT, ROLE>(SharedParams p) and of
// shared_tile_hits_kernel<KT, ROLE>(SharedParams p, SharedHits h) (csrc/softmax_shared.hip), included once into each with SS_HITS
// 0 / 1: the text is the same, so the kernel without hits compiles to what it was before the second one existed.
// SS_HITS: a lane keeps a cursor into its row's list (column ranges with the users resident, users with the samples resident) and
// ORs what overlaps the streamed tile into one 32-bit mask; a masked entry is an invalid one -- -inf in SS_STATS, a literal 0.f
// (never computed: with M = -inf the product would be 0 * inf) in the gradient roles.
    constexpr int BN = 32;                  // streamed rows per tile = one 32 x 32 MFMA block
    constexpr int RB = KT * 4;              // bytes per LDS row
    constexpr int CH = RB / 16;             // 16-byte chunks per row
    constexpr int KS = KT / 2;              // MFMA k-steps of the score
    constexpr int CB = KT / 32;             // 32-column blocks of the product
    constexpr int TILE_BYTES = BN * RB;
    constexpr int NSLOT = BN * CH / 256;    // 16-byte staging slots per thread per tile
    constexpr int NSIDE = 3;                // per streamed row: bias, then c (samples) or M, tK (users)
    static_assert(NSLOT >= 1, "tile too small for 256 threads");
    extern __shared__ __attribute__((aligned(16))) char ssmem[];
    float* side = (float*)(ssmem + 2 * TILE_BYTES);        // [2][NSIDE][BN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int rblock = blockIdx.x % p.n_rblocks;
    const int slice = blockIdx.x / p.n_rblocks;
    const int64_t row = ((int64_t)rblock * 4 + wave) * 32 + l31;
    const bool row_ok = row < p.n_res;
    const int64_t src = row_ok ? row : 0;
    const int d = p.d;
    const int64_t t_begin = (int64_t)slice * p.slice_len;
    const int64_t t_end = (t_begin + p.slice_len < p.n_str) ? t_begin + p.slice_len : p.n_str;
    const int n_tiles = (int)((t_end - t_begin + BN - 1) / BN);
    const float inv_t = p.inv_t;

    float rff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int k = 2 * ks + half;
        rff[ks] = (k < d) ? p.R[src * d + k] : 0.f;
    }
    const float rb = p.r_bias ? p.r_bias[src] : 0.f;
    float rM = 0.f, rK = 0.f, rc = 0.f;
    if (ROLE == SS_DU) { rM = p.M[src]; rK = row_ok ? p.tK[src] : 0.f; }
    if (ROLE == SS_DV) rc = p.cs ? p.cs[src] : 0.f;
#if SS_HITS
    // ---- [hcur, hend) is what is left of my row's list, (nlo, nhi) its head: a column range, or in SS_DV a user (nlo)
    int64_t hcur = 0, hend = 0;
    int32_t nlo = 0, nhi = 0;
    if (row_ok) {
        if (ROLE == SS_DV) {
            const int32_t id = h.sorted_ids[row];
            if (id >= 0 && id < h.n_items) {
                hcur = h.indptr_tp[id];
                hend = h.indptr_tp[id + 1];
                int64_t lo = hcur, hi = hend;                 // the first user of my slice: lower bound of t_begin
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (h.users_tp[mid] < t_begin) lo = mid + 1;
                    else hi = mid;
                }
                hcur = lo;
            }
            if (hcur < hend) nlo = h.users_tp[hcur];
        } else {
            hcur = h.indptr[row];
            hend = hcur + h.hit_cnt[row];
            if (hcur < hend) { nlo = h.hit_rng[2 * hcur]; nhi = h.hit_rng[2 * hcur + 1]; }
        }
    }
#endif

    // ---- staging: slot q = i * 256 + tid -> (row, physical 16-byte chunk), XOR-swizzled as in score_rank.hip; chunks past d are zeros
    int slot_row[NSLOT], slot_src[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int q = i * 256 + tid;
        const int r = q / CH, pc = q % CH;
        const int sw = (CH >= 16) ? (r & 15) : ((CH == 8) ? ((r >> 1) & 7) : 0);
        slot_row[i] = r;
        slot_src[i] = (pc ^ sw) * 16;
    }
    u32x4 stage[NSLOT];
    float side_v[NSIDE] = {0.f, 0.f, 0.f};
    auto stage_issue = [&](int tile) {
        const int64_t row0 = t_begin + (int64_t)tile * BN;
        if (tid < BN) {
            int64_t g = row0 + tid;
            if (g >= p.n_str) g = p.n_str - 1;              // clamped rows are masked below
            side_v[0] = p.t_bias ? p.t_bias[g] : 0.f;
            if (ROLE == SS_DV) { side_v[1] = p.M[g]; side_v[2] = p.tK[g]; }
            else side_v[1] = p.cs ? p.cs[g] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            int64_t g = row0 + slot_row[i];
            if (g >= p.n_str) g = p.n_str - 1;
            const u32x4 zero = {0u, 0u, 0u, 0u};
            stage[i] = (slot_src[i] < d * 4) ? *(const u32x4*)((const char*)p.T + g * (int64_t)d * 4 + slot_src[i]) : zero;
        }
    };
    auto stage_commit = [&](int buf) {
        if (tid < BN) {
#pragma unroll
            for (int j = 0; j < NSIDE; ++j) side[(buf * NSIDE + j) * BN + tid] = side_v[j];
        }
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) *(u32x4*)(ssmem + buf * TILE_BYTES + (i * 256 + tid) * 16) = stage[i];
    };

    f32x16 prod[ROLE == SS_STATS ? 1 : CB];
    if (ROLE != SS_STATS) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) prod[cb][r] = 0.f;
    }
    float run_m = -INFINITY, run_z = 0.f;    // SS_STATS
    float psum = 0.f;                        // SS_DV: this lane's share of d b_s

    stage_issue(0);
    stage_commit(0);
    __syncthreads();
    for (int t = 0; t < n_tiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < n_tiles) stage_issue(t + 1);
        const char* tile = ssmem + buf * TILE_BYTES;
        const char* rowp = tile + l31 * RB;
        const int sw = (CH >= 16) ? (l31 & 15) : ((CH == 8) ? ((l31 >> 1) & 7) : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (2 * ks < d) {                                                  // (uniform: the padded k-steps add exact zeros)
                const int k = 2 * ks + half;
                const float tf = *(const float*)(rowp + (((k >> 2) ^ sw) * 16) + (k & 3) * 4);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tf, rff[ks], acc, 0, 0, 0);
            }
        }
        const float* sd = side + buf * NSIDE * BN;
        const int64_t loc0 = t_begin + (int64_t)t * BN;
        const int rows_left = (int)((p.n_str - loc0 < BN) ? (p.n_str - loc0) : BN);
#if SS_HITS
        // ---- bit c of the mask = streamed row loc0 + c is masked for my resident row (a padded resident row masks them all)
        uint32_t hm = 0u;
        {
            uint32_t hmask = row_ok ? 0u : ~0u;
            const int64_t tile_end = loc0 + BN;
            if (ROLE == SS_DV) {
                while (hcur < hend && (int64_t)nlo < tile_end) {
                    hmask |= 1u << (int)((int64_t)nlo - loc0);
                    ++hcur;
                    if (hcur < hend) nlo = h.users_tp[hcur];
                }
            } else {
                while (hcur < hend && (int64_t)nlo < tile_end) {
                    const int a = ((int64_t)nlo > loc0) ? (int)((int64_t)nlo - loc0) : 0;
                    const int b = ((int64_t)nhi < tile_end) ? (int)((int64_t)nhi - loc0) : BN;
                    hmask |= (b - a >= 32) ? ~0u : (((1u << (b - a)) - 1u) << a);
                    if ((int64_t)nhi > tile_end) break;       // (it goes on in the next tile)
                    ++hcur;
                    if (hcur < hend) { nlo = h.hit_rng[2 * hcur]; nhi = h.hit_rng[2 * hcur + 1]; }
                }
            }
            hm = hmask >> (4 * half);
        }
#endif
        // ---- w of my resident row against the streamed rows ss_cd_row(r, half): ((dot + b_u) + b_s) t + c_s in every role
        float tile_m = -INFINITY;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const f32x4 tb4 = *(const f32x4*)(sd + 8 * q4 + 4 * half);
            const f32x4 s14 = *(const f32x4*)(sd + BN + 8 * q4 + 4 * half);
            f32x4 s24 = {0.f, 0.f, 0.f, 0.f};
            if (ROLE == SS_DV) s24 = *(const f32x4*)(sd + 2 * BN + 8 * q4 + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#if SS_HITS
                const bool valid = 8 * q4 + 4 * half + e < rows_left && !((hm >> (8 * q4 + e)) & 1u);
#else
                const bool valid = 8 * q4 + 4 * half + e < rows_left;
#endif
                float v = acc[4 * q4 + e];
                if (ROLE == SS_DV) {
                    v = (v + tb4[e]) + rb;
                    v = fmaf(v, inv_t, rc);
                    v = valid ? s24[e] * expf(v - s14[e]) : 0.f;
                    psum += v;
                } else {
                    v = (v + rb) + tb4[e];
                    v = fmaf(v, inv_t, s14[e]);
                    if (ROLE == SS_DU) v = valid ? rK * expf(v - rM) : 0.f;
                    else {
                        v = valid ? v : -INFINITY;
                        tile_m = fmaxf(tile_m, v);
                    }
                }
                acc[4 * q4 + e] = v;
            }
        }
        if (ROLE == SS_STATS) {
            if (tile_m > -INFINITY) {                        // (a half-wave whose columns all lie past S adds nothing)
                if (tile_m > run_m) {
                    run_z = run_z * expf(run_m - tile_m);    // (first tile: 0 * exp(-inf) = 0)
                    run_m = tile_m;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) run_z += expf(acc[r] - run_m);
            }
        } else {
            // ---- product: C[column cb * 32 + i][resident j] += sum_r T[row ss_cd_row(r, k)][column] P[k][j], k = half
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                if (cb * 32 < d) {
                    const int k = cb * 32 + l31;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rr = ss_cd_row(r, half);
                        const int swr = (CH >= 16) ? (rr & 15) : ((CH == 8) ? ((rr >> 1) & 7) : 0);
                        const float a = *(const float*)(tile + rr * RB + (((k >> 2) ^ swr) * 16) + (k & 3) * 4);
                        prod[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, acc[r], prod[cb], 0, 0, 0);
                    }
                }
            }
        }
        if (t + 1 < n_tiles) stage_commit(buf ^ 1);
        __syncthreads();
    }

    if (ROLE == SS_STATS) {
        const float om = __shfl_xor(run_m, 32, 64), oz = __shfl_xor(run_z, 32, 64);
        // half 0 first, then half 1, in both lanes: M = max, Z = z0 exp(m0 - M) + z1 exp(m1 - M); an empty half adds an exact 0
        const float m0 = half ? om : run_m, z0 = half ? oz : run_z;
        const float m1 = half ? run_m : om, z1 = half ? run_z : oz;
        const float Mx = fmaxf(m0, m1);
        const float a0 = (m0 > -INFINITY) ? z0 * expf(m0 - Mx) : 0.f;
        const float a1 = (m1 > -INFINITY) ? z1 * expf(m1 - Mx) : 0.f;
        if (row_ok && half == 0) { p.out_M[row] = Mx; p.out_Z[row] = a0 + a1; }
        return;
    }
    // ---- the product of my resident row: prod[cb][4 q + e] is column cb * 32 + 8 q + 4 half + e
    float* orow = p.out + ((ROLE == SS_DV ? (int64_t)slice * p.n_res : 0) + src) * d;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int c0 = cb * 32 + 8 * q4 + 4 * half;
            if (row_ok && c0 < d) {
                f32x4 o = {prod[cb][4 * q4], prod[cb][4 * q4 + 1], prod[cb][4 * q4 + 2], prod[cb][4 * q4 + 3]};
                if (ROLE == SS_DU) {
                    const f32x4 have = *(const f32x4*)(orow + c0);
                    o = have + o;
                }
                *(f32x4*)(orow + c0) = o;
            }
        }
    }
    if (ROLE == SS_DV) {
        const float other = __shfl_xor(psum, 32, 64);
        if (row_ok && half == 0 && p.out_sum) p.out_sum[(int64_t)slice * p.n_res + row] = psum + other;
    }
