// tensorrec_amd/csrc/tiled_pass_parts.hpp -- the two sweeps over a user's S + n_u item rows that the tiled one-pass steps share, as
// TEXT (the idiom of csrc/user_fused_body.hpp): wmrb_tiled_user (csrc/wmrb_tiled_body.hpp: WMRB, also inside csrc/step_coop.hip) and
// softmax_user_tiled_kernel (csrc/softmax_tiled.hip) include a part where the code stood, so both compile the same tokens and the
// WMRB kernels come out instruction for instruction as they did with the code inline.  No include guard: a file includes it once
// per part, with TILED_PASS_PART set.  (The line numbers that tests/step_reference.py quotes for wmrb_tiled_body.hpp -- :145-147 the
// score, :278-306 pass 2 and the sums -- are those the text had there: part 1 was lines 71-154 of that file, part 2 lines 244-308.)
//
// The including function provides: template parameters ITERS, RB, MODE, LPR; constexpr int NSG = 256 / LPR; the LDS arrays l_y, l_cf
// [max_rows4], l_part [NSG][d], l_red [8]; tid, lane, wave, sub, sg; b, e, n_pos, R = S + n_pos; U, V, ub, ib, xi, samp, S, d, u;
// the TiledOut o.
//   part 1   the n_pos == 0 exit; the user's row into registers (x, bu); pass 1: scores into l_y (Euclidean: the squared distance
//            into l_cf), pred_serial; a barrier.  The loss phase of the includer follows: it leaves the value of every row in l_cf
//            and each thread's share of the sums in raw_sum (the coefficients g) and val_sum (the values), ends with a barrier.
//   part 2   pass 2: dU from the values in l_cf; d b_u and val_rowsum from raw_sum / val_sum; the last barrier.

#if TILED_PASS_PART == 1
    if (n_pos == 0) {
        // no interactions: no loss terms, every coefficient is 0
        for (int s = tid; s < S; s += 256) {
            if (o.val_samples) o.val_samples[u * S + s] = 0.f;
            if (o.raw_samples) o.raw_samples[u * S + s] = 0.f;
        }
        if (o.dU) for (int c = tid; c < d; c += 256) o.dU[u * d + c] = 0.f;
        if (o.val_rowsum && tid == 0) o.val_rowsum[u] = 0.f;
        if (o.dub && tid == 0) o.dub[u] = 0.f;
        return;                                              // (uniform over the workgroup; no LDS was touched)
    }

    f32x4 x[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * LPR + sub) * 4;
        const f32x4 v = *(const f32x4*)(U + u * d + (c < d ? c : 0));
        x[it] = (c < d) ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const float bu = ub ? ub[u] : 0.f;

    // ---- pass 1: scores of the rows j = j0 + sg + 8 r.  Every load is unconditional, from a clamped (valid) address, selected
    // afterwards (`cond ? load : 0` becomes an exec-masked block behind s_waitcnt vmcnt(0)) ----
    for (int j0 = 0; j0 < R; j0 += NSG * RB) {
        int32_t item[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int j = j0 + sg + NSG * r;
            const int q = j - S;
            const int32_t is = samp[j < S ? j : S - 1];
            const int32_t iq = xi[b + (q < 0 ? 0 : (q < n_pos ? q : n_pos - 1))];
            item[r] = (j < S) ? is : iq;
        }
        f32x4 y[RB][ITERS];
        float bi[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int c = (it * LPR + sub) * 4;
                y[r][it] = *(const f32x4*)(V + (int64_t)item[r] * d + (c < d ? c : 0));
            }
            bi[r] = ib ? ib[item[r]] : 0.f;                   // (uniform branch; one address per subgroup)
        }
        float acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float a = 0.f;
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const bool in = (it * LPR + sub) * 4 < d;      // (columns past d: both sides count as zero)
                if (MODE == 0) {
                    const f32x4 w = in ? y[r][it] : (f32x4){0.f, 0.f, 0.f, 0.f};
                    a = fmaf(x[it].x, w.x, a); a = fmaf(x[it].y, w.y, a); a = fmaf(x[it].z, w.z, a); a = fmaf(x[it].w, w.w, a);
                } else {
                    const f32x4 w = in ? y[r][it] : x[it];
                    const float d0 = x[it].x - w.x, d1 = x[it].y - w.y, d2 = x[it].z - w.z, d3 = x[it].w - w.w;
                    a = fmaf(d0, d0, a); a = fmaf(d1, d1, a); a = fmaf(d2, d2, a); a = fmaf(d3, d3, a);
                }
            }
            acc[r] = a;
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float t = acc[r];
            t = dpp_add(t, 8); t = dpp_add(t, 4); t = dpp_add(t, 2); t = dpp_add(t, 1);     // every lane of a 16-lane row: the row's sum
            acc[r] = (LPR == 32) ? dpp_add(t, 0) : t;                                        // 32 lanes: row 0's sum into row 1
        }
        if (sub == LPR - 1) {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int j = j0 + sg + NSG * r;
                if (j < R) {
                    float s = acc[r];
                    if (MODE == 1) { l_cf[j] = s; s = -1.0f * sqrtf(fmaxf(s, EUCLID_EPS)); }
                    if (ub) s = s + bu;
                    if (ib) s = s + bi[r];
                    l_y[j] = s;
                    if (j >= S) o.pred_serial[b + (j - S)] = s;
                }
            }
        }
    }
    __syncthreads();
#endif

#if TILED_PASS_PART == 2
    // ---- pass 2: dU_u = sum_j val_j * row_j (dot) / sum_j val_j * (U_u - row_j) (euclidean); skipped when the caller takes dU
    // from the dense matrix (G . V on fp32 MFMA: the second sweep over the rows is 45 ms of configs[4]'s step, the GEMM 19) ----
    if (o.dU) {
        f32x4 part[ITERS];
#pragma unroll
        for (int it = 0; it < ITERS; ++it) part[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < R; j0 += NSG * RB) {
            int32_t item[RB];
            float cf[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int j = j0 + sg + NSG * r;
                const int q = j - S;
                const int32_t is = samp[j < S ? j : S - 1];
                const int32_t iq = xi[b + (q < 0 ? 0 : (q < n_pos ? q : n_pos - 1))];
                item[r] = (j < S) ? is : iq;
                const float v = l_cf[j < R ? j : 0];
                cf[r] = (j < R) ? v : 0.f;
            }
            f32x4 y[RB][ITERS];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
#pragma unroll
                for (int it = 0; it < ITERS; ++it) {
                    const int c = (it * LPR + sub) * 4;
                    y[r][it] = *(const f32x4*)(V + (int64_t)item[r] * d + (c < d ? c : 0));
                }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
#pragma unroll
                for (int it = 0; it < ITERS; ++it) {
                    f32x4 w = y[r][it];
                    if (MODE == 1) { w.x = x[it].x - w.x; w.y = x[it].y - w.y; w.z = x[it].z - w.z; w.w = x[it].w - w.w; }
                    part[it].x = fmaf(cf[r], w.x, part[it].x); part[it].y = fmaf(cf[r], w.y, part[it].y);
                    part[it].z = fmaf(cf[r], w.z, part[it].z); part[it].w = fmaf(cf[r], w.w, part[it].w);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * LPR + sub) * 4;
            if (c < d) *(f32x4*)(l_part + sg * d + c) = part[it];
        }
    }
    if (o.dub) {
        for (int off = 32; off > 0; off >>= 1) raw_sum += __shfl_xor(raw_sum, off, 64);
        if (lane == 0) l_red[wave] = raw_sum;
    }
    if (o.val_rowsum) {
        for (int off = 32; off > 0; off >>= 1) val_sum += __shfl_xor(val_sum, off, 64);
        if (lane == 0) l_red[4 + wave] = val_sum;
    }
    __syncthreads();
    if (o.dU) {
        for (int c = tid; c < d; c += 256) {
            float acc = l_part[c];
#pragma unroll
            for (int g8 = 1; g8 < NSG; ++g8) acc += l_part[g8 * d + c];
            o.dU[u * d + c] = acc;
        }
    }
    if (o.dub && tid == 0) o.dub[u] = (l_red[0] + l_red[1]) + (l_red[2] + l_red[3]);
    if (o.val_rowsum && tid == 0) o.val_rowsum[u] = (l_red[4] + l_red[5]) + (l_red[6] + l_red[7]);
    __syncthreads();
#endif
