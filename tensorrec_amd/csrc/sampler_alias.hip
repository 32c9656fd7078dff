// tensorrec_amd/csrc/sampler_alias.hip -- K7a: popularity-weighted negative sampling on the device (Walker's alias method).
//
// No counterpart in the reference (util.sample_items is uniform).  The table -- thr uint32 [n_items], alias int32 [n_items] -- is built
// once on the host (tensorrec.py: PopularitySampler); this kernel only draws from it, WITH replacement, one thread per sample:
//     block  = Philox4x32-10(counter (user_lo, s >> 1, step, ALIAS_STREAM + user_hi), key (seed_lo, seed_hi))
//     (w0, w1) = s even ? (block.x, block.y) : (block.z, block.w)          -- one block serves two samples
//     j      = (w0 * n_items) >> 32                                        -- the column, uniform over [0, n_items)
//     out    = w1 < thr[j] ? j : alias[j]                                  -- STRICTLY below: column j keeps thr[j] of its 2^32 words
// so that a threshold of 0 never accepts (an item of weight 0 is never drawn) and a column of probability 1 carries 2^32 - 1 with
// alias[j] = j.  The probabilities the table implements are exact integers over n_items * 2^32:
//     q_i * n_items * 2^32 = thr[i] + sum_{j : alias[j] = i} (2^32 - thr[j]).
// The counter layout is sample_items_kernel's replace branch (sampler.hip) with two words per sample instead of one and a stream
// constant K7 does not use (K7: 0, 1 for the keys, 2 + user_hi for the replace branch), so both samplers are independent under one
// seed.  Row r is the stream of the GLOBAL user user_base + r, as in K7.  Checked bit for bit against an integer restatement
// (tests/alias_sampler_reference.py).
// One thread per sample, so the two threads of a pair both run the block's ten rounds: a thread per PAIR (one block, two gathers, two
// stores 4 bytes apart) was measured and is slower, 1.76 ms against 1.20 ms for 1M users x 100 samples (docs/sampled_losses.md).
#include "common.hpp"

#include "sampler_common.hpp"

#define ALIAS_STREAM 0x414C4953u

__global__ __launch_bounds__(256) void sample_items_alias_kernel(int64_t n_users, int64_t user_base, int32_t n_items, int32_t n_sampled,
                                                                const uint32_t* __restrict__ thr, const int32_t* __restrict__ alias,
                                                                uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                                int32_t* __restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_users * n_sampled) return;
    const int64_t ul = idx / n_sampled;
    const uint32_t s = (uint32_t)(idx - ul * n_sampled);
    const int64_t u = ul + user_base;
    const u4 r = philox4x32_10(u4{(uint32_t)u, s >> 1, step, ALIAS_STREAM + (uint32_t)(u >> 32)}, seed_lo, seed_hi);
    const uint32_t w0 = (s & 1) ? r.z : r.x, w1 = (s & 1) ? r.w : r.y;
    const uint32_t j = (uint32_t)(((uint64_t)w0 * (uint64_t)(uint32_t)n_items) >> 32);      // < n_items: both gathers are in bounds
    out[idx] = w1 < thr[j] ? (int32_t)j : alias[j];
}

extern "C" int trec_sample_items_alias(int64_t n_users, int64_t user_base, int32_t n_items, int32_t n_sampled, const uint32_t* thr,
                                       const int32_t* alias, uint64_t seed, uint32_t step, int32_t* out, void* stream)
{
    TREC_REQUIRE(thr && alias && out, "trec_sample_items_alias: null pointer");
    TREC_REQUIRE(n_items >= 1 && n_sampled >= 1, "trec_sample_items_alias: n_items and n_sampled must be >= 1");
    TREC_REQUIRE(n_users >= 0, "trec_sample_items_alias: n_users must be >= 0");
    if (n_users == 0) return TREC_OK;
    const int64_t total = n_users * (int64_t)n_sampled;
    hipLaunchKernelGGL(sample_items_alias_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream, n_users,
                       user_base, n_items, n_sampled, thr, alias, (uint32_t)seed, (uint32_t)(seed >> 32), step, out);
    return trec_check_launch("trec_sample_items_alias");
}
