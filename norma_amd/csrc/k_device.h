// k_device.h -- small device functions that more than one kernel file relies on bit for bit (gfx950): workgroup reductions,
// the candidate comparison, the softmax pair merge, the logit rules, ordered float keys, swap23.  Device code only.
#pragma once
#include "nh_kernels.h"

// ---- workgroup reductions -------------------------------------------------------------------------------------------------
// The order is the contract (tests/test_gpu_token_ref.py, tests/test_gpu_beam.py): the xor tree with offsets 32 .. 1 inside
// a wave, then the waves' slots from 0 upward.  WAVES: the workgroup's waves where the kernel fixes them (beam_select_kernel),
// 0: blockDim.x / 64 (k_token.hip).  slots: that many floats of LDS, free again at the next barrier of the workgroup.  Every
// thread gets the result.
template <int WAVES = 0>
__device__ __forceinline__ float block_max(float v, float *slots) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    const int waves = WAVES ? WAVES : (int)(blockDim.x >> 6);
    float r = slots[0];
    for (int i = 1; i < waves; i++) r = fmaxf(r, slots[i]);
    return r;
}
template <int WAVES = 0>
__device__ __forceinline__ float block_sum(float v, float *slots) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    const int waves = WAVES ? WAVES : (int)(blockDim.x >> 6);
    float r = slots[0];
    for (int i = 1; i < waves; i++) r += slots[i];
    return r;
}
// larger value, then larger index (the reference's last-maximum rule); i < 0: nothing
__device__ __forceinline__ void better(float &v, int &i, float v2, int i2) {
    if (i2 >= 0 && (i < 0 || v2 > v || (v2 == v && i2 > i))) { v = v2; i = i2; }
}

// ---- softmax pair merge ---------------------------------------------------------------------------------------------------
// (m, s) <- the (maximum, sum of exp(l - maximum)) pair of the union of two column sets; f1, f2: what the merge scaled the two
// sums by, for whatever else was summed against the same maxima
__device__ __forceinline__ void merge_pair(float &m, float &s, float m2, float s2, float &f1, float &f2) {
    const float mn = fmaxf(m, m2);
    f1 = (m == -INFINITY) ? 0.f : __expf(m - mn); f2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
    s = s * f1 + s2 * f2; m = mn;
}
__device__ __forceinline__ void merge_pair(float &m, float &s, float m2, float s2) {
    float f1, f2;
    merge_pair(m, s, m2, s2, f1, f2);
}

// ---- the logit rules of Model::decode (src/models/whisper/model.rs:212-277, :331-338) --------------------------------------
// RULE_BY_MASS is no mask chain: the last token is text, and RULE_NON_TS or RULE_PAST applies once the timestamp mass and
// the best text probability are known (sum_ts >= max_text, model.rs:263-270)
enum { RULE_FIRST = 0, RULE_SUP_TS = 1, RULE_NON_TS = 2, RULE_PAST = 3, RULE_BY_MASS = 4 };

// which rule applies, as far as the row's own state says: n tokens so far, l1 = tokens[n - 1], l2 = tokens[n - 2]
__device__ __forceinline__ int rule_from_state(int have_last, int n, int l1, int l2, const RuleTokens &tk) {
    if (!have_last) return RULE_FIRST;
    if (l1 > tk.no_timestamps) return (n >= 2 && l2 >= tk.eot) ? RULE_SUP_TS : RULE_NON_TS;
    return RULE_BY_MASS;
}
// does `rule` mask token i?  sup: the token's suppress flag (RULE_FIRST does not look at it)
__device__ __forceinline__ bool rule_masks(int rule, int i, bool sup, const RuleTokens &tk, int last_ts) {
    if (rule == RULE_FIRST) return i < tk.zero_sec || i > tk.one_sec;                 // model.rs:336-337
    if (rule == RULE_SUP_TS) return sup || i > tk.no_timestamps;                      // :256-259
    if (rule == RULE_NON_TS) return sup || i <= tk.no_timestamps || i <= last_ts;     // :216-223
    return sup || (i > tk.no_timestamps && i <= last_ts);                             // :225-243
}

// ---- ordered float keys ---------------------------------------------------------------------------------------------------
// u32 keys ascending in the float's order: negative values with all bits flipped, the others with the sign bit set.  Integer
// work only: the same under -ffp-contract=off (k_mel.hip, k_vad.hip) as anywhere else.
__device__ __forceinline__ unsigned f32_ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_ordered(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// ---- swap23 ---------------------------------------------------------------------------------------------------------------
// x with bits 2 and 3 exchanged: the key order of the attention kernels' LDS tiles (k_attn_enc.hip, k_xabs.hip)
__device__ __forceinline__ int swap23(int x) { return (x & ~12) | ((x & 4) << 1) | ((x & 8) >> 1); }
