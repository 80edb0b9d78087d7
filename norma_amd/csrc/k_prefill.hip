// k_prefill.hip -- attention of the one-pass teacher-forced decoder forward (nh_prefill.hip): T query positions of a clip at
// once against that clip's keys, where a decode step (k_dec_attn.hip) has one query row per (clip, head).
//
//   prefill_attn_kernel<true>    causal self-attention over the clip's own positions <= i; the workgroup that holds the
//                                clip's last query tile also writes K and V into the head-major self cache [b][h][C][64] at
//                                slots 0 .. T-1, so that the decode steps that follow find them there
//   prefill_attn_kernel<false>   cross-attention of the T queries over the head-major cross K/V [b][h][S][64]
//
// One workgroup per (256-query tile, head, clip), one wave per 16 queries (so up to 16 waves; a prefix of a decode is at most
// max_target_positions / 2 - 1 = 223 positions: one workgroup, and the K/V of a (clip, head) pass through LDS once).  Keys
// come in blocks of 64: the block's K is staged as [key][64] (16-byte chunks, chunk' = chunk ^ ((key >> 1) & 7): conflict-free
// ds_read_b128), its V transposed as [dim][key].  Per wave and block, with v_mfma_f32_16x16x32_f16:
//   S^T[key][query] = K . Q^T     A = K rows from LDS, B = the wave's Q fragment (registers, loaded once from global memory)
//   s = S^T / 8 in f32, masked (key > query under the causal form, key >= the key count) to -inf
//   online softmax in f32 per query: m, and l summed in f32 from the weights AS ROUNDED TO FP16 for the product below: numerator
//                                 and denominator hold the same weights, so O / l is a convex combination of the V rows (summed
//                                 from the unrounded weights, l would miss what the rounding does to all of them alike:
//                                 up to 2^-11 |o| more, and not an average of V any more)
//   O^T[dim][query] += V^T . P^T  A = V^T rows from LDS, B = P^T: the score accumulators themselves, rounded to fp16 -- an
//                                 accumulator has its query on the lane and its keys in the registers, which is the B layout
//                                 up to the order of the 32 keys inside a k-step, and the V^T fragment is read in that order
// and at the end O / l in f32, rounded once to fp16.  Everything a query's result depends on -- its clip's rows, the order
// of the key blocks, the reduction trees -- is fixed by its position alone: bit-identical whatever the batch around the clip.
// The ragged form (PrefillAttn::clips; a decode pool's prefixes, nh_pool_prefix): clip z of the launch has its own length, its
// rows packed at its own offset, and its caches in its own context row, all read from a table; grid x covers the longest clip
// and a workgroup past its clip's last query leaves before its first barrier.  The uniform form is the same kernel with no
// table: length T, offset z * T, row z.  Nothing above looks at the grid or at the block size except the staging loops, which
// only move data: a clip's bits are the same in either form, whatever is packed around it.
// The kernel feeds MFMAs from LDS, so it takes its CU's whole LDS (nh_kernels.h, "kernels that do not share their CU's LDS").
#include "nh_kernels.h"

#define PF_KB 64                 // keys per block
#define PF_QW 16                 // queries per wave
#define PF_MAX_WAVES 16
#define PF_VT_LD 72              // halfs per V^T row: 64 keys + 8 of padding (144 B rows: 8-byte reads of 16 rows spread over the banks)
#define PF_LDS_K (PF_KB * NH_DH * 2)
#define PF_LDS_BYTES (PF_LDS_K + NH_DH * PF_VT_LD * 2)

struct PrefillAttn {
    const half_t *q; long ldq;                  // query of (clip b, position i, head h) at q + (off_b + i) * ldq + 64 h, off_b = b * T
    const half_t *k, *v;                        // key j of (b, h): causal -- the packed rows, k + (off_b + j) * kv_key + h * kv_head;
    long kv_clip, kv_head, kv_key;              //   cross -- k + row_b * kv_clip + h * kv_head + j * kv_key (64 halfs), row_b = b
    half_t *out; long ldo;                      // like q
    int T, nk;                                  // queries per clip; keys per clip (the causal form: T)
    half_t *ck, *cv; int C;                     // the causal form: self cache [row_b][h][C][64], slots 0 .. T-1 are written
    const PfClip *clips;                        // ragged: (row_b, T_b, off_b) of clip b = blockIdx.z; nullptr: uniform, as above
};

template <bool CAUSAL>
__global__ __launch_bounds__(64 * PF_MAX_WAVES) void prefill_attn_kernel(PrefillAttn p) {
    extern __shared__ __attribute__((aligned(16))) char pf_lds[];
    char *lk = pf_lds;
    half_t *lvt = reinterpret_cast<half_t *>(pf_lds + PF_LDS_K);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
    const int q0 = blockIdx.x * (PF_QW * PF_MAX_WAVES);           // first query of the workgroup
    int T = p.T, crow = b;                                        // the clip's queries, its context row (caches),
    long off = (long)b * p.T;                                     // and the packed row of its position 0
    if (p.clips) {
        const PfClip c = p.clips[b];
        T = c.T; crow = c.row; off = c.off;
        if (q0 >= T) return;                                      // the grid covers the longest clip: nothing here for a shorter one
    }
    const int nwaves = blockDim.x >> 6;
    const int wq0 = q0 + wave * PF_QW;                            // first query of the wave
    const bool active = wq0 < T;                                  // waves past the clip's last query only help staging
    // keys the workgroup needs: causal -- up to its last query; cross -- all
    const int wg_last_q = min(T, q0 + nwaves * PF_QW) - 1;
    const int nkeys = CAUSAL ? wg_last_q + 1 : p.nk;
    const bool writer = CAUSAL && q0 + PF_QW * PF_MAX_WAVES >= T; // the clip's own last tile stages every key of the clip: it fills the self cache
    const int myq = min(wq0 + fr, T - 1);                         // rows past the clip's last are clamped (computed, never stored)
    const half_t *qp = p.q + (off + myq) * p.ldq + h * NH_DH + 8 * fq;
    const half8 qf0 = *reinterpret_cast<const half8 *>(qp), qf1 = *reinterpret_cast<const half8 *>(qp + 32);
    const long kv0 = (CAUSAL ? off * p.kv_key : (long)crow * p.kv_clip) + (long)h * p.kv_head;
    const half_t *kb = p.k + kv0, *vb = p.v + kv0;
    const float ninf = -INFINITY;
    float m = ninf, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < nkeys; k0 += PF_KB) {
        __syncthreads();   // every wave has read the block before
        for (int s = tid; s < PF_KB * 8; s += blockDim.x) {
            const int key = s >> 3, c = s & 7;
            const int kg = k0 + key, kc = min(kg, nkeys - 1);     // never read past the last key: clamped, and masked below
            const half8 kk = *reinterpret_cast<const half8 *>(kb + (long)kc * p.kv_key + 8 * c);
            const half8 vv = *reinterpret_cast<const half8 *>(vb + (long)kc * p.kv_key + 8 * c);
            *reinterpret_cast<half8 *>(lk + key * 128 + ((c ^ ((key >> 1) & 7)) << 4)) = kk;
#pragma unroll
            for (int j = 0; j < 8; j++) lvt[(8 * c + j) * PF_VT_LD + key] = vv[j];
            if (writer && kg < T) {
                const long dst = (((long)crow * H + h) * p.C + kg) * NH_DH + 8 * c;
                *reinterpret_cast<half8 *>(p.ck + dst) = kk;
                *reinterpret_cast<half8 *>(p.cv + dst) = vv;
            }
        }
        __syncthreads();
        if (!active || (CAUSAL && k0 > wq0 + PF_QW - 1)) continue;   // wave-uniform: nothing of this block is visible to the wave
        f32x4 sc[4];
        float bm = ninf;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = 16 * t + fr;
            const char *kr = lk + row * 128;
            const int sw = (row >> 1) & 7;
            const half8 a0 = *reinterpret_cast<const half8 *>(kr + ((fq ^ sw) << 4));
            const half8 a1 = *reinterpret_cast<const half8 *>(kr + (((4 + fq) ^ sw) << 4));
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, qf0, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, qf1, c, 0, 0, 0);
            // c[r]: key k0 + 16 t + 4 fq + r, query wq0 + fr
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = k0 + 16 * t + 4 * fq + r;
                const bool vis = key < nkeys && (!CAUSAL || key <= wq0 + fr);
                const float s = vis ? c[r] * 0.125f : ninf;
                sc[t][r] = s;
                bm = fmaxf(bm, s);
            }
        }
        bm = fmaxf(bm, __shfl_xor(bm, 16));
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);   // finite from the first block on: key 0 is visible to every query
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * 1.4426950408889634f);   // first block: exp2(-inf) = 0
        float ps = 0.f;
        half8 pf[2];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const half_t e = (half_t)__builtin_amdgcn_exp2f((sc[t][r] - mn) * 1.4426950408889634f);   // masked keys: 0
                ps += (float)e;
                pf[t >> 1][4 * (t & 1) + r] = e;
            }
        }
        l = l * alpha + ps;   // per lane: the four lanes of a query meet after the last block
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 4; dt++) {
            o[dt] *= alpha;
            const half_t *vr = lvt + (16 * dt + fr) * PF_VT_LD + 4 * fq;
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                // k-slot 8 fq + j of the k-step holds key 32 ks + 4 fq + j (j < 4) and 32 ks + 16 + 4 fq + j - 4 (j >= 4)
                const half4 v0 = *reinterpret_cast<const half4 *>(vr + 32 * ks), v1 = *reinterpret_cast<const half4 *>(vr + 32 * ks + 16);
                const half8 a = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf[ks], o[dt], 0, 0, 0);
            }
        }
    }
    if (!active) return;
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const int qrow = wq0 + fr;
    if (qrow >= T) return;
    const float inv = 1.0f / l;
    half_t *op = p.out + (off + qrow) * p.ldo + h * NH_DH + 4 * fq;
#pragma unroll
    for (int dt = 0; dt < 4; dt++) {
        // o[dt][r]: dim 16 dt + 4 fq + r of query qrow
        const half4 hv = {(half_t)(o[dt][0] * inv), (half_t)(o[dt][1] * inv), (half_t)(o[dt][2] * inv), (half_t)(o[dt][3] * inv)};
        *reinterpret_cast<half4 *>(op + 16 * dt) = hv;
    }
}

static bool prefill_attn_launch(bool causal, const PrefillAttn &p, int B, int H, hipStream_t st) {
    if (B < 1 || H < 1 || p.T < 1 || p.nk < 1 || (causal && (p.nk != p.T || p.T > p.C))) return false;
    const int per = PF_QW * PF_MAX_WAVES;
    const int tiles = (p.T + per - 1) / per;
    // the workgroups of a clip all have the waves of a full tile but the last, which has what its queries need
    const int waves = tiles > 1 ? PF_MAX_WAVES : (p.T + PF_QW - 1) / PF_QW;
    const dim3 grid(tiles, H, B), block(64 * waves);
    if (causal) launch_lds_exclusive<prefill_attn_kernel<true>>(grid, block, PF_LDS_BYTES, st, p);
    else launch_lds_exclusive<prefill_attn_kernel<false>>(grid, block, PF_LDS_BYTES, st, p);
    return true;
}

bool launch_prefill_self_attention(const half_t *q, const half_t *k, const half_t *v, long ld, half_t *out, long ldo, half_t *ck,
                                   half_t *cv, int B, int T, int H, int C, hipStream_t st, const PfClip *clips) {
    PrefillAttn p{};
    p.q = q; p.ldq = ld; p.k = k; p.v = v; p.kv_clip = (long)T * ld; p.kv_head = NH_DH; p.kv_key = ld;
    p.out = out; p.ldo = ldo; p.T = T; p.nk = T; p.ck = ck; p.cv = cv; p.C = C; p.clips = clips;
    return prefill_attn_launch(true, p, B, H, st);
}

bool launch_prefill_cross_attention(const half_t *q, long ldq, const half_t *ck, const half_t *cv, half_t *out, long ldo, int B, int T,
                                    int H, int S, hipStream_t st, const PfClip *clips) {
    PrefillAttn p{};
    p.q = q; p.ldq = ldq; p.k = ck; p.v = cv; p.kv_clip = (long)H * S * NH_DH; p.kv_head = (long)S * NH_DH; p.kv_key = NH_DH;
    p.out = out; p.ldo = ldo; p.T = T; p.nk = S; p.C = 0; p.clips = clips;
    return prefill_attn_launch(false, p, B, H, st);
}
