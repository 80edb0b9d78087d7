// k_dec_attn.hip -- decoder attention of a decode step (gfx950).  HBM-bound: the cross-attention K/V are streamed once per
// generated token for the whole batch.
//
// Replaces, per decode step of Model::decode (src/models/whisper/model.rs:317-371):
//   dec_attn_kernel      qkv_attention of the decoder blocks (causal self-attention over the cache,
//                        cross-attention over the K/V cached at flush time)
// The absorbed cross-attention prototype (NH_OPT_ABSORBED_XATTN) is in k_xabs.hip.
#include "k_device.h"

// ---------------------------------------------------------------------------------------------------
// decoder attention, one query row per (b, h): 4 waves split the keys, inside a wave 8 key slots x
// 8 lanes (16 B of the 64-wide head each); each slot runs its own online softmax, merged at the end.
// ---------------------------------------------------------------------------------------------------
#define DA_U 4  // key groups (8 keys each) whose K and V rows are in flight together per wave: 2 x DA_U KiB (8: cross-attention 43 -> 46 us)
struct AttnPart { float m, l; float acc[8]; };

__device__ __forceinline__ void merge_part(AttnPart &a, float mo, float lo, const float (&ao)[8]) {
    float mn = fmaxf(a.m, mo);
    float sa = (a.m == -INFINITY) ? 0.f : __expf(a.m - mn);
    float so = (mo == -INFINITY) ? 0.f : __expf(mo - mn);
    a.l = a.l * sa + lo * so;
#pragma unroll
    for (int c = 0; c < 8; c++) a.acc[c] = a.acc[c] * sa + ao[c] * so;
    a.m = mn;
}

__global__ __launch_bounds__(256) void dec_attn_kernel(const half_t *__restrict__ q, const half_t *__restrict__ kc,
                                                       const half_t *__restrict__ vc, half_t *__restrict__ out,
                                                       int d, int ctx, int Tk, const int32_t *__restrict__ pos_ptr,
                                                       const int32_t *__restrict__ done) {
    // a finished sequence (eot, cap, or the no-speech exit) no longer streams its K/V: the reference's loop ends per
    // sequence at eot (model.rs:317); in a batch the others go on, and 0.49 GB of the 0.72 GB a step streams is per-sequence
    // cross K/V.  Its attention row is left as it was; every later product is row-wise, nothing of it reaches another row.
    if (done && done[blockIdx.y]) return;
    if (pos_ptr) Tk = pos_ptr[blockIdx.y] + 1;  // causal self-attention at this sequence's own position
    __shared__ float part[4][8][10];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int slot = lane >> 3, pp = lane & 7;
    const int h = blockIdx.x, b = blockIdx.y;
    float qv[8];
    {
        half8 qh = *reinterpret_cast<const half8 *>(q + (long)b * d + h * NH_DH + 8 * pp);
#pragma unroll
        for (int c = 0; c < 8; c++) qv[c] = (float)qh[c];
    }
    // candle scales q and k by dh^-1/4 each; the product of the two scalings is exactly 1/8
    const int per = (((Tk + 3) >> 2) + 7) & ~7;  // keys per wave, multiple of 8
    const int kbeg = w * per, kend = min(Tk, kbeg + per);
    // rows of one (clip, head), head-major [b][h][ctx][64]: the keys of a head are contiguous, a wave instruction reads
    // 1 KiB in one piece
    const long base = ((long)b * gridDim.x + h) * ctx * NH_DH;
    const half_t *kb = kc + base + 8 * pp;
    const half_t *vb = vc + base + 8 * pp;
    AttnPart st; st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int c = 0; c < 8; c++) st.acc[c] = 0.f;
    for (int j0 = kbeg; j0 < kend; j0 += 8 * DA_U) {
        half8 kk[DA_U], vv[DA_U];
#pragma unroll
        for (int u = 0; u < DA_U; u++) {
            int j = j0 + 8 * u + slot; if (j >= kend) j = kend - 1;
            // streamed once per token: non-temporal, so the K/V stream (491 MB per step at b32) does not evict the
            // decoder weights from the Infinity Cache between tokens
            kk[u] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(kb + j * NH_DH));
            vv[u] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(vb + j * NH_DH));
        }
#pragma unroll
        for (int u = 0; u < DA_U; u++) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 8; c++) s += qv[c] * (float)kk[u][c];
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
            s *= 0.125f;
            if (j0 + 8 * u + slot < kend) {
                float mn = fmaxf(st.m, s);
                float al = __expf(st.m - mn);  // exp(-inf) = 0 on the first key
                float pr = __expf(s - mn);
                st.l = st.l * al + pr;
#pragma unroll
                for (int c = 0; c < 8; c++) st.acc[c] = st.acc[c] * al + pr * (float)vv[u][c];
                st.m = mn;
            }
        }
    }
    // merge the 8 key slots of the wave (lane bits 3..5)
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
        float mo = __shfl_xor(st.m, o), lo = __shfl_xor(st.l, o);
        float ao[8];
#pragma unroll
        for (int c = 0; c < 8; c++) ao[c] = __shfl_xor(st.acc[c], o);
        merge_part(st, mo, lo, ao);
    }
    if (slot == 0) {
        part[w][pp][0] = st.m; part[w][pp][1] = st.l;
#pragma unroll
        for (int c = 0; c < 8; c++) part[w][pp][2 + c] = st.acc[c];
    }
    __syncthreads();
    if (tid < 8) {
        AttnPart a; a.m = part[0][tid][0]; a.l = part[0][tid][1];
#pragma unroll
        for (int c = 0; c < 8; c++) a.acc[c] = part[0][tid][2 + c];
        for (int ww = 1; ww < 4; ww++) {
            float ao[8];
#pragma unroll
            for (int c = 0; c < 8; c++) ao[c] = part[ww][tid][2 + c];
            merge_part(a, part[ww][tid][0], part[ww][tid][1], ao);
        }
        float inv = 1.0f / a.l;
        half8 o;
#pragma unroll
        for (int c = 0; c < 8; c++) o[c] = (half_t)(a.acc[c] * inv);
        *reinterpret_cast<half8 *>(out + (long)b * d + h * NH_DH + 8 * tid) = o;
    }
}

void launch_dec_attention(const half_t *q, const half_t *kc, const half_t *vc, half_t *out, int B, int H, int d, int ctx, int Tk,
                          const int32_t *pos_ptr, hipStream_t st, const int32_t *done) {
    hipLaunchKernelGGL(dec_attn_kernel, dim3(H, B), dim3(256), 0, st, q, kc, vc, out, d, ctx, Tk, pos_ptr, done);
}
