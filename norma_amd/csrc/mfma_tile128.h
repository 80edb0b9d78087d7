// mfma_tile128.h -- the 128 x 128 x 64 MFMA tile loop and the tile orders of the kernels built on LDS-DMA tiles (gfx950):
// gemm_f16_kernel and gemm256_f16_kernel (k_gemm.hip), score_logits_kernel (k_score.hip).  Device code only.
#pragma once
#include "nh_kernels.h"

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

#define T128_TILE_BYTES (128 * 64 * 2)   // 16 KiB per operand tile
#define T128_LDS (4 * T128_TILE_BYTES)   // two buffers of an A and a B tile

// One 128 (A rows) x 128 (B rows) tile over nt K-tiles of 64, by a 256-thread workgroup (4 waves as 2 x 2, 64 x 64 per wave,
// v_mfma_f32_16x16x32_f16): acc += A . B^T, the 32-deep k-steps of an output added in ascending order into one accumulator.
// a_row(r) / b_row(r), r = 0 .. 127: the first of the nt * 64 K-contiguous halfs of the tile's A / B row r.  Every row is read,
// so the caller clamps rows past its matrix to a row it may read.
// LDS image (smem, T128_LDS bytes): [128 rows][8 chunks of 16 B], chunk' = chunk ^ ((row >> 1) & 7) (conflict-free
// ds_read_b128, MI355X LDS banking), double buffered.  Global->LDS is global_load_lds_dwordx4 (LDS-DMA, no VGPR round trip,
// no ds_write): the loads of tile t+1 are issued before the MFMAs of tile t.
// SWAP: the B rows are the MFMA "A" operand, D[row = B row][col = A row]: acc[i][j][r] is B row 64 wn + 16 i + 4 fq + r of
// A row 64 wm + 16 j + fr.  Otherwise D[row = A row][col = B row]: acc[i][j][r] is A row 64 wm + 16 j + 4 fq + r of B row
// 64 wn + 16 i + fr.  (w = wave, wm = w >> 1, wn = w & 1, fr = lane & 15, fq = lane >> 4.)
template <bool SWAP, class ARow, class BRow>
__device__ __forceinline__ void tile128_mainloop(ARow a_row, BRow b_row, int nt, char *smem, f32x4 (&acc)[4][4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    // staging map: slot s = tid + 256 i (i = 0..3): row = s >> 3, chunk' = s & 7 (tid & 7 for all i).
    // One wave-instruction covers 64 consecutive slots = 1 KiB of the LDS image, in lane order -- exactly
    // the (wave-uniform base + lane * 16) destination of global_load_lds; the swizzle lives in the SOURCE.
    const int cq = tid & 7;
    const half_t *ag[4], *wg[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = (tid >> 3) + 32 * i;
        const int c = cq ^ ((row >> 1) & 7);
        ag[i] = a_row(row) + c * 8;
        wg[i] = b_row(row) + c * 8;
    }
    // fragment read offsets (bytes within a tile): row r, chunk 4*ks + (lane>>4), swizzled
    const int fr = lane & 15, fq = lane >> 4;
    int offA[4], offB[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int rowA = wm * 64 + 16 * j + fr;
        const int rowB = wn * 64 + 16 * j + fr;
        offA[j] = rowA * 128 + ((fq ^ ((rowA >> 1) & 7)) << 4);
        offB[j] = rowB * 128 + ((fq ^ ((rowB >> 1) & 7)) << 4);
    }
    const int wbase = __builtin_amdgcn_readfirstlane(w) * 1024;  // this wave's 1 KiB run inside each 4 KiB group
    auto stage = [&](int buf, int t) {
        char *la = smem + buf * 2 * T128_TILE_BYTES + wbase, *lb = la + T128_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            __builtin_amdgcn_global_load_lds((gbl_void *)(ag[i] + (long)t * 64), (lds_void *)(la + 4096 * i), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gbl_void *)(wg[i] + (long)t * 64), (lds_void *)(lb + 4096 * i), 16, 0, 0);
        }
    };
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < nt; t++) {
        const bool more = (t + 1 < nt);
        if (more) stage(cur ^ 1, t + 1);  // all waves left buf[cur^1] at the barrier that ended iteration t-1
        const char *ta = smem + cur * 2 * T128_TILE_BYTES, *tb = ta + T128_TILE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            half8 fa[4], fb[4];
            // chunk index 4*ks + fq; the xor only touches the low 3 bits, and (4*ks) flips bit 2:
            // (4ks + fq) ^ g == (fq ^ g) ^ (4ks) because fq < 4 -> byte offset ^ (ks << 6)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                fa[j] = *reinterpret_cast<const half8 *>(ta + (offA[j] ^ (ks << 6)));
                fb[j] = *reinterpret_cast<const half8 *>(tb + (offB[j] ^ (ks << 6)));
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (SWAP) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[i], fa[j], acc[i][j], 0, 0, 0);
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[j], fb[i], acc[i][j], 0, 0, 0);
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA for tile t+1 has landed
        __syncthreads();
        cur ^= 1;
    }
}

// XCD-aware tile order: workgroups b and b + 8 share an XCD (L2).  The bijection of 0 .. nwg - 1 that gives every XCD a
// contiguous run of tiles.
__device__ __forceinline__ int xcd_contiguous(int b, int nwg) {
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// Tile bid of an ntm x ntn grid walked in groups of gsz row panels x all column tiles, column tile outer / row panel inner:
// the workgroups that follow each other read ONE column tile of the B operand and gsz row panels of A.
__device__ __forceinline__ void grouped_tile(int bid, int ntn, int ntm, int gsz, int &tm, int &tn) {
    const int per_group = gsz * ntn;
    const int g = bid / per_group, rr = bid - g * per_group;
    const int gm = min(gsz, ntm - g * gsz);  // the last group may hold fewer row panels
    tn = rr / gm; tm = g * gsz + (rr - tn * gm);
}
