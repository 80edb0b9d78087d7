// skinny_plan.h -- which decode GEMV kernel launch_skinny runs for a shape, as one pure host function: no HIP calls, no
// statics, so that it can be read, and tested, without a GPU (tools/kref.hip: kref_skinny_plan; tests/test_kref_cpu.py).
// launch_skinny (k_skinny.hip) is a switch over the plan and instantiates only what a plan can name.
#pragma once
#include <stddef.h>

enum SkinnyEpi {
    SK_F16 = 0,         // fp16 out (row stride ldo, per-row base offsets)
    SK_GELU_F16 = 1,
    SK_RESID_F32 = 2,   // f32 x[r][n] += acc + bias
    SK_F32 = 3,         // f32 out = acc (+bias)  (logits)
    SK_QKV = 4,         // self-attn fused q|k|v: q -> out[0] [R][d]; k,v -> caches at position t
};

#define LN_MAX_STEPS 10   // the sliced LayerNorm covers K = 128 steps, steps <= 10
#define LP_MT 2           // skinny_ldsp_kernel: weight tiles per wave, at most

enum SkinnyKind {
    SKP_NONE = 0,   // refused: nothing is launched
    SKP_GEMM,       // skinny_gemm_kernel<ncb, ksplit, nt>: K-sliced (ksplit = 2 .. 16, nt = 1) or full rows (ksplit = 1, nt = 2)
    SKP_LN,         // skinny_ln_kernel<ksplit, nt>: LayerNorm fused, ksplit holds STEPS = K / 128
    SKP_LDS,        // skinny_lds_kernel<ncb>: the logits, activations staged in LDS once
    SKP_LDSP,       // skinny_ldsp_kernel<ncb>: the logits for 33 .. 96 rows, K in phases of sp k-steps through the LDS
};
struct SkinnyPlan {
    int kind;
    int ncb;            // 16-row activation blocks per workgroup (the kernel's NCB; skinny_ln_kernel: always 1)
    int nt;             // 16-row weight tiles per wave (SKP_GEMM) or per workgroup (SKP_LN)
    int ksplit;         // SKP_GEMM: KSPLIT; SKP_LN: STEPS; SKP_LDS, SKP_LDSP: 1 (every wave walks the whole K)
    int sp;             // SKP_LDSP: k-steps per phase; else 0
    int grid_x, grid_y; // grid_y > 1: workgroup y handles activation rows 16 ncb y .. only
    int block;
    size_t lds_used;    // dynamic LDS the kernel uses (SKP_LDS, SKP_LDSP), else 0
    bool lds_exclusive; // launched with the CU's whole LDS (launch_lds_exclusive, nh_kernels.h) instead of lds_used
};

// R rows of activations, W [N][K]; has_wt: the tile-major repack of W exists; has_ln: the activations come through the fused
// LayerNorm (SkinnyParams::ln_x).  Refused (SKP_NONE): R outside 1 .. 96; K % 64 != 0 (the kernels walk K in 32-deep k-steps and
// the narrowest form cuts it in 2 slices: a tail of K would be dropped); N % 4 != 0 under any epilogue but SK_F32 (those store 4
// features at a time); has_ln on a shape no fused form covers -- any other kernel would read x instead of ln_x.  What has_ln
// accepts depends on (R, N, K) alone, never on the weight layout or the epilogue: it is skinny_ln_supported.
inline SkinnyPlan skinny_plan(int R, int N, int K, int epi, bool has_wt, bool has_ln) {
    SkinnyPlan pl = {SKP_NONE, 0, 0, 0, 0, 0, 0, 0, 0, false};
    if (R < 1 || R > 96 || N < 1 || K < 64 || K % 64 != 0) return pl;   // R <= 96 (nh_create rejects a larger max_batch)
    if (epi != SK_F32 && N % 4 != 0) return pl;
    const int NCB = (R + 15) / 16, tiles = (N + 15) / 16, steps = K >> 5;
    pl.grid_y = 1;
    if (has_ln && tiles < 2048) {
        const int s = K / 128;
        if (K % 128 != 0 || !(s == 1 || s == 2 || s == 3 || s == 4 || s == 6 || s == 8 || s == 10)) return pl;
        // one 16-row block per workgroup: any number of row blocks.
        // per-CU fetch = NT x (16 rows of W) + (16 NCB rows of x, f32): few tiles -> one tile x one 16-row block per workgroup;
        // many tiles -> two tiles x one 16-row block (as many workgroups as tiles, a fifth fewer bytes each than 1 tile x 32 rows)
        pl.kind = SKP_LN; pl.ncb = 1; pl.ksplit = s; pl.block = 256;
        pl.nt = (NCB > 1 && tiles > 160) ? 2 : 1;
        pl.grid_x = (tiles + pl.nt - 1) / pl.nt; pl.grid_y = NCB;
        return pl;
    }
    if (tiles >= 2048) {  // the tied-embedding logits: plenty of tiles, stream full rows
        const size_t lds = (size_t)steps * 16 * NCB * 64;
        // the fused final LayerNorm lives in skinny_lds_kernel's staging pass alone (sliced tree: K = 128 steps, steps <= 10)
        if (has_ln && !(NCB <= 2 && lds <= 96 * 1024 && K <= 128 * LN_MAX_STEPS && K % 128 == 0)) return pl;
        if (NCB <= 2 && lds <= 96 * 1024) {
            // `lds` is what the kernel uses; it is given the whole LDS of the CU (NH_LDS_EXCLUSIVE, see there)
            pl.kind = SKP_LDS; pl.ncb = NCB; pl.nt = 1; pl.ksplit = 1; pl.grid_x = 256; pl.block = 512;
            pl.lds_used = lds; pl.lds_exclusive = true;
            return pl;
        }
        if (NCB >= 3 && has_wt && tiles <= LP_MT * 2048) {
            // 33 .. 96 rows: K in phases through the LDS (skinny_ldsp_kernel); as few phases as 144 KiB of LDS allow, balanced
            const int spmax = (144 * 1024) / (16 * NCB * 64);
            const int phases = (steps + spmax - 1) / spmax, sp = (steps + phases - 1) / phases;
            // the kernel uses sp * 16 NCB * 64 bytes; it is given the whole LDS of the CU (NH_LDS_EXCLUSIVE, see there)
            pl.kind = SKP_LDSP; pl.ncb = NCB; pl.nt = LP_MT; pl.ksplit = 1; pl.sp = sp; pl.grid_x = 256; pl.block = 512;
            pl.lds_used = (size_t)sp * 16 * NCB * 64; pl.lds_exclusive = true;
            return pl;
        }
        if (NCB <= 4) {
            const int waves = (tiles + 1) / 2;
            pl.kind = SKP_GEMM; pl.ncb = NCB; pl.nt = 2; pl.ksplit = 1; pl.grid_x = (waves + 1) / 2; pl.block = 128;
            return pl;
        }
        // 65 .. 96 rows without the tile-major repack: no full-row form exists for NCB 5, 6 (its registers would not fit);
        // the split-row K-sliced form below handles any number of tiles
    }
    // waves per workgroup: every wave keeps a whole number of 32-deep k-steps, and at most ~10 of them (one group of
    // loads in flight = one memory round trip per wave).  r01 split the long-K layer (fc2, K = 4 d) across workgroups
    // instead (slab stores + ticket + slab loads: three more dependent round trips and cross-workgroup atomics for the
    // same ~11 us); 16 waves of one workgroup meet in LDS.
    // (the slicing must not depend on the batch: one summation order for every NCB = bit-exact batch invariance)
    // Few weight tiles (N <= 2560): one workgroup per (tile, 16-row block of the activations) -- the single-block
    // instantiation on a tiles x NCB grid -- so that a CU fetches 16 rows of activations instead of all of them
    // (skinny_gemm_kernel, rb).  Same per-row arithmetic as the NCB-block form.
    // (more than 64 rows -- several encoder batches decoded together -- always take the split form: no NCB = 5, 6 instantiation
    // of the unsplit kernel exists, its LDS reduction buffer would not fit)
    const bool split_rows = NCB > 4 || (NCB > 1 && tiles * NCB <= 640 && tiles <= 160);
    pl.kind = SKP_GEMM; pl.nt = 1;
    pl.ncb = split_rows ? 1 : NCB;
    pl.grid_x = tiles; pl.grid_y = split_rows ? NCB : 1;
    pl.ksplit = (K >= 2560 && K % 512 == 0) ? 16 : (K >= 2560 && K % 256 == 0) ? 8 : K % 128 == 0 ? 4 : 2;
    pl.block = 64 * pl.ksplit;
    return pl;
}
