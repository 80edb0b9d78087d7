"""Kernel-level fp64 references for the launchers of norma_amd/csrc/nh_kernels.h, their error bounds, and the loader of
tools/bin/libnh_kref.so (tools/kref.hip: C entry points onto the shipped launchers).

Every reference is plain NumPy in float64 on the exact fp16 / f32 values the kernel was given.  Every bound is a formula
derived from the kernel's arithmetic (the comments say how), never a constant fitted to what the GPU produced.  u = 2^-24 is the
unit roundoff of f32, 2^-11 that of fp16.  A test also shows that its bound is tight enough to matter: `discriminates` rebuilds
the reference under plausible bugs (a dropped k-step, a missing bias tile, a key too few ...) and requires each of them to leave
the bound by a factor of two on the case's own data, so that a kernel with that bug would fail the case.
One stated limit: enc_attn_kernel clamps -m_ref to +-60000 log2 units (the largest fp16 pair it can subtract); encoder scores
beyond that are out of scope of its reference, bound and cases."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tools", "bin", "libnh_kref.so")
U32 = 2.0 ** -24      # f32 unit roundoff
U16 = 2.0 ** -11      # fp16 unit roundoff
SUB16 = 2.0 ** -25    # half the spacing of fp16 subnormals: the absolute part of rounding to fp16
NH_SP, NH_DH = 1536, 64
ENC_Q_SCALE = float(np.float32(np.float32(0.125) * np.float32(1.4426950408889634)))
SK_F16, SK_GELU_F16, SK_RESID_F32, SK_F32, SK_QKV = 0, 1, 2, 3, 4
SKP_NONE, SKP_GEMM, SKP_LN, SKP_LDS, SKP_LDSP = 0, 1, 2, 3, 4      # SkinnyKind of norma_amd/csrc/skinny_plan.h
PLAN_FIELDS = ("kind", "ncb", "nt", "ksplit", "sp", "grid_x", "grid_y", "block", "lds_used", "lds_exclusive")
EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_CONV2_F32 = 0, 1, 2, 3
WRAPPERS = ["kref_skinny", "kref_skinny_ln_supported", "kref_skinny_plan", "kref_dec_attention", "kref_xabs_attention", "kref_enc_attention",
            "kref_gemm", "kref_layernorm", "kref_embed", "kref_logit_step", "kref_sample_step", "kref_lang_detect",
            "kref_prefill_self_attention", "kref_prefill_cross_attention", "kref_mel_tables", "kref_mel_groups", "kref_logmel",
            "kref_mel_finish"]

# ---- loader ----------------------------------------------------------------------------------------------------------------
_lib = None


def load():
    """The wrapper library; a GPU run without it FAILS (pytest.fail): a vacuous pass is not a pass."""
    global _lib
    if _lib is None:
        import pytest
        if not os.path.exists(LIB_PATH):
            pytest.fail(f"{LIB_PATH} is not built (python -c 'import __graft_entry__ as g; g.build()')")
        _lib = C.CDLL(LIB_PATH)
        for n in WRAPPERS:
            getattr(_lib, n).restype = C.c_int
    return _lib


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _argtypes():
    L = load()
    vp, i, l, z, f = C.c_void_p, C.c_int, C.c_long, C.c_size_t, C.c_float
    L.kref_skinny.argtypes = [vp, l, i, i, i, vp, vp, i, i, vp, z, vp, vp, z, l, i, i, i, i, vp, i, vp, vp, vp]
    L.kref_skinny_ln_supported.argtypes = [i, i, i]
    L.kref_skinny_plan.argtypes = [i, i, i, i, i, i, vp]
    L.kref_dec_attention.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, i, vp]
    L.kref_xabs_attention.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp, i]
    L.kref_enc_attention.argtypes = [vp, vp, l, vp, vp, l, i, i, i]
    L.kref_gemm.argtypes = [i, vp, z, l, i, l, vp, vp, i, i, i, i, vp, vp, vp, z, i, l, i, l, l, i, i, f, i, i, vp]
    L.kref_layernorm.argtypes = [i, vp, vp, vp, vp, vp, i, i]
    L.kref_embed.argtypes = [vp, i, vp, i, vp, i, vp, i, i, i, vp, i]
    L.kref_logit_step.argtypes = [vp, i, i, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp]
    L.kref_sample_step.argtypes = [vp, i, i, i, i, i, i, i, f, C.c_ulonglong, C.c_uint, C.c_uint, vp, vp, vp, vp, vp, vp, vp,
                                   vp, vp]
    L.kref_lang_detect.argtypes = [vp, i, i, vp, i, vp, vp]
    L.kref_prefill_self_attention.argtypes = [vp, vp, vp, l, vp, l, vp, vp, i, i, i, i]
    L.kref_prefill_cross_attention.argtypes = [vp, l, vp, vp, vp, l, i, i, i, i]
    L.kref_mel_tables.argtypes = [vp, vp, vp, vp, vp]
    L.kref_mel_groups.argtypes = [vp, i, vp]
    L.kref_logmel.argtypes = [vp, l, vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, vp, l, l, vp, l, l]
    L.kref_mel_finish.argtypes = [vp, l, l, vp, l, l, vp, l, l, i, i, i, i]
    return L


def lib():
    L = load()
    if L.kref_skinny.argtypes is None:
        _argtypes()
    return L


def skinny_plan(R, N, Kd, epi, wt, ln):
    """skinny_plan (norma_amd/csrc/skinny_plan.h) of a launch_skinny shape as a dict of PLAN_FIELDS; pure host code: the
    wrapper library answers without a GPU"""
    out = np.zeros(10, dtype=np.int32)
    planned = lib().kref_skinny_plan(R, N, Kd, epi, int(wt), int(ln), ptr(out))
    plan = dict(zip(PLAN_FIELDS, (int(v) for v in out)))
    assert planned == (plan["kind"] != SKP_NONE)
    return plan


def check_rc(rc, what):
    assert rc == 0, f"{what}: launcher returned {rc}" + (" (shape refused)" if rc == -1 else " (hipError_t)")


# ---- data ------------------------------------------------------------------------------------------------------------------
def f16(a):
    return np.ascontiguousarray(a, dtype=np.float16)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def d64(a):
    return np.asarray(a, dtype=np.float64)


# ---- references ------------------------------------------------------------------------------------------------------------
def gelu(v):
    """tanh-GELU (nh_kernels.h gelu_tanh_fast is the same function, evaluated as v / (1 + exp(-2u)))"""
    return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))


def linear(x, W, bias=None):
    """x [R][K] . W[N][K]^T (+ bias) in fp64, and sum_k |x_k||w_k| per output (the scale of the accumulation error)"""
    x, W = d64(x), d64(W)
    y = x @ W.T
    if bias is not None:
        y = y + d64(bias)
    return y, np.abs(x) @ np.abs(W).T


def layernorm(x, w, b, eps=1e-5):
    """LayerNorm in fp64 (biased variance, eps inside the root, as candle / both kernels)"""
    x = d64(x)
    m = x.mean(axis=-1, keepdims=True)
    t = x - m
    var = (t * t).mean(axis=-1, keepdims=True)
    inv = 1.0 / np.sqrt(var + eps)
    return t * inv * d64(w) + d64(b), inv, t


def softmax_attend(s, v):
    """softmax over the last axis of s (fp64, max subtracted), then . v"""
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return p @ v


def dec_attention(q, k, v, H, nvis):
    """decoder attention of one query row per (b, h): q [B][d], k/v [B][T][d] (row-major form), nvis[b] visible keys (the first
    ones); scores q.k / 8 (candle scales q and k by dh^-1/4 each).  Returns o [B][d], sabs [B][H] = max over the visible keys
    of sum_c |q_c||k_c| / 8 (the scale of the score error), and (vdev, pv) [B][H][64] = sum_j p_j |v_j - o|, sum_j p_j |v_j|"""
    q, k, v = d64(q), d64(k), d64(v)
    B, d = q.shape
    T = k.shape[1]
    qh = q.reshape(B, H, NH_DH)
    kh, vh = k.reshape(B, T, H, NH_DH), v.reshape(B, T, H, NH_DH)
    vis = np.arange(T)[None, :] < np.asarray(nvis).reshape(B, 1)            # [B][T]
    s = np.einsum("bhc,bthc->bht", qh, kh) / 8.0
    s = np.where(vis[:, None, :], s, -np.inf)
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    o = np.einsum("bht,bthc->bhc", p, vh).reshape(B, d)
    sabs = np.where(vis[:, None, :], np.einsum("bhc,bthc->bht", np.abs(qh), np.abs(kh)), 0).max(axis=-1) / 8.0
    oh = o.reshape(B, H, 1, NH_DH)
    vdev = np.einsum("bht,bhtc->bhc", p, np.abs(vh.transpose(0, 2, 1, 3) - oh))       # sum_j p_j |v_j - o|
    pv = np.einsum("bht,bthc->bhc", p, np.abs(vh))                                     # sum_j p_j |v_j|
    return o, sabs, (vdev, pv)


def head_major(kv, H):
    """[B][T][d] -> [B][H][T][64] (GemmParams::head_major, the decoder's cache layout)"""
    B, T, d = kv.shape
    return np.ascontiguousarray(kv.reshape(B, T, H, NH_DH).transpose(0, 2, 1, 3))


def vt_image(v, H, S):
    """[B*S][d] -> V^T image [B][H][64][NH_SP] (GemmParams::vt_seg), pad columns S..NH_SP-1 zero"""
    d = H * NH_DH
    B = v.shape[0] // S
    out = np.zeros((B, H, NH_DH, NH_SP), dtype=v.dtype)
    out[:, :, :, :S] = v.reshape(B, S, H, NH_DH).transpose(0, 2, 3, 1)
    return out


def xabs_projected(xa, Wkv, bkv, d):
    """K = xa Wk^T + bk and V = xa Wv^T + bv in fp64 (the cross K/V the absorbed form never materialises)"""
    xa, Wkv, bkv = d64(xa), d64(Wkv), d64(bkv)
    return xa @ Wkv[:d].T + bkv[:d], xa @ Wkv[d:].T + bkv[d:]


def _softmax_cols(s):
    """softmax over axis 0 of s [S][H] (fp64)"""
    p = np.exp(s - s.max(axis=0, keepdims=True))
    return p / p.sum(axis=0, keepdims=True)


def xabs_attention(q, Wkv, bkv, xa, H, round_u=False):
    """softmax(q.(xa Wk^T + bk)^T / 8) . (xa Wv^T + bv) per (row, head): q [B][d], xa [B][S][d].  Evaluated re-associated in fp64
    (exact in real arithmetic): the scores are xa . u_h with u_h = Wk_h^T q_h / 8, plus q_h . bk_h / 8 (a per-head constant: it
    cancels in the softmax), the output Wv_h (sum_s p_s xa_s) + bv_h.  round_u: u rounded to fp16 first (what the kernels'
    fp16 U buffer holds).  Returns o [B][d]."""
    q, Wkv, bkv = d64(q), d64(Wkv), d64(bkv)
    B, d = q.shape
    Wk, Wv = Wkv[:d].reshape(H, NH_DH, d), Wkv[d:].reshape(H, NH_DH, d)
    o = np.zeros((B, H, NH_DH))
    for b in range(B):
        x = d64(xa[b])
        u = np.einsum("hjc,hj->hc", Wk, q[b].reshape(H, NH_DH)) / 8.0
        if round_u:
            u = d64(f16(u))
        z = _softmax_cols(x @ u.T).T @ x                                             # [H][d]
        o[b] = np.einsum("hjc,hc->hj", Wv, z) + bkv[d:].reshape(H, NH_DH)
    return o.reshape(B, d)


def xabs_reference(q, Wkv, bkv, xa, H):
    """the fp64 formula (xabs_attention) and the bound of both absorbed forms against it.  The kernels compute
    u = fp16(0.125 acc), acc an f32 dot of 64 fp16 products (depth <= 64), so |u_f32 - u| <= 66 u32 sum_j |Wk_jc||q_j| / 8;
    their fp16 u equals fp16(u) except where u lies that close to a rounding midpoint ("ties"), where it may be the other
    neighbour: one ulp16 away.  Against o16 = the formula with fp16(u) (round_u), writing y_s = Wv_h xa_s (key s's value row):
      score error  e <= sum_c[ties] |xa_c| ulp16(u_c) + Ds u32 sum_c |xa_c||fp16(u_c)| + 4 u32, where Ds = d / 8 + 32 bounds
                   the depth of the f32 score dot (xabs_attn_kernel: d / 64 per lane + 6 butterfly levels; xabs_main_kernel:
                   d / 8 features per wave in MFMAs of 16 + 8 waves met in LDS); the fast exp's argument error 2 u32 |s - m|
                   is inside the dot term (|s - m| <= 2 max sum|xa||u|)
      softmax      perturbing the scores by e_s moves o by sum_s p_s e_s (y_s - o) to first order (Wv_h is linear), and P in
                   fp16 the same way with 2^-11: |do| <= (2 e + 2 * 2^-11) sum_s p_s |y_s - o| (doubled for the second order)
      sums / z     the online accumulation of z (S / 4 keys per wave or 32-key MFMA tiles per key range, two roundings per step,
                   four ranges merged): (S / 2 + 64) u32 (sum_s p_s |xa_s| + |z|); z rounded to fp16: 2^-11 |z|; both carried
                   by |Wv_h|
      output       2^-11 |o| + 2^-25 + Dv u32 |Wv_h| |z| (1 + 2^-11) + u32 |bv|, Dv = d / 4 + 8 (the value dot: d / 4 per
                   thread + 2 shuffles, or d / 8 per wave + 8 waves)
    and |o16 - o| is computed exactly in fp64: bound = that + the above (triangle inequality).  sum_s p_s |y_s - o| is summed
    over the keys that hold all but 2^-40 of the weight; the rest is bounded by 2^-40 (|Wv_h| max_s |xa_s| + |o|).
    Returns o [B][d] (the formula) and the bound [B][d]."""
    q, Wkv, bkv = d64(q), d64(Wkv), d64(bkv)
    B, d = q.shape
    S = xa.shape[1]
    Wk, Wv = Wkv[:d].reshape(H, NH_DH, d), Wkv[d:].reshape(H, NH_DH, d)
    aWv, bv = np.abs(Wv), bkv[d:].reshape(H, NH_DH)
    Ds, Dv = d / 8 + 32, d / 4 + 8
    o, bound = np.zeros((B, H, NH_DH)), np.zeros((B, H, NH_DH))
    for b in range(B):
        x = d64(xa[b])
        ax = np.abs(x)
        qh = q[b].reshape(H, NH_DH)
        u = np.einsum("hjc,hj->hc", Wk, qh) / 8.0
        uerr = 66 * U32 * np.einsum("hjc,hj->hc", np.abs(Wk), np.abs(qh)) / 8.0
        u16 = d64(f16(u))
        tie = f16(u - uerr) != f16(u + uerr)
        tie_ulp = np.where(tie, d64(np.spacing(f16(np.abs(u) + uerr))), 0.0)
        e = (ax @ tie_ulp.T + Ds * U32 * (ax @ np.abs(u16).T)).max(axis=0) + 4 * U32        # [H]
        p16, p64 = _softmax_cols(x @ u16.T), _softmax_cols(x @ u.T)                    # [S][H]
        z16, z64 = p16.T @ x, p64.T @ x                                                  # [H][d]
        pxa, az = p16.T @ ax, np.abs(z16)
        o16 = np.einsum("hjc,hc->hj", Wv, z16) + bv
        o[b] = np.einsum("hjc,hc->hj", Wv, z64) + bv
        xmax = ax.max(axis=0)
        dev = np.zeros((H, NH_DH))
        for h in range(H):
            order = np.argsort(p16[:, h])[::-1]
            keep = order[:int(np.searchsorted(np.cumsum(p16[order, h]), 1.0 - 2.0 ** -40)) + 1]
            y = x[keep] @ Wv[h].T + bv[h]                                                # [keys][64]
            dev[h] = p16[keep, h] @ np.abs(y - o16[h]) + 2.0 ** -40 * (aWv[h] @ xmax + np.abs(bv[h]) + np.abs(o16[h]))
        dz = (S / 2 + 64) * U32 * (pxa + az) + U16 * az
        bound[b] = (np.abs(o16 - o[b]) + U16 * np.abs(o16) + SUB16 + (2 * e + 2 * U16)[:, None] * dev
                    + np.einsum("hjc,hc->hj", aWv, dz) + Dv * U32 * (1 + U16) * np.einsum("hjc,hc->hj", aWv, az)
                    + U32 * np.abs(bv))
    return o.reshape(B, d), bound.reshape(B, d)


def enc_attention(q, k, v, B, S, H):
    """encoder attention with q PRE-SCALED by NH_ENC_Q_SCALE: p = 2^(q.k) normalised (the log2(e) change of base lives in q);
    q, k, v [B*S][d].  Returns o [B*S][d], sabs [B*S][H] = max over the keys of sum_c |q_c||k_c| (score error scale, log2
    units) and (vdev, pv) [B*S][H][64] as dec_attention does"""
    q, k, v = d64(q), d64(k), d64(v)
    d = H * NH_DH
    o = np.zeros((B * S, d))
    sabs = np.zeros((B * S, H))
    vdev, pv = np.zeros((B * S, H, NH_DH)), np.zeros((B * S, H, NH_DH))
    for b in range(B):
        r = slice(b * S, (b + 1) * S)
        for h in range(H):
            c = slice(h * NH_DH, (h + 1) * NH_DH)
            s = (q[r, c] @ k[r, c].T) * np.log(2.0)
            s -= s.max(axis=-1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(axis=-1, keepdims=True)
            o[r, c] = p @ v[r, c]
            sabs[r, h] = (np.abs(q[r, c]) @ np.abs(k[r, c]).T).max(axis=-1)
            pv[r, h] = p @ np.abs(v[r, c])
            for i0 in range(0, S, 256):   # sum_j p_ij |v_j - o_i| in blocks of queries
                i1 = min(S, i0 + 256)
                vdev[b * S + i0:b * S + i1, h] = np.einsum("ij,ijc->ic", p[i0:i1], np.abs(v[r, c][None] - o[r, c][i0:i1, None]))
    return o, sabs, (vdev, pv)


# ---- enc_attn_kernel's deferred-maximum softmax (k_attn_enc.hip) -------------------------------------------------------------
# The kernel walks the keys in tiles of 64.  Its reference maximum m_ref is the tile maximum on tile 0 and moves afterwards only
# where a tile's maximum exceeds it by more than 8 log2 units (a "rebase": O and l are rescaled, the tile's scores shifted, and
# the pair of fp16 numbers that subtracts m_ref inside the score product rewritten); in between p = exp2(s - m_ref) runs up to
# 256.  None of that changes the result in real arithmetic, so the value reference stays enc_attention; what follows is the
# accounting that says which of these paths a case's inputs reach (enc_rebase_replay), the two bound terms the scheme adds
# (attn_bound's mref and p_floor), the adversarial cases (enc_rebase_case), and a NumPy emulation of the kernel's arithmetic
# with its rebase bugs (enc_emulate) for `discriminates`.
# Out of scope: scores beyond +-60000 log2 units.  The kernel clamps -m_ref there (fp16 has no larger finite number); no case
# here comes within a factor of 40 of it, and the bound has no term for the clamp.
ENC_KT = 64            # `#define KT 64` (k_attn_enc.hip:28): keys per tile
ENC_QW = 32            # `#define QW 32` (k_attn_enc.hip:29): queries per wave, one per lane of either half
ENC_REBASE = 8.0       # `const float REBASE = 8.0f` (k_attn_enc.hip:135), used as `reb = (t == 0) || (mx > REBASE)` (:178)
ENC_CLAMP = 60000.0    # `fminf(fmaxf(-m_ref, -60000.f), 60000.f)` (k_attn_enc.hip:186)
ENC_KEY_HALF = (np.arange(ENC_KT) >> 3) & 1    # the lane half that owns in-tile key position j: bit 3 (rho = (i & 3) + 8 (i >> 2) + 4 hh
#                                                is the LDS row, swap23(rho) the key: k_attn_enc.hip:163-164)
ENC_DH_HALF = (np.arange(NH_DH) >> 2) & 1      # the lane half that owns output dimension c: bit 2 (`+ 4 * hh`, k_attn_enc.hip:267)
ENC_REBASE_CASES = ("ramp", "spike", "threshold", "offset")
ENC_REBASE_SHAPES = ((1, 750), (2, 750), (1, 1500))     # (B, S) at H = 2: the last tile holds 46 or 28 keys
ENC_BUGS = {"rebase forgets to rescale l": "no_l", "rebase forgets to rescale O": "no_o",
            "later tiles keep the old m_ref (qx not updated)": "no_qx", "the key halves do not share the maximum": "no_share"}
ENC_THR_DELTA = 2.0 ** -6    # the threshold case's distance from REBASE; enc_rebase_case says why it is large enough
ENC_SPIKE = 80.0             # the spike case's dominating score


def _enc_tiles(s, S):
    """scores [S][S] -> [S][nT][64], keys past S at -inf"""
    nT = -(-S // ENC_KT)
    p = np.full((s.shape[0], nT * ENC_KT), -np.inf)
    p[:, :S] = s
    return p.reshape(s.shape[0], nT, ENC_KT)


def enc_rebase_replay(q, k, S, H):
    """the kernel's rule for m_ref, replayed in fp64 for every (query, head) of q, k [B*S][64 H] (q pre-scaled): on tile 0 m_ref
    is the tile maximum; on a later tile t it moves to the tile maximum only where gap[t] = max_t - m_ref > ENC_REBASE.  Coverage
    accounting only: the output does not depend on these decisions.  Returns a dict of arrays over [B*S][H] (`rows`):
      rebase [rows][nT]   the rebase map (tile 0: True)
      gap [rows][nT]      tile maximum - m_ref before the decision (tile 0: 0); a non-rebasing tile's largest p is 2^gap
      pos [rows][nT]      in-tile position of the tile's maximum
      near [rows][nT]     |gap - 8| <= 2 e: the kernel may decide either way.  e = attn_score_error(sabs, mref = max |m_ref|) is
                          the score error of attn_bound in log2 units; twice, because the kernel's m_ref is itself a computed
                          score
      decided [rows][nT]  no near pair at or before this tile: later tiles of a query inherit an undecided m_ref
      p_max [rows]        the largest p of a decided, non-rebasing tile after tile 0 (0 where there is none)
      m_final, m_absmax, margin (largest score - second largest over all keys), top_tile (the tile of the largest score), sabs,
      e [rows]"""
    q, k = d64(q), d64(k)
    B = q.shape[0] // S
    nT = -(-S // ENC_KT)
    out = {n: np.zeros((B * S, H, nT), dt) for n, dt in (("rebase", bool), ("gap", float), ("pos", np.int64))}
    for n in ("m_final", "m_absmax", "margin", "sabs"):
        out[n] = np.zeros((B * S, H))
    out["top_tile"] = np.zeros((B * S, H), np.int64)
    for b in range(B):
        r = slice(b * S, (b + 1) * S)
        for h in range(H):
            c = slice(h * NH_DH, (h + 1) * NH_DH)
            s = q[r, c] @ k[r, c].T
            top = np.partition(s, S - 2, axis=-1)
            out["margin"][r, h] = top[:, S - 1] - top[:, S - 2]
            out["top_tile"][r, h] = s.argmax(axis=-1) // ENC_KT
            out["sabs"][r, h] = (np.abs(q[r, c]) @ np.abs(k[r, c]).T).max(axis=-1)
            tiles = _enc_tiles(s, S)
            tmax, out["pos"][r, h] = tiles.max(axis=-1), tiles.argmax(axis=-1)
            m = tmax[:, 0].copy()
            out["rebase"][r, h, 0] = True
            mabs = np.abs(m)
            for t in range(1, nT):
                g = tmax[:, t] - m
                rb = g > ENC_REBASE
                out["gap"][r, h, t], out["rebase"][r, h, t] = g, rb
                m = np.where(rb, tmax[:, t], m)
                mabs = np.maximum(mabs, np.abs(m))
            out["m_final"][r, h], out["m_absmax"][r, h] = m, mabs
    out["e"] = attn_score_error(out["sabs"], mref=out["m_absmax"])
    near = np.abs(out["gap"] - ENC_REBASE) <= 2 * out["e"][:, :, None]
    near[:, :, 0] = False
    out["near"] = near
    out["decided"] = ~(np.cumsum(near, axis=-1) > 0)
    quiet = out["decided"] & ~out["rebase"]
    out["p_max"] = np.where(quiet, np.exp2(np.minimum(out["gap"], ENC_REBASE)), 0.0).max(axis=-1)
    return out


def enc_p16_floor(q, k, v, B, S, H):
    """attn_bound's p_floor for enc_attn_kernel, [B*S][H][64]: 2^-25 sum |v_j| over the keys whose weight CAN be below 2^-14 when
    the kernel rounds it to fp16.  m_ref never exceeds the running maximum of the tiles up to the key's own, so the kernel's
    p_j = 2^(s_j - m_ref) >= 2^(s_j - running maximum): the keys with s_j - running maximum < -14 are a superset, whatever the
    rebase decisions were.  Later rescalings multiply by alpha <= 1 and l >= 1."""
    q, k, v = d64(q), d64(k), d64(v)
    floor = np.zeros((B * S, H, NH_DH))
    tile_of = np.arange(S) // ENC_KT
    for b in range(B):
        r = slice(b * S, (b + 1) * S)
        for h in range(H):
            c = slice(h * NH_DH, (h + 1) * NH_DH)
            s = q[r, c] @ k[r, c].T
            run = np.maximum.accumulate(_enc_tiles(s, S).max(axis=-1), axis=-1)
            floor[r, h] = SUB16 * ((s - run[:, tile_of] < -14.0) @ np.abs(v[r, c]))
    return floor


def enc_attention_keys(q, k, v, B, S, H, nk):
    """encoder attention of every query over the first nk keys of its clip only (a tile mask that ends early); o [B*S][64 H]"""
    q, k, v = d64(q), d64(k), d64(v)
    o = np.zeros_like(q)
    for b in range(B):
        r, rk = slice(b * S, (b + 1) * S), slice(b * S, b * S + nk)
        for h in range(H):
            c = slice(NH_DH * h, NH_DH * h + NH_DH)
            o[r, c] = softmax_attend((q[r, c] @ k[rk, c].T) * np.log(2.0), v[rk, c])
    return o


def enc_emulate(q, k, v, B, S, H, bug=None, tile0_rescale=False):
    """enc_attn_kernel's arithmetic in NumPy: f32 scores of the fp16 operands; -m_ref as hi + lo, two fp16 numbers added to the
    score in f32; per query and per 64-key tile the maximum, the rebase rule, alpha = exp2(-dlt) on O and l, the tile's scores
    shifted by dlt; p = exp2(s') in f32, summed into l as it is and rounded to fp16 for the P.V product; O in f32; O / l rounded
    to fp16.  The two lane halves of a query are kept apart as the kernel keeps them: half hh owns the keys ENC_KEY_HALF == hh
    (their maximum, their part of l), the output dimensions ENC_DH_HALF == hh and a copy of m_ref; hi and lo live in half 0.
    bug: None, or a value of ENC_BUGS -- on rebases AFTER tile 0 "no_l" / "no_o" leave l / O unscaled and "no_qx" leaves hi, lo
    at their earlier values; "no_share" drops the exchange of the maximum between the halves.
    tile0_rescale=True is the kernel's former arithmetic: O and l, still zero, multiplied by alpha on tile 0 too -- 0 x inf = NaN
    as soon as tile 0's maximum is below -128."""
    f = np.float32
    assert bug in (None,) + tuple(ENC_BUGS.values())
    nT = -(-S // ENC_KT)
    own = ENC_KEY_HALF
    out = np.zeros((B * S, H * NH_DH), np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            r = slice(b * S, (b + 1) * S)
            for h in range(H):
                c = slice(h * NH_DH, (h + 1) * NH_DH)
                qq, kk = q[r, c].astype(f), np.zeros((nT * ENC_KT, NH_DH), f)
                vv = np.zeros((nT * ENC_KT, NH_DH), f)
                kk[:S], vv[:S] = k[r, c], v[r, c]
                m, l, O = np.zeros((2, S), f), np.zeros((2, S), f), np.zeros((2, S, NH_DH), f)
                hi, lo = np.zeros(S, f), np.zeros(S, f)
                for t in range(nT):
                    ks = slice(t * ENC_KT, (t + 1) * ENC_KT)
                    s = ((qq @ kk[ks].T + hi[:, None]) + lo[:, None]).astype(f)
                    s[:, np.arange(ks.start, ks.stop) >= S] = -np.inf
                    mx = np.stack([s[:, own == 0].max(axis=-1), s[:, own == 1].max(axis=-1)])
                    if bug != "no_share":
                        mx = np.broadcast_to(np.maximum(mx[0], mx[1]), (2, S))
                    reb = np.full((2, S), True) if t == 0 else mx > f(ENC_REBASE)
                    dlt = np.where(reb, mx, f(0)).astype(f)
                    alpha = np.exp2(-dlt).astype(f)
                    if t == 0 and not tile0_rescale:
                        alpha = np.ones((2, S), f)
                    O *= (np.ones((2, S, 1), f) if bug == "no_o" and t else alpha[:, :, None])
                    l *= (np.ones((2, S), f) if bug == "no_l" and t else alpha)
                    s = (s - dlt[own].T).astype(f)
                    m += dlt
                    if not (bug == "no_qx" and t):
                        nm = np.clip(-m[0], f(-ENC_CLAMP), f(ENC_CLAMP))
                        hi = nm.astype(np.float16).astype(f)
                        lo = (nm - hi).astype(np.float16).astype(f)
                    p = np.exp2(s).astype(f)
                    for hh in (0, 1):
                        l[hh] += p[:, own == hh].sum(axis=-1, dtype=f)
                    O += (p.astype(np.float16).astype(f) @ vv[ks])[None]
                inv = f(1) / (l[0] + l[1])
                out[r, c] = (np.where(ENC_DH_HALF == 0, O[0], O[1]) * inv[:, None]).astype(np.float16)
    return out


def _enc_units(r, H, signs=False):
    """one unit direction per head, [H][64]: Gaussian, or all components +-1/8 (its multiples by n / 4 are exact in fp16)"""
    if signs:
        return r.choice([-0.125, 0.125], size=(H, NH_DH))
    u = r.standard_normal((H, NH_DH))
    return u / np.linalg.norm(u, axis=-1, keepdims=True)


_ENC_CASES = {}


def enc_rebase_case(name, B, S, H=2):
    """the adversarial inputs of enc_attn_kernel's rebase tests: (q, k, v) fp16 [B*S][64 H], q pre-scaled; built once per (name,
    B, S, H) and shared (read-only).  Gaussian q (sigma ENC_Q_SCALE) and k, v; u_h a unit direction per head; i, j the query and
    key index in the clip, t = j // 64 the key's tile:
      ramp       k_j += t u, q_i += a u with a = +11, +3, 0, -11 by i % 4: one wave holds queries whose scores rise by 11 a tile
                 (a rebase every tile), by 3 (a rebase every third tile, p up to 256 in between), not at all, and fall by 11
                 (no rebase; the later keys' weights sink through the fp16 subnormals to zero)
      spike      every key is the dominating key of one query: q_i Gaussian directions of one length, k_pi(i) = ENC_SPIKE q_i /
                 |q_i|^2 for a random permutation pi of the clip's keys (as test_dec_attention_adversarial_scores plants its
                 keys): q_i scores ENC_SPIKE on its own key and ENC_SPIKE cos(q_i, q_i') on the others, at least 20 less (checked:
                 `margin`).  Every in-tile position of every tile is some query's, key S - 1 and keys 31 / 32 of each tile
                 among them; the rebase to the spike falls into tile 1, a middle tile or the masked last tile accordingly
      threshold  u_h with components +-1/8; one key per tile is (8 + 2 t) u exactly, the last tile's is key S - 1; q_i = g_i +
                 (4 +- delta / 2) u, + for even i, g_i Gaussian made orthogonal to u: the peak of tile t scores (4 +- delta / 2)
                 (8 + 2 t), every tile's peak lies 8 +- delta above the one before.  Even queries rebase on every tile by
                 8 + delta; odd ones stay on the odd tiles with p = 2^(8 - delta) and rebase by 16 - 2 delta on the even ones.
                 delta = ENC_THR_DELTA = 2^-6: the peaks are exact products of fp16 numbers up to the rounding of q (about 1e-4
                 in the gap), and 2 e < 2e-3 at the largest scores of the case (S = 1500: 4 * 54 = 216, e = 64 u 230 + ..), so
                 both sides are decided; p stays above 2^(8 - 2 delta) = 250
      offset     q_i += +-35 u (+ for even i), k_j += 32 u: every score of a query sits near +1120 or -1120, m_ref of either sign
                 near 1100, hi and lo both in use.  The keys' own spread along u (sigma 35 log2 units) is common to all queries of
                 one sign, so they agree on the winning key and key S - 1 would matter to none of them: per (clip, head) the last
                 key is set to a multiple of one query's direction that scores the log2-sum-exp2 of that query's other scores
                 (half the weight, as _xabs_case gives it); the query is even in head 0 and odd in head 1."""
    key = (name, B, S, H)
    if key in _ENC_CASES:
        return _ENC_CASES[key]
    assert name in ENC_REBASE_CASES
    r = np.random.default_rng(zlib_key("enc-rebase", name, B, S, H))
    d = H * NH_DH
    i = np.arange(B * S) % S
    tile = (i // ENC_KT).astype(np.float64)
    q = r.standard_normal((B * S, H, NH_DH)) * ENC_Q_SCALE
    k = r.standard_normal((B * S, H, NH_DH))
    v = r.standard_normal((B * S, H, NH_DH))
    u = _enc_units(r, H, signs=name == "threshold")
    if name == "ramp":
        q += np.array([11.0, 3.0, 0.0, -11.0])[i % 4][:, None, None] * u
        k += tile[:, None, None] * u
    elif name == "spike":
        q *= 8.0 * ENC_Q_SCALE / np.linalg.norm(q, axis=-1, keepdims=True)
        q = d64(f16(q))
        for b in range(B):
            for h in range(H):
                pi = b * S + r.permutation(S)
                qh = q[b * S:(b + 1) * S, h]
                k[pi, h] = ENC_SPIKE * qh / (qh * qh).sum(axis=-1, keepdims=True)
    elif name == "threshold":
        nT = -(-S // ENC_KT)
        q -= (q * u).sum(axis=-1, keepdims=True) * u
        q += (4.0 + np.where(i % 2 == 0, 0.5, -0.5) * ENC_THR_DELTA)[:, None, None] * u
        spots = (31, 32, 0, 63, 8, 55, 16, 47, 23, 40)
        for b in range(B):
            for t in range(nT):
                j = S - 1 if t == nT - 1 else t * ENC_KT + spots[t % len(spots)]
                k[b * S + j] = (8.0 + 2.0 * t) * u
    else:
        q += np.where(i % 2 == 0, 35.0, -35.0)[:, None, None] * u
        k += 32.0 * u
        q, k = d64(f16(q)), d64(f16(k))
        for b in range(B):
            for h in range(H):
                qd = q[b * S + 2 * (S // 4) + h % 2, h]
                so = k[b * S:(b + 1) * S - 1, h] @ qd
                k[(b + 1) * S - 1, h] = (so.max() + np.log2(np.exp2(so - so.max()).sum())) * qd / (qd @ qd)
    case = tuple(f16(a.reshape(B * S, d)) for a in (q, k, v))
    for a in case:
        a.setflags(write=False)
    _ENC_CASES[key] = case
    return case


def enc_rebase_coverage(name, rep, S):
    """what the case's inputs must reach, from the replay alone (conditions on the inputs, not measurements of the kernel),
    counting only decided (query, tile) pairs; asserts and returns the counts.  rep: enc_rebase_replay's dict.
      ramp       at least 1000 rebases after tile 0 in every (clip, head); every full wave mixed: on some later tile one of its 32
                 queries rebases and another does not; a largest non-rebased p above 200
      spike      every query's largest score leads the next by 20; the rebase onto it hits every in-tile position in tile 1, in
                 the middle tiles and in the last tile, where "every" is the S - 64 (nT - 1) positions that hold a key
      threshold  at least 32 pairs within 2 delta on either side of the threshold, and p above 250 on the quiet side
      offset     a final m_ref beyond 1000 of either sign, and nothing within a factor of 40 of the clamp"""
    rows, H, nT = rep["rebase"].shape
    B = rows // S
    later = np.arange(nT) > 0
    moved = rep["decided"] & rep["rebase"] & later          # decided rebases after tile 0
    quiet = rep["decided"] & ~rep["rebase"] & later         # decided tiles that keep m_ref
    per_head = moved.reshape(B, S, H, nT).sum(axis=(1, 3))
    cov = {"rebases after tile 0 per (clip, head)": int(per_head.min()), "largest non-rebased p": float(rep["p_max"].max()),
           "largest |m_ref|": float(rep["m_absmax"].max()), "undecided pairs": int((~rep["decided"]).sum()),
           "near-threshold pairs": int(rep["near"].sum())}
    if name == "ramp":
        full = S // ENC_QW                                   # full waves of a clip (a workgroup's waves start at multiples of 32)
        mv = moved.reshape(B, S, H, nT)[:, :full * ENC_QW].reshape(B, full, ENC_QW, H, nT).any(axis=2)
        qt = quiet.reshape(B, S, H, nT)[:, :full * ENC_QW].reshape(B, full, ENC_QW, H, nT).any(axis=2)
        cov["full waves"], cov["mixed full waves"] = B * full * H, int((mv & qt).any(axis=-1).sum())
        assert per_head.min() >= 1000, cov
        assert cov["mixed full waves"] == cov["full waves"], cov
        assert cov["largest non-rebased p"] > 200, cov
    elif name == "spike":
        assert rep["margin"].min() >= 20.0, float(rep["margin"].min())
        # the rebase onto the dominating key, by the tile it falls into and its position there; key S - 1 is the last live
        # position of the last tile, keys 31 and 32 are positions of every full tile
        last = S - (nT - 1) * ENC_KT
        classes = {"tile 1": ([1], ENC_KT), "middle tiles": (list(range(2, nT - 1)), ENC_KT), "last tile": ([nT - 1], last)}
        for cname, (ts, npos) in classes.items():
            for b in range(B):
                for h in range(H):
                    hit = set()
                    for t in ts:
                        sel = moved[b * S:(b + 1) * S, h, t] & (rep["top_tile"][b * S:(b + 1) * S, h] == t)
                        hit |= set(rep["pos"][b * S:(b + 1) * S, h, t][sel].tolist())
                    assert hit == set(range(npos)), (cname, b, h, sorted(set(range(npos)) - hit))
            cov[f"positions hit, {cname}"] = npos
    elif name == "threshold":
        w = 2 * ENC_THR_DELTA
        cov["decided pairs just below"] = int((quiet & (rep["gap"] > ENC_REBASE - w)).sum())
        cov["decided pairs just above"] = int((moved & (rep["gap"] < ENC_REBASE + w)).sum())
        assert cov["decided pairs just below"] >= 32 and cov["decided pairs just above"] >= 32, cov
        assert cov["largest non-rebased p"] > 250, cov
    else:
        cov["m_ref range"] = (float(rep["m_final"].min()), float(rep["m_final"].max()))
        assert rep["m_final"].min() <= -1000 and rep["m_final"].max() >= 1000, cov
        assert cov["largest |m_ref|"] < ENC_CLAMP / 40, cov
    return cov


def enc_rebase_reference(name, B, S, H=2):
    """everything a test of one case needs, computed once and shared: inputs, fp64 reference, replay, bound, mutations"""
    key = ("ref", name, B, S, H)
    if key not in _ENC_CASES:
        q, k, v = enc_rebase_case(name, B, S, H)
        ref, sabs, vstat = enc_attention(q, k, v, B, S, H)
        rep = enc_rebase_replay(q, k, S, H)
        bound = attn_bound(ref, sabs, np.full(B * S, S), vstat, p16=True, log2=True, mref=rep["m_absmax"],
                           p_floor=enc_p16_floor(q, k, v, B, S, H))
        vm = np.array(v)
        vm[:, -NH_DH:] = v[:, -2 * NH_DH:-NH_DH]
        muts = {"last key dropped": enc_attention_keys(q, k, v, B, S, H, S - 1),
                "last head reads the previous head's V": enc_attention(q, k, vm, B, S, H)[0]}
        for label, bug in ENC_BUGS.items():
            muts[label] = enc_emulate(q, k, v, B, S, H, bug=bug)
        _ENC_CASES[key] = {"q": q, "k": k, "v": v, "ref": ref, "rep": rep, "bound": bound, "mutations": muts}
    return _ENC_CASES[key]


# ---- the one-pass prefill attention (k_prefill.hip) -------------------------------------------------------------------------
PF_KB = 64            # keys per block of prefill_attn_kernel: the unit of its running maximum


def pf_natural_order(nk):
    """the V row each key's weight would meet if the V^T fragment of a 32-key k-step were read in natural order: the score
    accumulators put key 4 fq + j (j < 4) and 16 + 4 fq + j - 4 (j >= 4) of the step into k-slot 8 fq + j, and the kernel reads
    V^T in that order; read 0, 1, 2 ... instead, key j's weight multiplies the V row of its SLOT.  Rows past the last key are
    the clamped last row, as the staging leaves them.  (Keys 0 .. 3 of a step keep their place.)"""
    j = np.arange(nk)
    r = j % 32
    fq, jj = (r % 16) // 4, r % 4 + 4 * (r // 16)
    return np.minimum(j - r + 8 * fq + jj, nk - 1)


def _pf_weights(qh, kh, nvis, first):
    """scores / 8 of one (clip, head), masked to first[i] <= j < nvis[i]; returns (s, visible)"""
    j = np.arange(kh.shape[0])[None, :]
    vis = (j < nvis[:, None]) & (j >= first[:, None])
    return np.where(vis, (qh @ kh.T) / 8.0, -np.inf), vis


def prefill_attention(q, k, v, B, T, H, nk, causal, nvis=None, first=None, vperm=None, stats=True):
    """prefill_attn_kernel in fp64: T queries per clip, q [B*T][64 H], over that clip's nk keys, k / v [B*nk][64 H] (row-major;
    the cross form's head-major buffers go through head_major's inverse first); scores q.k / 8.  Query i of a clip sees keys
    first[i] <= j < nvis[i]; nvis defaults to i + 1 under the causal form and to nk otherwise, first to 0, and vperm [nk]
    (default: the identity) names the V row that key j's weight multiplies: a mask off by one, a tile that skips keys and a
    wrong key order inside a k-step are this function with a changed argument.  Computed per (clip, head); returns o
    [B*T][64 H], sabs [B*T][H] = max over the visible keys of sum_c |q_c||k_c| / 8, (vdev, pv) [B*T][H][64] = sum_j p_j |v_j - o|,
    sum_j p_j |v_j| (zeros with stats=False: a mutated reference needs o only), and the visible-key count per row [B*T]."""
    q, k, v = d64(q).reshape(B, T, H, NH_DH), d64(k).reshape(B, nk, H, NH_DH), d64(v).reshape(B, nk, H, NH_DH)
    nvis = (np.arange(T) + 1 if causal else np.full(T, nk)) if nvis is None else np.asarray(nvis)
    first = np.zeros(T, dtype=np.int64) if first is None else np.asarray(first)
    o = np.zeros((B, T, H, NH_DH))
    sabs = np.zeros((B, T, H))
    vdev, pv = np.zeros((B, T, H, NH_DH)), np.zeros((B, T, H, NH_DH))
    for b in range(B):
        for h in range(H):
            qh, kh, vh = q[b, :, h], k[b, :, h], v[b, :, h]
            s, vis = _pf_weights(qh, kh, nvis, first)
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            p /= p.sum(axis=-1, keepdims=True)
            o[b, :, h] = p @ (vh if vperm is None else vh[vperm])
            if not stats:
                continue
            sabs[b, :, h] = np.where(vis, np.abs(qh) @ np.abs(kh).T, 0).max(axis=-1) / 8.0
            pv[b, :, h] = p @ np.abs(vh)
            for i0 in range(0, T, 64):   # sum_j p_ij |v_j - o_i| in blocks of queries, over the keys any of them sees
                i1 = min(T, i0 + 64)
                j1 = int(nvis[i0:i1].max())
                vdev[b, i0:i1, h] = np.einsum("ij,ijc->ic", p[i0:i1, :j1], np.abs(vh[None, :j1] - o[b, i0:i1, h][:, None]))
    n = np.tile(nvis - first, B)
    return o.reshape(B * T, H * NH_DH), sabs.reshape(B * T, H), (vdev.reshape(B * T, H, NH_DH), pv.reshape(B * T, H, NH_DH)), n


def prefill_p16_floor(q, k, v, B, T, H, nk, causal):
    """the fp16 subnormal floor of P, per element [B*T][H][64] (prefill_bound says what it is measured against):
    sum_j min(w_j, 2^-25) a_j |v_j - o| / l over the visible keys whose weight w_j = exp(s_j - m_b), relative to the running maximum
    m_b of their 64-key block, is below 2^-14, the smallest normal fp16.  There the rounding is absolute: up to 2^-25, and never
    more than w_j itself.  a_j = exp(m_b - m) <= 1 is the later rescaling to the row's final maximum, l >= 1 the row sum."""
    q, k, v = d64(q).reshape(B, T, H, NH_DH), d64(k).reshape(B, nk, H, NH_DH), d64(v).reshape(B, nk, H, NH_DH)
    nvis = np.arange(T) + 1 if causal else np.full(T, nk)
    floor = np.zeros((B, T, H, NH_DH))
    blk = np.arange(nk) // PF_KB
    for b in range(B):
        for h in range(H):
            s, vis = _pf_weights(q[b, :, h], k[b, :, h], nvis, np.zeros(T, dtype=np.int64))
            m = s.max(axis=-1, keepdims=True)
            run = np.full_like(s, -np.inf)
            for kb in range(blk[-1] + 1):
                c = blk == kb
                prev = run[:, kb * PF_KB - 1:kb * PF_KB] if kb else np.full((T, 1), -np.inf)
                run[:, c] = np.maximum(prev, s[:, c].max(axis=-1, keepdims=True))
            w = np.where(vis, np.exp(s - run), 0.0)              # relative to the running maximum, as the kernel rounds it
            e = np.exp(s - m)
            l = e.sum(axis=-1, keepdims=True)
            o = (e / l) @ v[b, :, h]
            f = np.where(vis & (w < 2.0 ** -14), np.minimum(w, SUB16) * np.exp(run - m), 0.0) / l
            for i0 in range(0, T, 64):
                i1 = min(T, i0 + 64)
                if f[i0:i1].any():
                    floor[b, i0:i1, h] = np.einsum("ij,ijc->ic", f[i0:i1], np.abs(v[b, :, h][None] - o[i0:i1, None]))
    return floor.reshape(B * T, H, NH_DH)


def prefill_bound(o, sabs, n, vstat, floor=None):
    """attn_bound(..., p16=True) with n the row's visible keys, re-derived for prefill_attn_kernel ("Where the
    roundings sit").  Per query, in the order the kernel computes:
      scores   two chained 32-deep MFMAs into one f32 accumulator: 64 products, <= 64 u sum_c |q_c||k_c|; the division by 8 is
               exact.  The exponent (s - m) log2(e) adds 2 u |s - m| and v_exp_f32 a relative 2 u: with |s - m| <= 2 sabs that is
               inside the dot term (an MFMA chain rounds far less than 64 times) and the 4 u.  A score error e moves o by
               sum_j p_j e_j (v_j - o) to first order: 2 e sum_j p_j |v_j - o| with the second order.
      P        w_j = exp(s_j - m_b) against the RUNNING maximum m_b of the key's 64-key block, rounded to fp16: w_j (1 + eps_j),
               |eps_j| <= 2^-11 while w_j is normal; later blocks scale it by alpha <= 1 in f32 (counted under the sums).
      l        summed in f32 from the ROUNDED weights, the ones the P.V product multiplies.  Numerator and denominator then
               hold the same perturbed weights, o stays a convex combination of the V rows, and the perturbation acts like a
               score error, only exactly: o' - o = sum_j p_j eps_j (v_j - o) / (1 + sum_j p_j eps_j), at most 2^-11 (1 + 2^-10)
               sum_j p_j |v_j - o| -- a little over half of attn_bound's p16 term 2 * 2^-11 sum_j p_j |v_j - o|.  (Were l summed from the unrounded weights, as this kernel once did, the numerator alone
               would see eps: o' = o + sum_j p_j eps_j v_j, which adds o sum_j p_j eps_j, up to 2^-11 |o| that the bound has
               no term for.  An emulation of that arithmetic left the bound on a row of two keys whose V nearly agree.)
      sums     l: per lane one rounding per visible key it holds, two per later block (l alpha + ps), two shuffles; O: one
               addition per key inside the MFMAs (fp16 x fp16 products are exact in f32), one rescaling per block, then 1 / l and
               one product: at most n + 2 ceil(n / 64) + 3 roundings on any path, relative to sum_j p_j |v_j| or |o|.  That is
               <= 4 n u (pv + |o|) from n = 2 on, and everything is exact at n = 1: half of attn_bound's 8 n u (pv + |o|).
      output   rounded once: <= max(2^-11 |o|, 2^-25), where attn_bound grants the sum of the two.
      floor    the fp16 subnormal floor of P has no term of its own in attn_bound and strictly needs one: below 2^-14 the
               rounding of w_j is absolute, up to 2^-25 (never more than w_j), which moves o by `floor` = sum_j min(w_j, 2^-25)
               a_j |v_j - o| / l (prefill_p16_floor) -- at most n 2^-25 max_j |v_j - o|.  It is covered by what attn_bound grants
               beyond need: 0.99 * 2^-11 sum_j p_j |v_j - o|, the unused part of the p16 term, 4 n u (pv + |o|), the unused half
               of the sums term, and min(2^-11 |o|, 2^-25) of the output term -- on ordinary data by a wide margin, but not as a
               theorem, so with `floor` given it is ASSERTED here, element by element, from the fp64 reference alone.
    Nothing is added to the bound and nothing is fitted to the kernel's output."""
    if floor is not None:
        B, H = sabs.shape
        ao = np.abs(o).reshape(B, H, NH_DH)
        nn = np.asarray(n, dtype=np.float64).reshape(-1, 1, 1)
        spare = 0.99 * U16 * vstat[0] + 4 * nn * U32 * (vstat[1] + ao) + np.minimum(U16 * ao, SUB16)
        assert np.all(floor <= spare), (f"the fp16 subnormal floor of P needs a term of its own on this data: floor / spare up to "
                                        f"{float(np.max(floor / np.maximum(spare, 1e-300)))}")
    return attn_bound(o, sabs, n, vstat, p16=True)


def prefill_mask_mutations(q, k, v, T, H, nk, causal):
    """the two mask errors on (clip, head) units laid out as H heads of ONE clip, so that in the cross form the key past a head's
    last is the next head's key 0, as in the flat head-major buffer (the last head: its own last key once more)"""
    if causal:
        i = np.arange(T)
        return {"one key too few": prefill_attention(q, k, v, 1, T, H, nk, True, nvis=np.maximum(i, 1), stats=False)[0],
                "one key too many": prefill_attention(q, k, v, 1, T, H, nk, True, nvis=np.minimum(i + 2, T), stats=False)[0]}
    m = {}
    if nk > 1:
        m["one key too few"] = prefill_attention(q, k, v, 1, T, H, nk, False, nvis=np.full(T, nk - 1), stats=False)[0]
    if H > 1:
        k3, v3 = np.asarray(k).reshape(nk, H, NH_DH), np.asarray(v).reshape(nk, H, NH_DH)
        kx = np.concatenate([k3, np.concatenate([k3[:1, 1:], k3[-1:, -1:]], axis=1)]).reshape(nk + 1, H * NH_DH)
        vx = np.concatenate([v3, np.concatenate([v3[:1, 1:], v3[-1:, -1:]], axis=1)]).reshape(nk + 1, H * NH_DH)
        m["one key too many"] = prefill_attention(q, kx, vx, 1, T, H, nk + 1, False, stats=False)[0]
    return m


def pf_units(a, B, n, H):
    """[B*n][64 H] -> [n][B*H*64]: every (clip, head) as a head of ONE clip, in the order of the flat head-major buffer"""
    return np.ascontiguousarray(np.asarray(a).reshape(B, n, H, 64).transpose(1, 0, 2, 3)).reshape(n, B * H * 64)


def pf_from_head_major(c, B, H, S):
    """[B][H][S][64] -> [S][B*H*64] (the unit layout)"""
    return np.ascontiguousarray(c.reshape(B * H, S, 64).transpose(1, 0, 2)).reshape(S, B * H * 64)


def prefill_cross_case(r, B, T, H, S):
    """random q, K, V (head-major, exactly S keys per (clip, head)).  From S = 3 on, two planted keys per unit make both mask
    errors matter to query 0 whatever S is: the unit's last key and the key right behind it in the flat buffer (the next unit's
    key 0) each score the logsumexp of query 0's other scores, so each holds about half the weight when it is seen"""
    U = B * H
    q = f16(r.standard_normal((B * T, 64 * H)))
    ck, cv = f16(r.standard_normal((U, S, 64))), f16(r.standard_normal((U, S, 64)))
    if S >= 3:
        q0 = d64(pf_units(q, B, T, H)[0].reshape(U, 64))
        for u in range(U):
            so = d64(ck[u, 1:S - 1]) @ q0[u] / 8.0
            lse = so.max() + np.log(np.exp(so - so.max()).sum())
            loud = f16(lse * 8.0 * q0[u] / (q0[u] @ q0[u]))
            ck[u, S - 1] = loud
            if u + 1 < U:
                ck[u + 1, 0] = loud
    return q, ck.reshape(B, H, S, 64), cv.reshape(B, H, S, 64)


def prefill_cross_mutations(qu, ku, vu, B, T, H, S):
    """in the unit layout ([n][B*H*64], one clip of B*H heads)"""
    U = B * H
    m = prefill_mask_mutations(qu, ku, vu, T, U, S, False)

    def slab(shift):
        kk, vv = (np.roll(a.reshape(S, U, 64), shift, axis=1).reshape(S, U * 64) for a in (ku, vu))
        return prefill_attention(qu, kk, vv, 1, T, U, S, False, stats=False)[0]

    if H > 1:
        m["wrong head slab (kv_head): head h reads head h-1"] = slab(1)
    if B > 1:
        m["wrong clip slab (kv_clip): clip b reads clip b-1"] = slab(H)
    return m


PF_FAMILIES = ("dominant-last", "ascending", "dominant-first", "equal")


def prefill_adversarial(r, nq, nk, causal):
    """adversarial (clip, head) units for both forms of prefill_attn_kernel, one per PF_FAMILIES entry (+ a random filler unit
    in the cross form): q [U][nq][64], k, v [U][nk][64] fp16.  The queries of unit u are g_u + noise orthogonal to g_u, all on
    one half of the 64 dimensions (alternating by unit), so that a key a g_u 8 / (g_u.g_u) scores a for every query of the unit:
      equal           all keys equal: uniform weights, every P exactly 1
      ascending       key j scores 0.2 j: every 64-key block raises the maximum and rescales, and the low keys of a block sit
                      on the fp16 subnormal floor relative to it
      dominant-first  key 5 scores 40 above random rest: later blocks' P is zero in fp16 while l still counts them
      dominant-last   causal: keys 63, 64 score 40 and keys nk - 2, nk - 1 score 80: queries 63 and nk - 2 have the dominating key
                      last and an equally loud one first out of sight.  cross: key nk - 1 scores 40.
    Cross form: key 0 of unit u + 1 is the first key past unit u's last in the flat [unit][key][64] buffer.  It carries, on
    unit u's half of the dimensions, what makes it loud for unit u's queries (40 after the dominating families, 0.2 nk after
    the ascending one, 6 after the equal one) and its own role on the other half."""
    f = PF_FAMILIES
    U = len(f) + (0 if causal else 1)
    q, k = np.zeros((U, nq, 64)), r.standard_normal((U, nk, 64))
    v = r.standard_normal((U, nk, 64))
    g = np.zeros((U, 64))
    for u in range(U):
        half = slice(32 * (u % 2), 32 * (u % 2) + 32)
        g[u, half] = r.standard_normal(32)
        noise = 0.25 * r.standard_normal((nq, 32))
        noise -= np.outer(noise @ g[u, half], g[u, half]) / (g[u] @ g[u])
        q[u, :, half] = g[u, half] + noise

    def loud(u, a):
        return a * 8.0 * g[u] / (g[u] @ g[u])

    for u, fam in enumerate(f):
        if fam == "equal":
            k[u] = k[u, 0]
        elif fam == "ascending":
            k[u] = np.arange(nk)[:, None] * loud(u, 0.2)[None]
        elif fam == "dominant-first":
            k[u, min(5, nk - 1)] = loud(u, 40.0)
        elif causal:
            if nk > 65:
                k[u, 63:65] = loud(u, 40.0)
            k[u, max(nk - 2, 0):] = loud(u, 80.0)
        else:
            k[u, nk - 1] = loud(u, 40.0)
    if not causal:
        past = {"dominant-last": 40.0, "ascending": 0.2 * nk, "dominant-first": 40.0, "equal": 6.0}
        for u, fam in enumerate(f):
            half = slice(32 * (u % 2), 32 * (u % 2) + 32)
            if f[u + 1:u + 2] == ("equal",):
                k[u + 1, :, half] = loud(u, past[fam])[half]      # every key of the equal unit: they stay equal
            else:
                k[u + 1, 0, half] = loud(u, past[fam])[half]
    return f16(q), f16(k), f16(v)


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def acc_bound(absdot, K):
    """f32 accumulation of K products (MFMA chains, K-slice partials met in LDS, the bias add): at most K + 2 roundings on the
    way of any partial sum, each <= u times a partial sum <= sum |x||w|: |acc - exact| <= (K + 2) u sum_k |x_k||w_k| <= 2 K u (..)"""
    return 2.0 * K * U32 * absdot


def f16_out_bound(ref, absdot, K):
    """fp16 output of acc (+ bias): the one rounding to fp16 (2^-11 relative, subnormal floor) + the accumulation"""
    return U16 * np.abs(ref) + SUB16 + acc_bound(absdot, K)


def gelu_f16_bound(pre, absdot, K):
    """fp16(gelu(acc + bias)): |gelu'| <= 1.13 carries the accumulation error; v_exp_f32 / v_rcp_f32 (1 ulp each) and the three
    f32 products of gelu_tanh_fast are < 8 u relative to v / (1 + e), whose size is <= |v|; then the fp16 rounding of the result"""
    g = gelu(pre)
    return U16 * np.abs(g) + SUB16 + 1.13 * acc_bound(absdot, K) + 8 * U32 * np.abs(pre)


def f32_out_bound(ref, absdot, K, extra=0.0):
    """f32 output (logits, residual x += acc + bias): one more f32 rounding of the result + the accumulation"""
    return U32 * (np.abs(ref) + np.abs(extra)) + acc_bound(absdot, K)


def ln_act_bound(x, w, b):
    """|LN_f32(x) - LN(x)| per element for both LayerNorm kernels.  The row sum is a tree of depth D <= 64 (layernorm_kernel:
    20 sequential adds per lane + 6 butterfly levels; the sliced tree: 2 x 10 STEPS + 3 + 2 + 2 + 2), so the mean is off by
    dm <= 64 u mean|x| (+ u for the multiplication by 1/K); x - mean adds u|t|.  The squared sum has relative error <= 64 u +
    (dm / sigma)^2 (the first order of dm cancels, sum t = 0); inv = 1 / sqrt(var + eps) then <= half that + 3 u (add, sqrt,
    division); y = t inv g + b <= 3 u (|y| + |b|)."""
    x64 = d64(x)
    K = x64.shape[-1]
    y, inv, t = layernorm(x64, w, b)
    dm = 65 * U32 * np.abs(x64).mean(axis=-1, keepdims=True)
    var = (t * t).mean(axis=-1, keepdims=True)
    rel_inv = 0.5 * (64 * U32 + 2 * U32 + dm * dm / (var + 1e-5)) + 3 * U32
    g = np.abs(d64(w))
    return g * inv * (dm + U32 * np.abs(t)) + g * np.abs(t) * inv * rel_inv + 3 * U32 * (np.abs(y) + np.abs(d64(b))), y


def ln_f16_bound(x, w, b):
    """fp16 LayerNorm output: the f32 error above plus the one rounding to fp16"""
    e, y = ln_act_bound(x, w, b)
    return U16 * np.abs(y) + SUB16 + e, y


def attn_score_error(sabs, s_extra=0.0, mref=0.0):
    """the score error e of attn_bound, in the scores' own units (before the x ln2 of log2 scores)"""
    return 64 * U32 * sabs + s_extra + 4 * U32 + (U32 + 2.0 ** -22) * mref


def attn_bound(o, sabs, n, vstat, p16=False, s_extra=0.0, v_extra=0.0, log2=False, mref=0.0, p_floor=0.0):
    """o = sum_j p_j v_j with p = softmax(s).  Perturbing the scores by e_j moves o by sum_j p_j (e_j - sum_k p_k e_k) v_j
    = sum_j p_j e_j (v_j - o) to first order, so |do| <= e_max sum_j p_j |v_j - o| (doubled for the second order).  With
      score error  e <= 64 u sum_c|q_c||k_c| (f32 dot of 64 products) + s_extra (rounded operands) + 4 u (fast exp's argument);
                   x ln2 when the scores are log2 units (the encoder's exp2)
      mref         enc_attn_kernel subtracts its reference maximum m_ref INSIDE the score accumulator: one more k-step adds
                   hi + lo, two fp16 numbers with hi + lo = -m_ref.  hi is off by <= 2^-11 |m_ref|, lo = fp16(-m_ref - hi) by
                   2^-11 of that: a residual <= 2^-22 |m_ref|; the accumulator holds a number of size |m_ref| when the step is
                   added: one f32 rounding, u |m_ref|.  The residual is the same for every key between two rebases but differs
                   from one stretch to the next, so it does not cancel: e += (u + 2^-22) mref, mref [B][H] = the largest
                   |m_ref| the query's walk reaches (enc_rebase_replay), in the scores' units.  Not in this term: `m_ref +=
                   dlt` rounds once per rebase while O, l and the tile's scores move by dlt exactly, r u |m_ref| after r
                   rebases.  |m_ref| is a computed score, <= sabs (1 + 64 u), so all of this is <= (r + 5) u sabs, r <= 23; it
                   is granted nothing beyond the 64 u sabs of the dot (whose four MFMA k-steps round far less than 64 times)
      weights      relative error of P <= 2^-11 when P is rounded to fp16 for the matrix pipe (p16): the same first-order form.
                   (enc_attn_kernel sums l from the UNROUNDED weights, so the common part o sum_j p_j eps_j, <= 2^-11 |o|, has
                   no term here.  The sums term carries it from n >= 595 on: its own need is <= (n + 64) u on either sum (one
                   addition per key, one product per rebase, 1 / l), and sum_j p_j|v_j| >= |o|, so what it grants beyond need
                   is (7 n - 64) u (sum p|v| + |o|) >= (14 n - 128) u |o| >= 2^-11 |o|.  The product runs the kernel at n = 750
                   and 1500 only.)
      p_floor      below 2^-14, the smallest normal fp16, the rounding of a weight is absolute: up to 2^-25 per key, where
                   2^-11 relative would be less.  A kernel that rounds P for the numerator only and keeps l >= 1 (the maximum
                   of the last rebased tile has weight exactly 1) moves o by at most 2^-25 sum |v_j| over those keys:
                   p_floor [B][H][64] (enc_p16_floor), added as it stands
      sums         the online-softmax accumulations of numerator and denominator, n keys: <= 4 n u relative each, on
                   sum_j p_j |v_j| and |o|
    |o_k - o| <= 2^-11 |o| + 2^-25 (fp16 output) + (2 e + 2 2^-11 [p16]) sum_j p_j|v_j - o| + 8 n u (sum_j p_j|v_j| + |o|)
    + p_floor + v_extra.  sabs, s_extra, mref: [B][H]; vstat = (vdev, pv) [B][H][64] from the reference; o [B][H*64]."""
    vdev, pv = vstat
    B, H = sabs.shape
    e = attn_score_error(sabs, s_extra, mref)
    if log2:
        e = e * np.log(2.0)
    w = 2 * e + (2 * U16 if p16 else 0.0)
    nn = np.asarray(n, dtype=np.float64).reshape(-1, 1, 1)
    ao = np.abs(o).reshape(B, H, NH_DH)
    return (U16 * ao + SUB16 + w[:, :, None] * vdev + 8 * nn * U32 * (pv + ao) + p_floor).reshape(B, H * NH_DH) + v_extra


# ---- discrimination --------------------------------------------------------------------------------------------------------
def violation(ref, bound, mutated):
    """how far a mutated reference leaves the bound: max |mutated - ref| / bound (> 2 means a kernel with that bug fails even
    with its own error at the bound's edge)"""
    return float(np.max(np.abs(d64(mutated) - d64(ref)) / bound))


def discriminates(ref, bound, mutations):
    """every mutation must leave the bound by a factor of two; returns {name: factor}"""
    got = {name: violation(ref, bound, m) for name, m in mutations.items()}
    weak = {k: v for k, v in got.items() if not v > 2.0}
    assert not weak, f"bound too loose to catch {weak}"
    return got


def within(got, ref, bound, what):
    err = np.abs(d64(got) - d64(ref))
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / bound, 0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} outside the bound; worst at {i}: got {d64(got)[i]!r}, "
                             f"ref {d64(ref)[i]!r}, bound {bound[i]!r}")


# ---- token selection: logit_step_kernel, sample_step_kernel, lang_detect_kernel (k_token.hip) -------------------------------
# model.rs:212-277, 293-370 restated literally on fp64 PROBABILITIES.  Token outputs are discrete, so the bound becomes a
# margin: a step is *decidable* when its outcome cannot change under the kernel's arithmetic error, and the kernel must then
# match exactly; an undecidable step accepts either candidate.  The error model, per path (PATHS):
#   exp      logit_step_kernel takes e_i = __expf(l_i - m_t) against its thread's maximum m_t: the f32 subtraction (u|x|),
#            v_exp_f32's scaling of the argument by log2 e (u|x|) and v_exp_f32 itself (<= 2 u) give (2|x| + 4) u with
#            x = l_i - m <= 0 against the row maximum m.  Every merge (6 lane levels, 3 waves, 8 partials: 17 rescalings)
#            multiplies by another __expf(m_a - m_b) of error (2|m_a - m_b| + 4) u; the maxima rise monotonically, so the
#            |m_a - m_b| telescope to m - m_t <= |x|: per term (4|x| + 68) u  ->  a = 4, c = 68.  sample_step_kernel and
#            lang_detect_kernel use expf (correctly rounded to ~1 ulp) on the f32 difference: (|x| + 3) u -> a = 1, c = 3.
#   sums     all terms are positive, so a summation of depth D (roundings on the way of any partial sum) is off by <= D u
#            relative.  logit_step: <= LMAX = 32 adds per thread + 17 merges of 3 roundings (two products, one add): D = 83.
#            sample_step: ceil(V / 1024) adds per thread + block_sum (6 shuffles + 16 waves): D = ceil(V / 1024) + 22.
#            lang_detect: 4 per lane + 6 shuffles: D = 10.  The f32 CPU path (numpy softmax, pairwise sums) D = 64, and the
#            C oracle's timestamp sum is sequential: D_ts = V - no_timestamps.
#   se       eps_se = (D + c + a sum_i p_i |x_i|) u (each term's exp error weighted by its share of the sum) + V 2^-126 (terms
#            that flush to zero below 2^-126, against se >= 1)
#   p_i      expf(x_i) / se: rel(i) = eps_se + (|x_i| + 3) u (expf, the f32 difference, the division)
#   sum_ts   ts / se: eps_se + (D_ts + c + a mean_ts|x|) u + u, mean_ts weighted by the timestamps' own probabilities
# The top two allowed candidates are decided when p1 (1 - rel1) > p2 (1 + rel2), or exactly when their f32 logits are equal
# (then every path compares equal values and the tie rule alone decides); the TEXT decision when
# |sum_ts - max_text| > sum_ts rel_ts + max_text rel_text, or exactly when either side is -inf.
FIRST, SUP_TS, NON_TS, TEXT_NON_TS, TEXT_PAST = "FIRST", "SUP_TS", "NON_TS", "TEXT>NON_TS", "TEXT>PAST"
RULE_STATES = (FIRST, SUP_TS, NON_TS, TEXT_NON_TS, TEXT_PAST)
PATHS = {"logit_step": (4.0, 68.0, 83.0), "f32": (1.0, 3.0, 64.0), "lang": (1.0, 3.0, 10.0)}
NH_MAX_VOCAB = 65536
# plausible bugs the discrete references are rebuilt under (token_discriminates); each must change a decided outcome
MUTATIONS = ("nt_as_text", "last_ts_lt", "text_gt", "window_lo", "window_hi", "sup_sum_ignored", "tie_low", "cap_off",
             "max_new_off", "pos_prompt_stuck", "pos_prompt_twice", "done_touched")


def sample_path(V):
    return (1.0, 3.0, float(-(-V // 1024) + 22))


def tk_array(tk):
    """RuleTokens {sot, eot, lang, task, no_speech, no_timestamps, zero_sec, one_sec} of a vocab.SpecialTokens"""
    return np.array([tk.sot, tk.eot, tk.en, tk.transcribe, tk.no_speech, tk.no_timestamps, tk.zero_sec, tk.one_sec],
                    dtype=np.int32)


def ldl_of(V):
    return (V + 63) & ~63


def softmax64(l):
    """fp64 softmax of f32 logits; also x = l - max"""
    l = d64(l)
    x = l - l.max()
    e = np.exp(x)
    return e / e.sum(), x


def _eps_se(p, x, path, V):
    a, c, D = path[:3]
    return (D + c + a * float(p @ np.abs(x))) * U32 + V * 2.0 ** -126


def _rel(eps_se, x):
    return eps_se + (np.abs(x) + 3.0) * U32


class Step:
    """outcome of one row's step: next token (-1 = none), acceptable tokens, decided flags, rule state, log-prob"""
    __slots__ = ("state", "next", "ok", "decided", "lp", "lp_bound", "p")

    def __init__(self, state, nxt, ok, decided, lp, lp_bound, p=None):
        self.state, self.next, self.ok, self.decided, self.lp, self.lp_bound, self.p = state, nxt, ok, decided, lp, lp_bound, p


def _rule_state(tok_hist, have_last, tk, NT):
    n = len(tok_hist)
    if not have_last:
        return FIRST
    l1 = tok_hist[-1]
    if l1 > NT:
        return SUP_TS if (n >= 2 and tok_hist[-2] >= tk[1]) else NON_TS
    return "TEXT"


def _allowed(rule, V, sup, tk, last_ts, mut):
    i = np.arange(V)
    NT, zs, os_ = int(tk[5]), int(tk[6]), int(tk[7])
    past = (i > NT) & ((i < last_ts) if "last_ts_lt" in mut else (i <= last_ts))       # supress_past_timestamps (:225-243)
    if rule == FIRST:                                                                  # first_token_supress (:336-337)
        return (i >= zs + ("window_lo" in mut)) & (i <= os_ + ("window_hi" in mut))
    if rule == SUP_TS:                                                                 # suppress + supress_timestamps
        return ~sup & (i <= NT)
    if rule == NON_TS:                                                                 # suppress + supress_non_timestamps
        return ~sup & (i > NT) & ~past
    return ~sup & ~past                                                                # PAST: suppress + past timestamps


def _argmax_decide(p, l, allowed, rel, mut):
    """arg max under total_cmp (the LAST maximum wins) over the allowed set; (winner, acceptable set, decided)"""
    idx = np.nonzero(allowed)[0]
    if idx.size == 0:
        return len(p) - 1, {len(p) - 1}, True      # every entry -inf: the last index (H3), probability -inf
    pa = p[idx]
    top = pa.max()
    ties = idx[pa == top]
    w = int(ties[0] if "tie_low" in mut else ties[-1])
    if idx.size == 1:
        return w, {w}, True
    rest = np.where(idx == w, -1.0, pa)
    j = int(idx[int(np.argmax(rest))])
    if l[j] == l[w]:
        return w, {w}, True                           # an exact tie of f32 logits: the tie rule decides on every path
    decided = p[w] * (1 - rel[w]) > p[j] * (1 + rel[j])
    return w, ({w} if decided else {w, j}), bool(decided)


def step_ref(l, tok_hist, have_last, last_ts, sup, tk, path, mut=()):
    """one greedy token (model.rs:331-356) from f32 logits l [V] for a live row; returns a Step"""
    V = len(l)
    NT = int(tk[5])
    p, x = softmax64(l)
    eps = _eps_se(p, x, path, V)
    rel = _rel(eps, x)
    rule = _rule_state(tok_hist, have_last, tk, NT)
    lv = d64(l)
    if rule != "TEXT":
        w, ok, dec = _argmax_decide(p, lv, _allowed(rule, V, sup, tk, last_ts, mut), rel, mut)
        state = rule
    else:                                                                              # model.rs:263-272
        i = np.arange(V)
        ts = i > NT
        if sup[ts].any() and "sup_sum_ignored" not in mut:
            sum_ts, rel_ts = -np.inf, 0.0
        else:
            pts = p[ts]
            s = pts.sum()
            D_ts = path[2] if len(path) < 4 else path[3]
            rel_ts = eps + (D_ts + path[1] + path[0] * float(pts @ np.abs(x[ts])) / s) * U32 + U32
            sum_ts = s
        text = ((i <= NT) if "nt_as_text" in mut else (i < NT)) & ~sup
        if text.any():
            jt = int(np.nonzero(text)[0][np.argmax(p[text])])
            max_text, rel_text = p[jt], rel[jt]
        else:
            max_text, rel_text = -np.inf, 0.0
        non_ts = (sum_ts > max_text) if "text_gt" in mut else (sum_ts >= max_text)
        if np.isinf(sum_ts) or np.isinf(max_text):
            dec_rule = True
        else:
            dec_rule = abs(sum_ts - max_text) > sum_ts * rel_ts + max_text * rel_text
        outs = {}
        for r in (NON_TS, "PAST"):
            outs[r] = _argmax_decide(p, lv, _allowed(r, V, sup, tk, last_ts, mut), rel, mut)
        w, ok, dec = outs[NON_TS if non_ts else "PAST"]
        state = TEXT_NON_TS if non_ts else TEXT_PAST
        if not dec_rule:
            ok = ok | outs["PAST" if non_ts else NON_TS][1]
            dec = False
    pw = p[w] if np.nonzero(_allowed_final(state, V, sup, tk, last_ts, mut, NT))[0].size else -np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.log(pw) if pw >= 0 else np.nan
    lp_bound = rel[w] + 2.0 ** -50 if x[w] > -80 else np.inf                        # f32 p underflows below e^-87
    return Step(state, w, ok, dec, lp, lp_bound, p)


def _allowed_final(state, V, sup, tk, last_ts, mut, NT):
    r = {FIRST: FIRST, SUP_TS: SUP_TS, NON_TS: NON_TS, TEXT_NON_TS: NON_TS, TEXT_PAST: "PAST"}[state]
    return _allowed(r, V, sup, tk, last_ts, mut)


class TokenCase:
    """K launches of launch_logit_step (or sample_step) on one decode state.  logits f32 [K][B][ldl] (pad columns NaN),
    state arrays as DecodeState holds them, modes / use_pos [K], admits [n][6] = {before launch, row, t0, t1, t2, P}"""

    def __init__(self, name, V, tk, sup, logits, tokens, n_tokens, done, have_last, last_ts, ctx, cap, max_new, prompt_len,
                 modes=None, use_pos=None, pos=None, admits=(), inv_t=0.0, seed=0, clip0=0, attempt=0, labels=None):
        self.name, self.V, self.tk, self.sup = name, V, tk, sup
        self.logits = logits
        self.K, self.B = logits.shape[0], logits.shape[1]
        self.tokens, self.n_tokens, self.done = tokens, n_tokens, done
        self.have_last, self.last_ts = have_last, last_ts
        self.sum_logprob = np.zeros(self.B)
        self.no_speech = np.zeros(self.B)
        self.ctx, self.cap, self.max_new, self.prompt_len = ctx, cap, max_new, prompt_len
        self.modes = np.full(self.K, 1, np.int32) if modes is None else np.asarray(modes, np.int32)
        self.use_pos = np.zeros(self.K, np.int32) if use_pos is None else np.asarray(use_pos, np.int32)
        self.pos = pos
        self.admits = np.asarray(admits, np.int32).reshape(-1, 6)
        self.inv_t, self.seed, self.clip0, self.attempt = inv_t, seed, clip0, attempt
        self.labels = labels if labels is not None else [""] * self.B

    def state(self):
        return dict(tokens=self.tokens.copy(), n_tokens=self.n_tokens.copy(), done=self.done.copy(),
                    have_last=self.have_last.copy(), last_ts=self.last_ts.copy(), sum_logprob=self.sum_logprob.copy(),
                    no_speech=self.no_speech.copy(), pos=None if self.pos is None else self.pos.copy())


def _bookkeep(st, b, nxt, lp, tk, cap, max_new, prompt_len, mut):
    """model.rs:359-370 (+ the max_new bench knob): push next, log-prob, cap at C - 1, eot, max_new"""
    NT, eot = int(tk[5]), int(tk[1])
    n = int(st["n_tokens"][b])
    if nxt > NT:
        st["last_ts"][b] = nxt
        st["have_last"][b] = 1
    st["tokens"][b, n] = nxt
    n += 1
    st["sum_logprob"][b] += lp
    fin = 0
    if (n > cap) if "cap_off" in mut else (n >= cap):
        st["tokens"][b, n] = eot; n += 1; fin = 1
    elif nxt == eot:
        fin = 1
    elif max_new > 0 and ((n - prompt_len > max_new) if "max_new_off" in mut else (n - prompt_len >= max_new)):
        st["tokens"][b, n] = eot; n += 1; fin = 1
    st["n_tokens"][b] = n
    if fin:
        st["done"][b] = 1


def logit_step_ref(case, mut=(), path=None):
    """the fp64 reference of case's K launches.  Returns (final state, per-row info): info[b] = dict(decided = every step of
    the row decided, steps = [Step], lp_bound, ns_bound, ns_decided)"""
    path = PATHS["logit_step"] if path is None else path
    st = case.state()
    st["tokens"] = np.concatenate([st["tokens"], np.zeros((case.B, 2 * case.K + 2), np.int32)], axis=1)   # room for a mutant's overrun
    tk, P = case.tk, case.prompt_len
    info = [dict(decided=True, steps=[], lp_bound=0.0, ns_bound=0.0, ns_decided=True) for _ in range(case.B)]
    ad = [tuple(a) for a in case.admits]
    for k in range(case.K + 1):
        for a in [a for a in ad if a[0] == k]:                                        # pool_admit_kernel
            _, row, t0, t1, t2, Pa = a
            st["tokens"][row, :Pa] = [t0, t1, t2][:Pa]
            st["n_tokens"][row], st["done"][row], st["have_last"][row], st["last_ts"][row] = Pa, 0, 0, 0
            st["sum_logprob"][row] = st["no_speech"][row] = 0.0
            st["pos"][row] = 0
        if k == case.K:
            break
        pos = st["pos"] if case.use_pos[k] else None
        for b in range(case.B):
            if st["done"][b] and "done_touched" not in mut:
                continue
            mode = int(case.modes[k])
            if mode == 2:
                mp = int(pos[b])
                mode = 0 if mp == 0 else (3 if mp < P - 1 else 1)
                if mode == 3:                                                          # prompt phase: only the position
                    if "pos_prompt_stuck" not in mut:
                        pos[b] = mp + (2 if "pos_prompt_twice" in mut else 1)
                    continue
            l = case.logits[k, b, :case.V]
            if pos is not None:
                pos[b] += 1
            if mode == 0:                                                              # model.rs:293-315
                p, x = softmax64(l)
                ns = int(tk[4])
                rel = _rel(_eps_se(p, x, path, case.V), x[ns])
                st["no_speech"][b] = p[ns]
                info[b]["ns_bound"] = p[ns] * rel
                info[b]["ns_decided"] &= bool(abs(p[ns] - 0.6) > p[ns] * rel)
                if p[ns] > 0.6:
                    st["done"][b] = 2
                continue
            n = int(st["n_tokens"][b])
            s = step_ref(l, list(st["tokens"][b, :n]), int(st["have_last"][b]), int(st["last_ts"][b]), case.sup, tk, path, mut)
            info[b]["steps"].append(s)
            info[b]["decided"] &= s.decided
            info[b]["lp_bound"] += s.lp_bound
            _bookkeep(st, b, s.next, s.lp, tk, case.cap, case.max_new, P, mut)
    st["tokens"] = st["tokens"][:, :case.ctx]
    return st, info


def _philox_u(seed, clip, step, attempt):
    from oracle import oracle as O
    r0 = O.philox([step, clip, attempt, 0x6e6f726d], [seed & 0xFFFFFFFF, seed >> 32])[0]
    return (r0 >> 8) * 2.0 ** -24


def sample_ref(q, rel_q, t, u):
    """the seeded draw (include/norma_hip.h) in fp64: weights exp((q - max q) / t) over the allowed entries (q > -inf), the
    first j whose running sum exceeds u total.  Its margin: the kernel's weight w'_i = sexp((q'_i - q'max) inv_t) differs from
    w_i by eta_i relative, eta_i = q_i rel_i / t (the probabilities' error, carried by 1/t; the error of q'max shifts every
    y alike and cancels in the normalisation) + 3 u |y_i|
    (the f32 subtraction, the product, inv_t = f32(1 / t)) + 3 u (sexp's polynomial, the f32 weight); the f64 sums add
    2^-52 V.  A relative perturbation eta of the weights moves every normalised boundary F_k by <= 2 sum_i pi_i eta_i
    (pi = w / total), doubled for the second order: delta.  Returns (j, acceptable set, decided); j = -1: nothing allowed."""
    al = np.isfinite(q)
    if not al.any():
        return -1, {-1}, True
    qm = q[al].max()
    y = np.where(al, (q - qm) / t, -np.inf)
    w = np.exp(y)
    T = w.sum()
    F = np.cumsum(w) / T
    j = int(np.searchsorted(F, u, side="right"))
    j = min(j, len(q) - 1)
    eta = np.where(al, np.abs(np.where(al, q, 0)) * rel_q / t + 3 * U32 * np.abs(np.where(al, y, 0)) + 3 * U32, 0.0)
    delta = 4 * float((w / T) @ eta) + 2.0 ** -52 * len(q)
    Fprev = np.concatenate([[0.0], F[:-1]])
    ok = set(int(i) for i in np.nonzero(al & (Fprev - delta < u) & (u < F + delta))[0]) | {j}
    return j, ok, len(ok) == 1


def sample_step_ref(case, mut=()):
    """fp64 reference of K launches of launch_sample_step (t = 1 / inv_t): rules as step_ref, then the seeded draw"""
    path = sample_path(case.V)
    st = case.state()
    st["tokens"] = np.concatenate([st["tokens"], np.zeros((case.B, 2 * case.K + 2), np.int32)], axis=1)
    tk = case.tk
    t = 1.0 / float(np.float32(case.inv_t))
    info = [dict(decided=True, steps=[], lp_bound=0.0) for _ in range(case.B)]
    for k in range(case.K):
        for b in range(case.B):
            if st["done"][b] and "done_touched" not in mut:
                continue
            n = int(st["n_tokens"][b])
            l = case.logits[k, b, :case.V]
            s = step_ref(l, list(st["tokens"][b, :n]), int(st["have_last"][b]), int(st["last_ts"][b]), case.sup, tk, path, mut)
            p, x = s.p, softmax64(l)[1]
            allowed = _allowed_final(s.state, case.V, case.sup, tk, int(st["last_ts"][b]), mut, int(tk[5]))
            q = np.where(allowed, p, -np.inf)
            rel = _rel(_eps_se(p, x, path, case.V), x)
            u = _philox_u(case.seed, case.clip0 + b, n, case.attempt)
            j, ok, dec = sample_ref(q, rel, t, u)
            s.ok = ok if s.decided else (s.ok | ok)   # an undecided rule state: the draw is checked against both
            s.decided = s.decided and dec
            info[b]["steps"].append(s)
            info[b]["decided"] &= s.decided
            if j < 0:                                                                  # :343-346 push eot, stop
                st["tokens"][b, n] = tk[1]; st["n_tokens"][b] = n + 1; st["done"][b] = 1
                continue
            s.next = j
            lp = np.log(p[j])
            info[b]["lp_bound"] += rel[j] + 2.0 ** -50 if x[j] > -80 else np.inf
            _bookkeep(st, b, j, lp, tk, case.cap, case.max_new, case.prompt_len, mut)
    st["tokens"] = st["tokens"][:, :case.ctx]
    return st, info


def lang_ref(l, lang_tokens, mut=()):
    """Model::detect_language (model.rs:194-210): fp64 softmax over the language tokens' logits and the FIRST maximum;
    (probabilities, their bound, winner token, acceptable tokens, decided).  Bound: PATHS["lang"]."""
    v = d64(l)[lang_tokens]
    p, x = softmax64(v)
    rel = _rel(_eps_se(p, x, PATHS["lang"], len(v)), x)
    top = p.max()
    ties = np.nonzero(p == top)[0]
    w = int(ties[-1] if "tie_low" in mut else ties[0])     # the mutation for language: ties to the higher index
    if len(v) == 1:
        return p, p * rel, int(lang_tokens[w]), {int(lang_tokens[w])}, True
    rest = p.copy(); rest[w] = -1
    j = int(np.argmax(rest))
    if v[j] == v[w]:
        dec = True
    else:
        dec = bool(p[w] * (1 - rel[w]) > p[j] * (1 + rel[j]))
    ok = {int(lang_tokens[w])} | (set() if dec else {int(lang_tokens[j])})
    return p, p * rel, int(lang_tokens[w]), ok, dec


# ---- token-selection cases (the suite's own data: tests/test_gpu_token_ref.py runs them, tests/test_kref_cpu.py checks that
# every mutation changes a decided outcome on them) --------------------------------------------------------------------------
def small_layout(V=1000):
    """a short vocabulary with the Whisper order of specials: text, eot, sot, languages, tasks, no_speech, no_timestamps,
    then timestamps"""
    from norma_amd.vocab import SpecialTokens
    eot = V - 200
    return SpecialTokens(V, eot, eot + 1, eot + 2, eot + 42, eot + 43, eot + 46, eot + 47, eot + 48, 40)


def token_layouts():
    """(name, V, SpecialTokens, suppress list): the three Whisper vocabularies, the largest supported one and a short one"""
    from norma_amd import vocab
    out = [(n, vocab.VOCABS[n].n_vocab, vocab.VOCABS[n], vocab.default_suppress_tokens(n)) for n in ("EnV1", "V1", "V2")]
    v2 = vocab.VOCABS["V2"]
    out.append(("V2@65536", NH_MAX_VOCAB, v2, vocab.default_suppress_tokens("V2")))
    sm = small_layout()
    out.append(("small", sm.n_vocab, sm, [1, 2, 7, 8, 9, 10, 14, 25, sm.eot + 44]))
    return out


def sup_array(V, sup_list, nt, with_nt=True):
    s = np.zeros(V, dtype=np.uint8)
    s[[t for t in sup_list if 0 <= t < V]] = 1
    if with_nt:
        s[nt] = 1                         # monolingual.rs:386-395 (nh_set_tokens): suppress_tokens U {no_timestamps}
    return s


def edge_positions(V):
    """index 0, V - 1, the first and last index of each of the LSPLIT = 8 slices, and lane / wave edges inside them"""
    per = -(-V // 8)
    pos = {0, V - 1}
    for s in range(8):
        lo, hi = s * per, min(V, (s + 1) * per) - 1
        if lo >= V:
            continue
        pos |= {lo, hi} | {lo + e for e in (63, 64, 127, 128, 255, 256, 257) if lo + e <= hi}
    return sorted(pos)


def _hist(state, tk, rng, V):
    """(tokens, have_last, last_ts) of a row in a rule state"""
    NT, zs = tk.no_timestamps, tk.zero_sec
    pr = [tk.sot, tk.en, tk.transcribe]
    ts0 = int(rng.integers(zs, zs + 40))
    if state == FIRST:
        return pr, 0, 0
    if state == SUP_TS:
        return pr + [ts0], 1, ts0
    if state == NON_TS:
        ts1 = int(rng.integers(ts0 + 1, ts0 + 60))
        return pr + [ts0, 11, ts1], 1, ts1
    return pr + [ts0, 11], 1, ts0                                                      # the last token was text


def _winner_ok(state, i, tk, sup, last_ts):
    NT = tk.no_timestamps
    if state == FIRST:
        return tk.zero_sec <= i <= tk.one_sec
    if sup[i]:
        return False
    if state == SUP_TS:
        return i <= NT
    if state in (NON_TS, TEXT_NON_TS):
        return i > NT and i > last_ts
    return i < NT or i > last_ts                                                       # TEXT>PAST


def _row_logits(rng, V, ldl, tk, state, win, last_ts, sup, flat=False):
    """f32 logits [ldl] (pad columns NaN) whose allowed winner in `state` is `win` (or, when win is not allowed there, a
    decoy: the largest logit sits on win and the winner is some allowed token)"""
    NT = tk.no_timestamps
    l = np.full(ldl, np.nan, dtype=np.float32)
    bg = np.zeros(V) if flat else rng.standard_normal(V)
    if not flat:
        if state == TEXT_NON_TS:
            bg[NT + 1:] += 4.0          # timestamps carry the mass: sum_ts >= max_text
        elif state == TEXT_PAST:
            bg[NT + 1:] -= 4.0
    top = bg.max()
    if win is not None:
        if _winner_ok(state, win, tk, sup, last_ts):
            bg[win] = top + 5.0
        else:
            bg[win] = top + 7.0         # a decoy the rules must mask
    l[:V] = bg
    return l


def greedy_cases(layout, seed=0):
    """single-launch cases over every rule state x winner position, exact ties, flat logits and the special cases"""
    name, V, tk, sl = layout
    rng = np.random.default_rng(zlib_key(name, seed))
    sup = sup_array(V, sl, tk.no_timestamps)
    ldl = ldl_of(V)
    ctx = 24
    specs = []
    for state in RULE_STATES:
        for win in edge_positions(V) + [tk.zero_sec, tk.one_sec, tk.zero_sec - 1, tk.one_sec + 1, tk.no_timestamps, tk.eot]:
            specs.append((state, win, False))
        specs.append((state, None, True))                                              # flat logits
    rows = []
    for state, win, flat in specs:
        toks, hl, lt = _hist(state, tk, rng, V)
        rows.append((f"{state}@{'flat' if flat else win}", toks, hl, lt, _row_logits(rng, V, ldl, tk, state, win, lt, sup, flat)))
    # exact ties between slices and between waves of a slice: two allowed tokens share the largest logit
    per = -(-V // 8)
    for state in RULE_STATES:
        toks, hl, lt = _hist(state, tk, rng, V)
        cand = sorted({i for i in edge_positions(V) + [tk.zero_sec, tk.zero_sec + 1, tk.one_sec - 1, tk.one_sec, V - 2]
                       if _winner_ok(state, i, tk, sup, lt)})
        for a_, b_ in [(cand[0], cand[-1])] + list(zip(cand[:-1], cand[1:]))[:6]:
            l = _row_logits(rng, V, ldl, tk, state, None, lt, sup)
            l[a_] = l[b_] = np.float32(np.nanmax(l[:V]) + 5.0)
            rows.append((f"{state}@tie{a_}/{b_}", toks, hl, lt, l))
    # the special cases: a suppressed timestamp in the TEXT state forces PAST; last_ts = V - 1 in NON_TS masks everything
    for k in range(3):
        toks, hl, lt = _hist("TEXT", tk, rng, V)
        l = _row_logits(rng, V, ldl, tk, TEXT_NON_TS, None, lt, sup)
        l[100 + 7 * k] = np.nanmax(l) + 1.0     # the largest logit is text, yet the timestamps' sum would beat it
        rows.append((f"TEXT@sup_ts{k}", toks, hl, lt, l))
    rows.append(("NON_TS@all_masked", [tk.sot, tk.en, tk.transcribe, tk.zero_sec, 11, V - 1], 1, V - 1,
                 _row_logits(rng, V, ldl, tk, NON_TS, None, V - 1, sup)))
    out = []
    for B in (1, 7, 64, 96):
        take = [rows[i % len(rows)] for i in range(B)] if B < len(rows) else rows + rows[:B - len(rows)]
        if B == 1:
            take = [rows[0]]
        out.append(_pack(f"{name}/B{B}", V, tk, sup, [take], ctx, ctx - 1, 0, 3, done_every=5 if B > 1 else 0))
    rest = rows[96:]
    while rest:
        out.append(_pack(f"{name}/B96+", V, tk, sup, [rest[:96]], ctx, ctx - 1, 0, 3, done_every=7))
        rest = rest[96:]
    # the special-case rows need their own suppression (a suppressed timestamp; no_timestamps left open)
    s2 = sup.copy(); s2[tk.zero_sec + 45] = 1
    tr = [r for r in rows if r[0].startswith("TEXT@sup_ts")]
    out.append(_pack(f"{name}/sup_ts", V, tk, s2, [tr], ctx, ctx - 1, 0, 3))
    out.append(_open_nt_case(name, V, tk, sup, rng, ctx))
    return out


def zlib_key(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def _open_nt_case(name, V, tk, sup, rng, ctx):
    """no_timestamps left out of the suppression (nh_set_tokens always adds it; the kernel must not rely on that): in the
    TEXT state it is a PAST candidate but not part of max_text (model.rs:267-270 runs over i < no_timestamps)"""
    NT = tk.no_timestamps
    s = sup.copy(); s[NT] = 0
    ldl = ldl_of(V)
    rows = []
    for k in range(4):
        toks, hl, lt = _hist("TEXT", tk, rng, V)
        l = np.full(ldl, np.nan, np.float32)
        bg = rng.standard_normal(V)
        p_ts = np.log(np.exp(bg[NT + 1:]).sum())
        bg[NT] = p_ts + 1.5 + 0.3 * k          # above sum_ts: a mutant counting it as text would pick PAST
        l[:V] = bg
        rows.append((f"TEXT@open_nt{k}", toks, hl, lt, l))
    # every text token suppressed, no_timestamps open, one timestamp suppressed: sum_ts = max_text = -inf, and >= picks NON_TS
    s3 = s.copy(); s3[:NT] = 1; s3[NT + 3] = 1
    toks, hl, lt = _hist("TEXT", tk, rng, V)
    l = np.full(ldl, np.nan, np.float32)
    bg = rng.standard_normal(V); bg[NT] = bg.max() + 5
    l[:V] = bg
    c1 = _pack(f"{name}/open_nt", V, tk, s, [rows], ctx, ctx - 1, 0, 3)
    c2 = _pack(f"{name}/inf_tie", V, tk, s3, [[("TEXT@inf_tie", toks, hl, lt, l)]], ctx, ctx - 1, 0, 3)
    c1.extra = c2
    return c1


def _pack(name, V, tk, sup, launches, ctx, cap, max_new, P, done_every=0, **kw):
    """rows [(label, tokens, have_last, last_ts, logits)] per launch (the first launch's histories set the state)"""
    K, B = len(launches), len(launches[0])
    ldl = ldl_of(V)
    logits = np.stack([np.stack([r[4] for r in rows]) for rows in launches]).astype(np.float32)
    tokens = np.zeros((B, ctx), np.int32)
    n = np.zeros(B, np.int32); hl = np.zeros(B, np.int32); lt = np.zeros(B, np.int32); done = np.zeros(B, np.int32)
    for b, r in enumerate(launches[0]):
        tokens[b, :len(r[1])] = r[1]; n[b] = len(r[1]); hl[b] = r[2]; lt[b] = r[3]
        if done_every and b % done_every == done_every - 1:
            done[b] = 1
    assert logits.shape == (K, B, ldl)
    c = TokenCase(name, V, tk_array(tk), sup.astype(bool), logits, tokens, n, done, hl, lt, ctx, cap, max_new, P,
                  labels=[r[0] for r in launches[0]], **kw)
    c.extra = None
    return c


def sequence_cases(layout, seed=0):
    """K = 24 launches on a small ctx: rows reach the cap (C - 1), eot and max_new; random peaks move them through the rule
    states; mode 2 on a pool with rows admitted in mixed phases (P = 2 and 3); the no-speech probe (mode 0)"""
    name, V, tk, sl = layout
    rng = np.random.default_rng(zlib_key(name, seed, "seq"))
    sup = sup_array(V, sl, tk.no_timestamps)
    ldl = ldl_of(V)
    NT = tk.no_timestamps
    out = []

    def peak_logits(K, B, p_eot):
        L = np.full((K, B, ldl), np.nan, np.float32)
        for k in range(K):
            for b in range(B):
                bg = rng.standard_normal(V)
                r = rng.random()
                if r < p_eot:
                    bg[tk.eot] = bg.max() + 6
                elif r < 0.5:
                    bg[int(rng.integers(NT + 1, V))] = bg.max() + 6 + rng.random()
                else:
                    bg[int(rng.integers(0, tk.eot))] = bg.max() + 9 + rng.random()
                L[k, b, :V] = bg
        return L

    for max_new, p_eot in ((0, 0.0), (5, 0.0), (0, 0.06)):
        ctx, K, B = 16, 24, 7
        rows = [("SEQ", [tk.sot, tk.en, tk.transcribe], 0, 0, None) for _ in range(B)]
        c = _pack(f"{name}/seq_mn{max_new}_eot{p_eot}", V, tk, sup, [[(r[0], r[1], r[2], r[3], np.zeros(ldl, np.float32))
                                                                      for r in rows]], ctx, ctx - 1, max_new, 3, done_every=6)
        c.logits = peak_logits(K, B, p_eot); c.K = K
        c.modes = np.full(K, 1, np.int32); c.use_pos = np.ones(K, np.int32); c.pos = np.arange(B, dtype=np.int32) + 3
        out.append(c)
    for P in (2, 3):
        ctx, K, B = 16, 10, 7
        rows = [("POOL", [tk.sot, tk.en, tk.transcribe][:P], 0, 0, np.zeros(ldl, np.float32)) for _ in range(B)]
        c = _pack(f"{name}/pool_P{P}", V, tk, sup, [rows], ctx, ctx - 1, 6, P)
        c.done[:] = 1                                                                    # idle rows until admitted
        c.done[B - 1] = 0                                                                # one row already generating
        c.n_tokens[B - 1] = P + 1; c.tokens[B - 1, P] = 11
        c.logits = peak_logits(K, B, 0.0); c.K = K
        c.modes = np.full(K, 2, np.int32); c.use_pos = np.ones(K, np.int32)
        c.pos = np.full(B, 5, np.int32)
        c.admits = np.array(sorted([r % 4, r, tk.sot, tk.en if P == 3 else tk.transcribe, tk.transcribe, P]
                                   for r in range(B - 1)), np.int32)
        out.append(c)
    # the no-speech probe: p(no_speech) spread over [0.3, 0.9] around the 0.6 threshold
    B = 64
    L = np.full((1, B, ldl), np.nan, np.float32)
    for b in range(B):
        bg = rng.standard_normal(V)
        t = 0.3 + 0.6 * b / (B - 1)
        so = np.exp(np.delete(bg, tk.no_speech).astype(np.float32).astype(np.float64)).sum()
        bg[tk.no_speech] = np.log(t * so / (1 - t))
        L[0, b, :V] = bg
    rows = [("PROBE", [tk.sot, tk.en, tk.transcribe], 0, 0, L[0, b]) for b in range(B)]
    c = _pack(f"{name}/probe", V, tk, sup, [rows], 16, 15, 0, 3, done_every=9)
    c.modes = np.zeros(1, np.int32)
    c.use_pos = np.ones(1, np.int32); c.pos = np.zeros(B, np.int32)
    out.append(c)
    return out


def _sample_win(rng, V, tk, state):
    return int(rng.integers(tk.no_timestamps + 1, V)) if state == TEXT_NON_TS else int(rng.integers(0, V))


def sample_cases(layout, seed=0):
    """launch_sample_step at t in {0.2, 0.6, 1.0} in every rule state (3 launches), and everything masked"""
    name, V, tk, sl = layout
    rng = np.random.default_rng(zlib_key(name, seed, "sample"))
    sup = sup_array(V, sl, tk.no_timestamps)
    ldl = ldl_of(V)
    out = []
    for t in (0.2, 0.6, 1.0):
        rows = []
        for state in RULE_STATES:
            for k in range(10 if state == TEXT_NON_TS else 4):
                toks, hl, lt = _hist(state if not state.startswith("TEXT") else "TEXT", tk, rng, V)
                rows.append((state, toks, hl, lt, _row_logits(rng, V, ldl, tk, state, _sample_win(rng, V, tk, state), lt, sup)))
        rows.append(("NON_TS@all_masked", [tk.sot, tk.en, tk.transcribe, tk.zero_sec, 11, V - 1], 1, V - 1,
                     _row_logits(rng, V, ldl, tk, NON_TS, None, V - 1, sup)))
        c = _pack(f"{name}/sample_t{t}", V, tk, sup, [rows], 24, 23, 0, 3, done_every=8,
                  inv_t=float(np.float32(1.0) / np.float32(t)), seed=0x1234_5678_9abc + int(t * 10), clip0=3, attempt=1)
        c.logits = np.concatenate([c.logits] + [np.stack([_row_logits(rng, V, ldl, tk, r[0], _sample_win(rng, V, tk, r[0]), r[3], sup)
                                                          for r in rows])[None] for _ in range(2)])
        c.K = 3
        out.append(c)
    return out


# ---- log-mel: logmel_kernel, mel_finish_kernel (k_mel.hip) -----------------------------------------------------------------
# The kernel evaluates, per frame of 400 samples, a LINEAR map that its five tables define -- 16 leaf DFTs of length 25 over the
# samples l, l + 16, l + 32 .. and four radix-2 levels --, then |X|^2, the fold P[j] += P[400 - j], the filter sum and
# S > 1e-10 ? log10 S : -10.  The reference below evaluates the same map in fp64 on the exact f32 PCM, table and filter values;
# that the map IS the DFT (to the accuracy of the f32 tables) is a separate, derived statement (mel_matrix_bound), so the
# reference cannot share a structural mistake with the kernel unnoticed.
MEL_NFFT, MEL_HOP, MEL_BINS = 400, 160, 201
MEL_FLOOR = 1e-10
MEL_TW_OFF = (0, 25, 75, 175)          # twiddles of the levels with child length 25, 50, 100, 200
MEL_C = 44.0                           # spectrum error constant, derived in mel_bound
MEL_LOG10_ULPS = 3.0                   # device log10f, see mel_interval
MEL_UNDERFLOW = 2.0 ** -110            # see mel_bound


def mel_tables():
    """the product's tables (norma_amd/csrc/mel_host.h through the wrapper library; pure host code, no GPU): a dict of f32
    arrays hann [400], dft_cos / dft_sin [25][25], tw_cos / tw_sin [375] (tw_sin holds -sin)"""
    t = {"hann": np.zeros(400, np.float32), "dft_cos": np.zeros((25, 25), np.float32), "dft_sin": np.zeros((25, 25), np.float32),
         "tw_cos": np.zeros(375, np.float32), "tw_sin": np.zeros(375, np.float32)}
    check_rc(lib().kref_mel_tables(*(ptr(t[k]) for k in ("hann", "dft_cos", "dft_sin", "tw_cos", "tw_sin"))), "kref_mel_tables")
    return t


def mel_groups(filters):
    """the product's group scan of filters f32 [n_mel][201] -> i32 [n_mel][2] (first, last + 1 group of four bins with a tap)"""
    filters = f32(filters)
    grp = np.zeros((filters.shape[0], 2), np.int32)
    check_rc(lib().kref_mel_groups(ptr(filters), filters.shape[0], ptr(grp)), "kref_mel_groups")
    return grp


def mel_table_angles():
    """the f32 angles of the table entries, the expressions of mel_host.h restated in NumPy f32 (every step rounds to f32):
    (two_pi k) j / 25 for the leaves, (two_pi k) / n for the twiddles, (two_pi i) / 400 for the window"""
    two_pi = np.float32(np.pi) + np.float32(np.pi)
    k = np.arange(25, dtype=np.float32)
    leaf = (two_pi * k)[:, None] * k[None, :] / np.float32(25)
    tw = np.concatenate([(two_pi * np.arange(h, dtype=np.float32)) / np.float32(2 * h) for h in (25, 50, 100, 200)])
    hann = (two_pi * np.arange(400, dtype=np.float32)) / np.float32(400)
    assert leaf.dtype == tw.dtype == hann.dtype == np.float32
    return leaf, tw, hann


def mel_matrix_bound():
    """max |T - exp(-2 pi i n k / 400)| over the effective 400 x 400 matrix T of the table-defined map, derived.  Entry (k, n) of T
    is a product of five table entries: one leaf entry cos - i sin of the angle 2 pi k' j / 25 and one twiddle per level (times an
    exact sign).  An f32 angle is fl(fl(fl(two_pi k) j) / 25): three roundings, and two_pi = 2 fl(pi) carries the rounding of pi
    (|fl(pi) - pi| / pi = 2.8e-8 <= u), so |angle - theta| <= theta ((1 + u)^4 - 1) (the twiddle angles have a rounding fewer).
    cos and sin are 1-Lipschitz, so the complex entry moves by at most that; the table entry is then rounded once per component,
    <= 2^-23 each (test_kref_cpu.py checks exactly this against fp64 cos / sin of the same f32 angle): sqrt 2 * 2^-23.  With
    per-factor deviations d_i of factors of modulus <= 1 the product deviates by <= prod (1 + d_i) - 1.  theta <= 2 pi 24 24 / 25
    for the leaves and < pi for the twiddles."""
    ang = (1 + U32) ** 4 - 1
    rnd = np.sqrt(2.0) * 2.0 ** -23
    d_leaf = 2 * np.pi * 24 * 24 / 25 * ang + rnd
    d_tw = np.pi * ang + rnd
    return float((1 + d_leaf) * (1 + d_tw) ** 4 - 1)


def mel_frames(pcm, n_samples, frames):
    """the frames pcm_to_mel cuts: x[b][160 f + j], zero at and beyond n_samples[b]; pcm [B][stride] -> fp64 [B][frames][400]"""
    pcm = d64(pcm)
    B, stride = pcm.shape
    idx = MEL_HOP * np.arange(frames)[:, None] + np.arange(MEL_NFFT)[None, :]
    out = np.zeros((B, frames, MEL_NFFT))
    for b in range(B):
        ok = idx < int(n_samples[b])
        out[b][ok] = pcm[b][idx[ok]]
    return out


def mel_spectrum(xw, t, drop_leaf_term=None, tw_shift_last=0):
    """the table-defined linear map in fp64: xw [.., 400] (windowed frames) -> complex [.., 400].  Leaf l (0 .. 15) is the
    25-point DFT of xw[l + 16 j] with the table entries cos - i sin; a level of child length h turns the nodes n and n + nodes
    of the level below into node n: out[k] = e[k] + w[k] o[k], out[k + h] = e[k] - w[k] o[k], w = tw_cos + i tw_sin.
    Mutations: drop_leaf_term = j leaves sample j out of every leaf sum; tw_shift_last = s reads the last level's twiddle
    k + s (mod 200) instead of k."""
    xw = d64(xw)
    lead = xw.shape[:-1]
    W = d64(t["dft_cos"]) - 1j * d64(t["dft_sin"])                     # [k][j]
    if drop_leaf_term is not None:
        W = W.copy(); W[:, drop_leaf_term] = 0
    x = xw.reshape(lead + (25, 16))                                     # [.., j, l]
    cur = np.einsum("...jl,kj->...lk", x, W)                           # [.., 16 nodes, 25]
    tw = d64(t["tw_cos"]) + 1j * d64(t["tw_sin"])
    for lvl, h in enumerate((25, 50, 100, 200)):
        nodes = cur.shape[-2] // 2
        w = tw[MEL_TW_OFF[lvl]:MEL_TW_OFF[lvl] + h]
        if h == 200 and tw_shift_last:
            w = np.roll(w, -tw_shift_last)
        e, o = cur[..., :nodes, :], cur[..., nodes:, :]
        cur = np.concatenate([e + w * o, e - w * o], axis=-1)
    return cur[..., 0, :]


def mel_fold(P, fold=True):
    """P [.., 400] -> [.., 201]: P[j] + P[400 - j] for j in 1 .. 199 (fold=False: the mutation that omits it)"""
    out = P[..., :MEL_BINS].copy()
    if fold:
        out[..., 1:200] += P[..., :200:-1]
    return out


def mel_power_sums(frames_x, t, filters, **mut):
    """S [.., n_mel] = filters . fold(|X|^2) in fp64 of frames_x [.., 400] (unwindowed), with X, the windowed frames and the
    folded power returned as well"""
    fold = mut.pop("fold", True)
    xw = d64(frames_x) * d64(t["hann"])
    X = mel_spectrum(xw, t, **mut)
    Pf = mel_fold(X.real ** 2 + X.imag ** 2, fold)
    return Pf @ d64(filters).T, X, xw, Pf


def mel_bound(X, xw, Pf, filters, grp, c=MEL_C):
    """dS per output: how far the kernel's f32 filter sum may lie from the fp64 S.  u = 2^-24, A = sum_j |hann_j x_j| of the
    frame, g_n = n u / (1 - n u).  logmel_kernel is compiled without contraction, every operation rounds once.
      spectrum  the windowed sample is one product (1 rounding).  A leaf output is a sequential sum of 25 products: a term meets
                its product's rounding and at most 24 adds (the first add, to 0, is exact): with the window, 26 roundings, and
                the table entries have modulus <= 1 (+ 2^-23), so the complex leaf error is <= g_26 A_leaf, A_leaf the sum of
                |hann x| over the leaf's samples.  A level computes (e + w_re o_re) - w_im o_im per component: two products and
                two adds, at most 3 roundings on the way of any term, on |e| + |w_re o_re| + |w_im o_im| <= |e| + |o| per
                component, so <= sqrt 2 g_3 (|e| + |o|) as a complex number, and it passes the children's errors on with factors
                1 and |w| <= 1 + 2^-23.  |e| + |o| <= (1 + d) (A_e + A_o) with d = mel_matrix_bound, and A_e + A_o = A_node, so by
                induction the error at the root is <= (26 + 4 * 3 sqrt 2) u A = 42.97 u A to first order; the second-order
                terms (g_n against n u, the 2^-23 and d factors) are below 1e-4 relative, and c = 44 covers them:
                |X^_k - X_k| <= D = c u A.
      power     | |X^|^2 - |X|^2 | <= 2 |X| D + D^2, and re^2 + im^2 in f32 adds g_2 (|X| + D)^2: dP.
      fold      one add: dPf_j = (dP_j + dP_400-j)(1 + u) + u (P_j + P_400-j) for 1 <= j <= 199, dP_j for j = 0, 200.
      filters   sum += ((p0 f0 + p1 f1) + p2 f2) + p3 f3 over the G = g1 - g0 <= 50 groups of the filter, then the bin-200 term:
                a term meets its product, at most 3 adds inside its group, at most G adds of the running sum and the last
                add: n = G + 5 <= 55 roundings; all terms are >= 0 (checked), so the sum is off by <= g_n sum f (Pf + dPf),
                on top of sum f dPf.
      underflow an f32 result below 2^-126 may lose its low bits or be flushed: <= 2^-126 absolute per operation, < 2^10
                operations carry into one output with factors <= 2 -- MEL_UNDERFLOW = 2^-110 covers it with room to spare.
    X [.., 400] complex, xw [.., 400], Pf [.., 201] from mel_power_sums; returns dS [.., n_mel]."""
    f = d64(filters)
    assert (f >= 0).all()
    A = np.abs(xw).sum(axis=-1, keepdims=True)
    D = c * U32 * A
    aX = np.abs(X)
    g2 = 2 * U32 / (1 - 2 * U32)
    dP = 2 * aX * D + D * D + g2 * (aX + D) ** 2
    dPf = dP[..., :MEL_BINS].copy()
    dPf[..., 1:200] = (dP[..., 1:200] + dP[..., :200:-1]) * (1 + U32) + U32 * Pf[..., 1:200]
    n = (np.asarray(grp)[:, 1] - np.asarray(grp)[:, 0] + 5).astype(np.float64)
    gn = n * U32 / (1 - n * U32)
    return dPf @ f.T + gn * ((Pf + dPf) @ f.T) + MEL_UNDERFLOW


def mel_interval(S, dS):
    """[lo, hi] for the kernel's S^ > 1e-10 ? log10f(S^) : -10 given |S^ - S| <= dS: log10 max(S -+ dS, 1e-10) -+ e, no case
    excluded.  e is the error of the device log10f: the ROCm device library (OCML) documents that its f32 functions meet the
    OpenCL accuracy requirements, which allow log10 3 ulp; HIP's math API page lists 2 ulp for log10f.  The larger figure is
    taken; it is DOCUMENTED, NOT MEASURED.  An ulp of a result v is <= 2^-23 |v|.  (The kernel compares with the f32 constant
    1e-10f = 1e-10 (1 + 1.3e-8): a sum between the two gives -10 where the formula gives up to -10 + 6e-9, well inside e.)"""
    lo = np.log10(np.maximum(S - dS, MEL_FLOOR))
    hi = np.log10(np.maximum(S + dS, MEL_FLOOR))
    e = MEL_LOG10_ULPS * 2.0 ** -23 * np.maximum(np.abs(lo), np.abs(hi))
    return lo - e, hi + e


def mel_reference(pcm, n_samples, frames, t, filters, grp):
    """(lo, hi, ref) [B][n_mel][frames] (the kernel's mel32 layout) for launch_logmel_grp on pcm [B][stride]"""
    S, X, xw, Pf = mel_power_sums(mel_frames(pcm, n_samples, frames), t, filters)
    dS = mel_bound(X, xw, Pf, filters, grp)
    lo, hi = mel_interval(S, dS)
    tr = lambda a: np.ascontiguousarray(np.swapaxes(a, -1, -2))
    return tr(lo), tr(hi), tr(np.log10(np.maximum(S, MEL_FLOOR)))


def mel_inside(got, lo, hi, what, ref=None):
    """every value finite and inside its interval; returns the largest |got - ref| / half-width (a measurement; ref defaults to
    the interval's middle)"""
    g = d64(got)
    bad = ~(np.isfinite(g) & (g >= lo) & (g <= hi))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} outside their interval; first at {i}: got {g[i]!r}, "
                             f"interval [{lo[i]!r}, {hi[i]!r}]")
    return float(np.max(np.abs(g - (0.5 * (lo + hi) if ref is None else ref)) / (0.5 * (hi - lo))))


def mel_emulate_f32(frames_x, t, filters, grp):
    """NumPy f32 emulation of logmel_kernel's arithmetic, operation for operation and in its order (every NumPy f32 operation
    rounds once, as the uncontracted kernel does): frames_x f32 [F][400] -> (X^ complex64-as-two-f32 [F][400][2], S^ f32
    [F][n_mel]).  The CPU check that the bound is sound; it is not the reference."""
    x = f32(frames_x)
    F = x.shape[0]
    s_in = t["hann"][None, :] * x
    c, s = t["dft_cos"], t["dft_sin"]
    xin = s_in.reshape(F, 25, 16)                                        # [F][j][leaf]
    re = np.zeros((F, 16, 25), np.float32); im = np.zeros((F, 16, 25), np.float32)
    for j in range(25):
        v = xin[:, j, :, None]                                           # [F][leaf][1]
        re = re + v * c[None, None, :, j]
        im = im - v * s[None, None, :, j]
    for lvl, h in enumerate((25, 50, 100, 200)):
        nodes = re.shape[1] // 2
        wr = t["tw_cos"][MEL_TW_OFF[lvl]:MEL_TW_OFF[lvl] + h]
        wi = t["tw_sin"][MEL_TW_OFF[lvl]:MEL_TW_OFF[lvl] + h]
        er, ei, orr, oi = re[:, :nodes], im[:, :nodes], re[:, nodes:], im[:, nodes:]
        re = np.concatenate([er + wr * orr - wi * oi, er - wr * orr + wi * oi], axis=-1)
        im = np.concatenate([ei + wr * oi + wi * orr, ei - wr * oi - wi * orr], axis=-1)
    re, im = re[:, 0], im[:, 0]
    pw = re * re + im * im
    pf = pw[:, :MEL_BINS].copy()
    pf[:, 1:200] = pw[:, 1:200] + pw[:, :200:-1]
    f = f32(filters)
    S = np.zeros((F, f.shape[0]), np.float32)
    for m in range(f.shape[0]):
        acc = np.zeros(F, np.float32)
        for g in range(int(grp[m][0]), int(grp[m][1])):
            k = 4 * g
            acc = acc + (pf[:, k] * f[m, k] + pf[:, k + 1] * f[m, k + 1] + pf[:, k + 2] * f[m, k + 2] + pf[:, k + 3] * f[m, k + 3])
        S[:, m] = acc + pf[:, 200] * f[m, 200]
    assert S.dtype == re.dtype == np.float32
    return np.stack([re, im], axis=-1), S


def mel_log_f32(S):
    """S^ > 1e-10f ? log10f(S^) : -10 in NumPy f32 (its log10 stands in for the device's within the 3 ulp of mel_interval)"""
    S = f32(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(S > np.float32(1e-10), np.log10(np.maximum(S, np.float32(1e-30))), np.float32(-10.0)).astype(np.float32)


def mel_impulse_expected(offsets, t, filters):
    """a frame whose only non-zero sample is a 1 at offset o: the exact DFT has |X_k| = hann_o for every k, so
    S_m = hann_o^2 sum_k w_k f[m][k] with w = 2 for the folded bins 1 .. 199 and 1 for bins 0 and 200 -- no FFT involved.
    The table-defined map has |T| within d = mel_matrix_bound of 1, so S is off by <= (1 + d)^2 - 1 relative; the kernel adds
    only zeros in its accumulations: one rounding in the leaf product, per level two products and an add on the one non-zero
    child (<= 3 sqrt 2 u as a complex number), so |X^|^2 carries <= 2 (1 + 12 sqrt 2) u < 36 u; power 2 u, fold u, and the
    filter sum its g_n <= 55 u: 100 u covers them.  Returns (S, dS) [len(offsets)][n_mel]."""
    f = d64(filters)
    w = np.full(MEL_BINS, 2.0); w[0] = w[200] = 1.0
    S = (d64(t["hann"])[np.asarray(offsets)] ** 2)[:, None] * (f @ w)[None, :]
    rel = (1 + mel_matrix_bound()) ** 2 - 1 + 100 * U32
    return S, rel * S + MEL_UNDERFLOW


def f32_ordered(v):
    """the order-preserving u32 encoding of an f32 that logmel_kernel feeds to atomicMax (k_mel.hip f32_ordered)"""
    u = f32(v).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def logmel(pcm, n_samples, frames, t, filters, grp, mel32=None, mel_off=0, chunk_max=None, cm_off=0):
    """one launch_logmel_grp through the wrapper library; mel32 / chunk_max default to fresh buffers of exactly the window
    (mel32 NaN-filled, chunk_max zero as the product's memset leaves it).  Returns (mel32, chunk_max) as given, written."""
    pcm, filters = f32(pcm), f32(filters)
    B, stride = pcm.shape
    n_mel = filters.shape[0]
    ns = np.ascontiguousarray(n_samples, dtype=np.int32)
    grp = np.ascontiguousarray(grp, dtype=np.int32)
    if mel32 is None:
        mel32 = np.full(B * n_mel * frames, np.nan, np.float32)
    if chunk_max is None:
        chunk_max = np.zeros(B, np.uint32)
    rc = lib().kref_logmel(ptr(pcm), stride, ptr(ns), B, ptr(t["hann"]), ptr(t["dft_cos"]), ptr(t["dft_sin"]), ptr(t["tw_cos"]),
                           ptr(t["tw_sin"]), ptr(filters), ptr(grp), n_mel, frames, ptr(mel32), mel_off, mel32.size, ptr(chunk_max),
                           cm_off, chunk_max.size)
    check_rc(rc, f"launch_logmel_grp B={B} n_mel={n_mel} frames={frames}")
    return mel32, chunk_max


def mel_finish(mel32, mel_off, chunk_max, cm_off, img, img_off, B, n_mel, frames, normalise):
    """one launch_mel_finish_ex through the wrapper library on windows of the three buffers (written in place)"""
    rc = lib().kref_mel_finish(ptr(mel32), mel_off, mel32.size, ptr(chunk_max), cm_off, chunk_max.size, ptr(img), img_off, img.size,
                               B, n_mel, frames, int(normalise))
    check_rc(rc, f"launch_mel_finish_ex B={B} n_mel={n_mel} frames={frames} normalise={normalise}")


# the signal families of tests/test_gpu_mel_ref.py; tests/test_kref_cpu.py runs the f32 emulation over the same data
MEL_FRAMES = (1, 15, 16, 17, 33)        # a lone wave, dead waves (frames % 16 != 0), a full workgroup, one and two workgroups more
MEL_FAMILIES = ("noise-0.1", "noise-3e-4", "burst", "dc", "square")
MEL_BROADBAND = ("noise-0.1", "noise-3e-4")
MEL_CANARY = 1.0e4                      # what the samples at and beyond n_samples hold: a read past the length shows


def mel_full_length(frames):
    return (frames - 1) * MEL_HOP + MEL_NFFT


def mel_ragged_lengths(frames, B):
    """n_samples of the ragged noise case: B = 1 the full clip; B = 3 the full clip, 16 * 160 + 1 (one sample into frame 16) and
    399 (frame 0 one sample short); B = 4 those and a length that ends inside the last live frame"""
    full = mel_full_length(frames)
    return [full, 16 * MEL_HOP + 1, 399, full - 200][:B]


def mel_case(family, frames, B, seed=0):
    """(pcm f32 [B][stride], n_samples i32 [B]) of one family; stride exceeds the longest clip, and every sample at or beyond a
    clip's n_samples holds MEL_CANARY"""
    rng = np.random.default_rng(zlib_key("mel", family, frames, B, seed))
    full = mel_full_length(frames)
    stride = max(full, 16 * MEL_HOP + 1) + 67
    ns = np.full(B, full, dtype=np.int32)
    i = np.arange(stride)
    if family == "noise-0.1":
        pcm = 0.1 * rng.standard_normal((B, stride))
        ns = np.asarray(mel_ragged_lengths(frames, B), dtype=np.int32)
    elif family == "noise-3e-4":
        pcm = 3e-4 * rng.standard_normal((B, stride))
    elif family == "burst":            # a 0.5 tone over the first frame, then noise 94 dB below it
        pcm = 1e-5 * rng.standard_normal((B, stride))
        pcm[:, :MEL_NFFT] = 0.5 * np.sin(2 * np.pi * (440.0 + 300.0 * np.arange(B)[:, None]) * i[None, :MEL_NFFT] / 16000.0)
    elif family == "dc":
        pcm = np.full((B, stride), 0.7)
    elif family == "square":           # full scale, period 50 + 14 b samples
        pcm = np.stack([np.where((i // (25 + 7 * b)) % 2 == 0, 1.0, -1.0) for b in range(B)])
    else:
        raise ValueError(family)
    pcm = f32(pcm)
    for b in range(B):
        pcm[b, ns[b]:] = MEL_CANARY
    return pcm, ns
