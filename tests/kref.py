"""Kernel-level fp64 references for the launchers of norma_amd/csrc/nh_kernels.h, their error bounds, and the loader of
tools/bin/libnh_kref.so (tools/kref.hip: C entry points onto the shipped launchers).

Every reference is plain NumPy in float64 on the exact fp16 / f32 values the kernel was given.  Every bound is a formula
derived from the kernel's arithmetic (the comments say how), never a constant fitted to what the GPU produced.  u = 2^-24 is the
unit roundoff of f32, 2^-11 that of fp16.  A test also shows that its bound is tight enough to matter: `discriminates` rebuilds
the reference under plausible bugs (a dropped k-step, a missing bias tile, a key too few ...) and requires each of them to leave
the bound by a factor of two on the case's own data, so that a kernel with that bug would fail the case."""
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
EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_CONV2_F32 = 0, 1, 2, 3
WRAPPERS = ["kref_skinny", "kref_skinny_ln_supported", "kref_dec_attention", "kref_xabs_attention", "kref_enc_attention",
            "kref_gemm", "kref_layernorm", "kref_embed"]

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
    L.kref_dec_attention.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, i, vp]
    L.kref_xabs_attention.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp, i]
    L.kref_enc_attention.argtypes = [vp, vp, l, vp, vp, l, i, i, i]
    L.kref_gemm.argtypes = [i, vp, z, l, i, l, vp, vp, i, i, i, i, vp, vp, vp, z, i, l, i, l, l, i, i, f, i, i, vp]
    L.kref_layernorm.argtypes = [i, vp, vp, vp, vp, vp, i, i]
    L.kref_embed.argtypes = [vp, i, vp, i, vp, i, vp, i, i, i, vp, i]
    return L


def lib():
    L = load()
    if L.kref_skinny.argtypes is None:
        _argtypes()
    return L


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


def attn_bound(o, sabs, n, vstat, p16=False, s_extra=0.0, v_extra=0.0, log2=False):
    """o = sum_j p_j v_j with p = softmax(s).  Perturbing the scores by e_j moves o by sum_j p_j (e_j - sum_k p_k e_k) v_j
    = sum_j p_j e_j (v_j - o) to first order, so |do| <= e_max sum_j p_j |v_j - o| (doubled for the second order).  With
      score error  e <= 64 u sum_c|q_c||k_c| (f32 dot of 64 products) + s_extra (rounded operands) + 4 u (fast exp's argument);
                   x ln2 when the scores are log2 units (the encoder's exp2)
      weights      relative error of P <= 2^-11 when P is rounded to fp16 for the matrix pipe (p16): the same first-order form
      sums         the online-softmax accumulations of numerator and denominator, n keys: <= 4 n u relative each, on
                   sum_j p_j |v_j| and |o|
    |o_k - o| <= 2^-11 |o| + 2^-25 (fp16 output) + (2 e + 2 2^-11 [p16]) sum_j p_j|v_j - o| + 8 n u (sum_j p_j|v_j| + |o|)
    + v_extra.  sabs, s_extra: [B][H]; vstat = (vdev, pv) [B][H][64] from the reference; o [B][H*64]."""
    vdev, pv = vstat
    B, H = sabs.shape
    e = 64 * U32 * sabs + s_extra + 4 * U32
    if log2:
        e = e * np.log(2.0)
    w = 2 * e + (2 * U16 if p16 else 0.0)
    nn = np.asarray(n, dtype=np.float64).reshape(-1, 1, 1)
    ao = np.abs(o).reshape(B, H, NH_DH)
    return (U16 * ao + SUB16 + w[:, :, None] * vdev + 8 * nn * U32 * (pv + ao)).reshape(B, H * NH_DH) + v_extra


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
