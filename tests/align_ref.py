"""NumPy references for token-level timestamps (nh_align, include/norma_hip.h; kernels in norma_amd/csrc/k_align.hip), their
error bounds, and the ctypes signatures of the kref_align_* entry points of tools/kref.hip.

Stages 2 - 5 (weights, z-score, median, mean over heads) are float64 on the exact fp16 / f32 inputs; stage 6 (DTW) is float32
with the recurrence exactly as the contract writes it, so its path is compared for integer equality.  `chain` is a float64
Whisper decoder built from kref's blocks: for a token prefix and an encoder output it returns every layer's cross-attention q
and K -- what the weights are made of -- optionally with every activation rounded to fp16 where the GPU path stores fp16.
Every bound is derived from the kernels' arithmetic (the docstrings say how); u = 2^-24."""
import ctypes as C

import numpy as np

import kref as K
from kref import U32, d64

DH = 64


# ---- stage 2: weights -------------------------------------------------------------------------------------------------------
def weights(q, k, nk, scale=0.125):
    """softmax over s < nk of q . k_s * scale: q [n][64], k [S][64] (fp16 values) -> (W [n][nk], sabs [n] = max_s sum_c |q_c||k_c|
    * scale, x [n][nk] = score - row maximum)"""
    q, k = d64(q), d64(k)[:nk]
    s = (q @ k.T) * scale
    x = s - s.max(axis=1, keepdims=True)
    e = np.exp(x)
    sabs = (np.abs(q) @ np.abs(k).T).max(axis=1) * scale
    return e / e.sum(axis=1, keepdims=True), sabs, x


def weights_bound(W, sabs, x):
    """|W_gpu - W| for align_weights_kernel.  score: two chained MFMAs accumulate the 64 products in f32, kref.acc_bound's
    2 K u sum|q||k| (the * 1/8 is exact): E.  The kernel's row maximum carries the same error, so the exponent's argument
    x = s - m is off by 2 E + u |x| (the subtraction), the product with log2(e) adds 2 u |x| (the constant, the product) and
    v_exp_f32 one ulp: e_i has relative error 2 E + (3 |x_i| + 2) u.  The sum of the (positive) terms: <= 24 adds per lane,
    4 shuffle levels, 3 adds across the waves: 31 u relative, on top of the terms' own errors weighted by their share
    (sum_j p_j (3 |x_j| + 2) u + 2 E).  The division: u.  Doubled E for the second order of the two exponent errors' product
    is below the rounding of this formula (E ~ 1e-6).  Terms below 2^-126 flush to zero: + 2^-126 absolute."""
    E = K.acc_bound(sabs, 64)[:, None]
    ax = np.abs(x)
    rel = 4 * E + (3 * ax + 3 * (W * ax).sum(axis=1, keepdims=True) + 36) * U32
    return W * rel + 2.0 ** -126


# ---- stages 3 - 5: z-score, median of 7, mean over the heads ----------------------------------------------------------------
def zscore(W, ddof=0):
    """(W - mean) / std over axis -2 (the rows), population std; std == 0 -> 0.  W [..][n][nk]"""
    W = d64(W)
    n = W.shape[-2]
    mean = W.mean(axis=-2, keepdims=True)
    t = W - mean
    var = (t * t).sum(axis=-2, keepdims=True) / max(n - ddof, 1)
    sd = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd == 0, 0.0, t / np.where(sd == 0, 1.0, sd))
    return z, mean, sd


def reflect_index(j, nk):
    j = np.where(j < 0, -j, j)
    return np.where(j >= nk, 2 * (nk - 1) - j, j)


def window_index(nk, width=7, edge=False):
    """[nk][width] key indices of the filter window: reflect padding without repeating the edge (edge=True: the mutation that
    repeats it)"""
    j = np.arange(nk)[:, None] + np.arange(width)[None, :] - width // 2
    return np.clip(j, 0, nk - 1) if edge else reflect_index(j, nk)


def median_filter(z, width=7, edge=False):
    """median of `width` along the last axis with reflect padding; nk <= width // 2 (3 for width 7) is left unfiltered"""
    nk = z.shape[-1]
    if nk <= 3:
        return np.array(z, copy=True)
    z = np.asarray(z)
    win = z[..., window_index(nk, width, edge)]          # [..][nk][width]
    return np.sort(win, axis=-1)[..., width // 2]


def matrix(W, P, ddof=0, width=7, edge=False, heads=None):
    """stages 3 - 5 on W [A][n - 1][nk] -> M [n - P][nk]"""
    z, _, _ = zscore(W, ddof)
    f = median_filter(z, width, edge)
    if heads is not None:
        f = f[heads]
    return f.mean(axis=0)[P - 1:]


def matrix_bound(W, P):
    """|M_gpu - M| for align_stats_kernel + align_reduce_kernel on f32 W [A][N][nk] (N rows).
    mean: N sequential f32 adds of non-negative terms and one division: dm <= (N + 1) u mean.  t = w - mean: dm + u |t|.
    The squared sum: its first-order dependence on dm cancels (sum t = 0), leaving (dm / sd)^2 relative, plus N + 2 roundings
    of the fused sum and 2 u per square: rel_var <= (N + 6) u + (dm / sd)^2; sd = sqrt(var / N): half of it + 2 u.
    z = t / sd: (dm + u |t|) / sd -- the 1 / std factor -- + |z| (rel_sd + u).
    The median is 1-Lipschitz in the sup norm: its error is at most the largest z error in its window, nothing is added.
    The mean over A heads: A adds and a division, (A + 1) u sum_a |med_a| / A."""
    W = d64(W)
    A, N, nk = W.shape
    z, mean, sd = zscore(W)
    dm = (N + 1) * U32 * np.abs(mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        isd = np.where(sd == 0, 0.0, 1.0 / np.where(sd == 0, 1.0, sd))
    rel_sd = 0.5 * ((N + 6) * U32 + (dm * isd) ** 2) + 2 * U32
    ez = (dm + U32 * np.abs(W - mean)) * isd + np.abs(z) * (rel_sd + U32)
    if nk > 3:
        ez = ez[..., window_index(nk)].max(axis=-1)
    med = median_filter(z)
    return (ez.mean(axis=0) + (A + 1) * U32 * np.abs(med).mean(axis=0))[P - 1:] + 2.0 ** -126


# ---- stage 6: DTW in float32 ------------------------------------------------------------------------------------------------
def dtw(M):
    """the contract's recurrence on x = -M (f32), row by row.  Returns (first [R], last [R], end cost)"""
    x = -np.asarray(M, dtype=np.float32)
    R, nk = x.shape
    inf = np.float32(np.inf)
    cost = np.full((R + 1, nk + 1), inf, dtype=np.float32)
    trace = np.full((R + 1, nk + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    trace[0, :] = 2
    trace[:, 0] = 1
    for i in range(1, R + 1):
        ci, cp, ti, xi = cost[i], cost[i - 1], trace[i], x[i - 1]
        for j in range(1, nk + 1):
            c0, c1, c2 = cp[j - 1], cp[j], ci[j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            ci[j] = xi[j - 1] + c
            ti[j] = t
    first, last = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    i, j = R, nk
    while i >= 1 and j >= 1:
        if last[i - 1] < 0:
            last[i - 1] = j - 1
        first[i - 1] = j - 1
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return first, last, cost[R, nk]


def dtw_diagonals(M):
    """the same recurrence evaluated along anti-diagonals with NumPy vectors (every cell is still one f32 add of the same
    operands, so cost, trace and path are those of dtw; tests/test_align_cpu.py checks that): for the full-size case"""
    x = -np.asarray(M, dtype=np.float32)
    R, nk = x.shape
    cost = np.full((R + 1, nk + 1), np.inf, dtype=np.float32)
    trace = np.zeros((R + 1, nk + 1), dtype=np.int8)
    cost[0, 0] = 0
    for k in range(2, R + nk + 1):
        i = np.arange(max(1, k - nk), min(R, k - 1) + 1)
        j = k - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t0 = (c0 < c1) & (c0 < c2)
        t1 = ~t0 & (c1 < c0) & (c1 < c2)
        cost[i, j] = x[i - 1, j - 1] + np.where(t0, c0, np.where(t1, c1, c2))
        trace[i, j] = np.where(t0, 0, np.where(t1, 1, 2))
    first, last = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    i, j = R, nk
    while i >= 1 and j >= 1:
        if last[i - 1] < 0:
            last[i - 1] = j - 1
        first[i - 1] = j - 1
        t = trace[i, j]
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    return first, last, cost[R, nk]


def planted_path(R, nk, rng):
    """a matrix whose DTW path is known by construction: a random monotone path from (0, 0) to (R - 1, nk - 1) holds 10, every
    other cell -1 -- leaving the path costs at least 1 per cell and gains nothing.  Returns (M f32, first, last)"""
    M = np.full((R, nk), -1.0, dtype=np.float32)
    i = j = 0
    first, last = np.full(R, -1, np.int32), np.full(R, -1, np.int32)
    while True:
        M[i, j] = 10.0
        if first[i] < 0:
            first[i] = j
        last[i] = j
        if i == R - 1 and j == nk - 1:
            return M, first, last
        moves = [(1, 1)] * (i + 1 < R and j + 1 < nk) + [(1, 0)] * (i + 1 < R) + [(0, 1)] * (j + 1 < nk)
        # steer towards the corner so that neither axis runs out early
        want_i, want_j = (R - 1 - i), (nk - 1 - j)
        wts = np.array([1.0 + min(want_i, want_j) if m == (1, 1) else 1.0 + (want_i if m == (1, 0) else want_j) for m in moves])
        di, dj = moves[int(rng.choice(len(moves), p=wts / wts.sum()))]
        i, j = i + di, j + dj


def dtw_brute(M):
    """least cost over ALL monotone paths (0, 0) -> (R - 1, nk - 1) with steps (1, 1), (1, 0), (0, 1), in float64"""
    x = -d64(M)
    R, nk = x.shape
    best = np.inf

    def walk(i, j, c):
        nonlocal best
        c += x[i, j]
        if i == R - 1 and j == nk - 1:
            best = min(best, c)
            return
        if i + 1 < R and j + 1 < nk:
            walk(i + 1, j + 1, c)
        if i + 1 < R:
            walk(i + 1, j, c)
        if j + 1 < nk:
            walk(i, j + 1, c)
    walk(0, 0, 0.0)
    return best


# ---- the decoder chain ------------------------------------------------------------------------------------------------------
def r16(a, on):
    return d64(K.f16(a)) if on else a


def _attend(q, k, v, H, nvis):
    """one query row per position through kref.dec_attention: q [T][d], k / v [Tk][d], nvis [T] visible keys"""
    T = q.shape[0]
    kb = np.broadcast_to(k[None], (T,) + k.shape)
    vb = np.broadcast_to(v[None], (T,) + v.shape)
    return K.dec_attention(q, kb, vb, H, nvis)[0]


def chain(cfg, wts, tokens, xa, rounded=False, layers=None):
    """float64 TextDecoder::forward over the prefix `tokens` against the encoder output xa [S][d] (f32 values).
    wts: {HF name: array of fp16-representable values}.  rounded: every activation is rounded to fp16 where the GPU path stores
    fp16 -- the encoder output (xa16), LayerNorm outputs, q / k / v, both K/V caches, attention outputs, the GELU hidden.
    Returns dict(hidden [T][d] after the final LayerNorm, q [L][T][d] the cross-attention queries, k [L][S][d] the cross K)."""
    d, H = cfg.d_model, cfg.decoder_attention_heads
    L = cfg.decoder_layers if layers is None else layers
    tokens = np.asarray(tokens)
    T = len(tokens)
    w = lambda n: d64(wts[n])
    x = w("model.decoder.embed_tokens.weight")[tokens] + w("model.decoder.embed_positions.weight")[:T]
    xa = r16(d64(xa), rounded)
    qs, ks = [], []
    for l in range(L):
        p = f"model.decoder.layers.{l}"
        sa, ca = p + ".self_attn", p + ".encoder_attn"
        h = r16(K.layernorm(x, w(p + ".self_attn_layer_norm.weight"), w(p + ".self_attn_layer_norm.bias"))[0], rounded)
        q = r16(K.linear(h, w(sa + ".q_proj.weight"), w(sa + ".q_proj.bias"))[0], rounded)
        k = r16(K.linear(h, w(sa + ".k_proj.weight"))[0], rounded)
        v = r16(K.linear(h, w(sa + ".v_proj.weight"), w(sa + ".v_proj.bias"))[0], rounded)
        att = r16(_attend(q, k, v, H, np.arange(T) + 1), rounded)
        x = x + K.linear(att, w(sa + ".out_proj.weight"), w(sa + ".out_proj.bias"))[0]
        h = r16(K.layernorm(x, w(p + ".encoder_attn_layer_norm.weight"), w(p + ".encoder_attn_layer_norm.bias"))[0], rounded)
        cq = r16(K.linear(h, w(ca + ".q_proj.weight"), w(ca + ".q_proj.bias"))[0], rounded)
        ck = r16(K.linear(xa, w(ca + ".k_proj.weight"))[0], rounded)
        cv = r16(K.linear(xa, w(ca + ".v_proj.weight"), w(ca + ".v_proj.bias"))[0], rounded)
        qs.append(cq)
        ks.append(ck)
        att = r16(_attend(cq, ck, cv, H, np.full(T, xa.shape[0])), rounded)
        x = x + K.linear(att, w(ca + ".out_proj.weight"), w(ca + ".out_proj.bias"))[0]
        h = r16(K.layernorm(x, w(p + ".final_layer_norm.weight"), w(p + ".final_layer_norm.bias"))[0], rounded)
        hid = r16(K.gelu(K.linear(h, w(p + ".fc1.weight"), w(p + ".fc1.bias"))[0]), rounded)
        x = x + K.linear(hid, w(p + ".fc2.weight"), w(p + ".fc2.bias"))[0]
    hidden = K.layernorm(x, w("model.decoder.layer_norm.weight"), w("model.decoder.layer_norm.bias"))[0]
    return dict(hidden=hidden, q=np.stack(qs), k=np.stack(ks))


def chain_weights(out, layer, head, nk, rows=None):
    """W [n - 1][nk] of head (layer, head) from a chain result; rows: the query positions (default: all)"""
    c = slice(head * DH, (head + 1) * DH)
    q = out["q"][layer][:, c]
    if rows is not None:
        q = q[rows]
    return weights(q, out["k"][layer][:, c], nk)[0]


def decoder_weights(cfg, seed=0, overrides=None):
    """{name: f32 array} of every decoder tensor of the synthetic checkpoint"""
    from norma_amd import synth
    return {n: a for n, a in synth.synth_weights(cfg, seed, overrides) if n.startswith("model.decoder.")}


# ---- the kref_align_* entry points (tools/kref.hip) -------------------------------------------------------------------------
def lib():
    L = K.lib()
    if L.kref_align_weights.argtypes is None:
        vp, i = C.c_void_p, C.c_int
        for n in ("kref_align_weights", "kref_align_reduce", "kref_align_dtw"):
            getattr(L, n).restype = C.c_int
        L.kref_align_weights.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, i, vp]
        L.kref_align_reduce.argtypes = [vp, i, i, i, i, vp, vp, i, vp]
        L.kref_align_dtw.argtypes = [vp, i, i, i, vp, vp, i, vp, vp, i]
    return L


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def gpu_weights(q, k, heads, n_rows, n_keys, fill=np.nan):
    """q fp16 [A][max_rows][B][64], k fp16 [B][H][S][64] -> W f32 [B][A][max_rows][S], pre-filled with `fill`"""
    A, max_rows, B, _ = q.shape
    H, S = k.shape[1], k.shape[2]
    W = np.full((B, A, max_rows, S), fill, dtype=np.float32)
    q, k, heads, n_rows, n_keys = K.f16(q), K.f16(k), i32(heads), i32(n_rows), i32(n_keys)   # named: alive across the call
    rc = lib().kref_align_weights(K.ptr(q), K.ptr(k), K.ptr(heads), A, H, S, B, K.ptr(n_rows), K.ptr(n_keys), max_rows, K.ptr(W))
    K.check_rc(rc, "kref_align_weights")
    return W


def gpu_reduce(W, n_rows, n_keys, P, fill=np.nan):
    """W f32 [B][A][max_rows][S] -> M f32 [B][max_rows][S], pre-filled with `fill`"""
    B, A, max_rows, S = W.shape
    M = np.full((B, max_rows, S), fill, dtype=np.float32)
    W, n_rows, n_keys = K.f32(W), i32(n_rows), i32(n_keys)
    rc = lib().kref_align_reduce(K.ptr(W), A, B, S, max_rows, K.ptr(n_rows), K.ptr(n_keys), P, K.ptr(M))
    K.check_rc(rc, "kref_align_reduce")
    return M


def gpu_dtw(M, n_rows, n_keys, P):
    """M f32 [B][max_rows][S] -> first, last i32 [B][max_rows + 1] (entries P + r; -1 elsewhere)"""
    B, max_rows, S = M.shape
    ldo = max_rows + 1
    first, last = np.full((B, ldo), -7, np.int32), np.full((B, ldo), -7, np.int32)
    M, n_rows, n_keys = K.f32(M), i32(n_rows), i32(n_keys)
    rc = lib().kref_align_dtw(K.ptr(M), B, S, max_rows, K.ptr(n_rows), K.ptr(n_keys), P, K.ptr(first), K.ptr(last), ldo)
    K.check_rc(rc, "kref_align_dtw")
    return first, last
