"""GPU: every kernel launcher of nh_kernels.h called directly (tools/kref.hip -> tools/bin/libnh_kref.so) on random data and
compared with a plain fp64 NumPy computation of the same operation on the exact fp16 / f32 inputs the kernel saw (tests/kref.py).
Independent of the C oracle and of every other HIP path.  Each bound is derived from the arithmetic (kref.py), and each case
also shows that the bound would catch plausible bugs on its own data (kref.discriminates)."""
import zlib

import numpy as np
import pytest

import kref as K

pytestmark = pytest.mark.gpu

D = 1280
V_LOGITS = (51866, 51865)     # multilingual / English vocabularies: N not a multiple of 16
ROWS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 95, 96]
WIDTH_ROWS = [1, 17, 33, 65, 96]
WIDTHS = [128, 256, 384, 512, 768, 1024]


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _data(r, R, N, Kd, bias=True):
    x = K.f16(r.standard_normal((R, Kd)))
    W = K.f16(r.standard_normal((N, Kd)) / np.sqrt(Kd))
    b = K.f32(r.standard_normal(N) * 0.5) if bias else None
    return x, W, b


def _skinny(x, W, bias, R, epi, out0, use_wt, ldo, ln=None, qkv=None):
    """one launch_skinny on the first R rows; returns out0 (and the caches for SK_QKV)"""
    L = K.lib()
    N, Kd = W.shape
    o1 = o2 = None
    d = t0 = ctx = B = 0
    pos = None
    if qkv is not None:
        o1, o2, d, t0, ctx, pos = qkv
        B = R
    lnx, lnw, lnb = ln if ln is not None else (None, None, None)
    xx = None if ln is not None else np.ascontiguousarray(x[:R])
    rc = L.kref_skinny(K.ptr(xx), Kd, R, N, Kd, K.ptr(W), K.ptr(bias), int(use_wt), epi, K.ptr(out0), out0.nbytes,
                       K.ptr(o1), K.ptr(o2), 0 if o1 is None else o1.nbytes, ldo, d, t0, 1, ctx, K.ptr(pos), B,
                       K.ptr(None if lnx is None else np.ascontiguousarray(lnx[:R])), K.ptr(lnw), K.ptr(lnb))
    K.check_rc(rc, f"launch_skinny R={R} N={N} K={Kd} epi={epi} wt={use_wt}")
    return out0


# launch_skinny at d = 1280 over the row sweep, on every decoder shape.  Which kernel each (rows, shape, weight layout) reaches is
# skinny_plan (norma_amd/csrc/skinny_plan.h; swept on the CPU by tests/test_kref_cpu.py); test_skinny_sweeps_reach_every_kernel
# asserts through it that these sweeps reach every kernel family and form.
SHAPES = [  # (name, N, K, epilogue)
    ("qkv-f16", 3 * D, D, K.SK_F16),
    ("outproj-resid", D, D, K.SK_RESID_F32),
    ("fc1-gelu", 4 * D, D, K.SK_GELU_F16),
    ("fc2-resid", D, 4 * D, K.SK_RESID_F32),
    ("logits-51866", 51866, D, K.SK_F32),
    ("logits-51865-bias", 51865, D, K.SK_F32),
]


@pytest.mark.parametrize("name,N,Kd,epi", SHAPES, ids=[s[0] for s in SHAPES])
def test_skinny_row_sweep_matches_fp64(name, N, Kd, epi):
    _run_skinny(name, N, Kd, epi, ROWS, bias=not name.startswith("logits-51866"))


# the width sweep: d in 128 .. 1024 at the row counts that change NCB; KS = 2 (d = 128 at K = d: 4 k-steps, fits(4) holds for
# K % 128 == 0 -> KS 4 everywhere except fc2, whose K = 4 d >= 2560 takes 8 / 16 once d >= 640)
@pytest.mark.parametrize("d", WIDTHS)
def test_skinny_width_sweep_matches_fp64(d):
    for name, N, Kd, epi in [("outproj-f16", d, d, K.SK_F16), ("fc1-gelu", 4 * d, d, K.SK_GELU_F16), ("fc2-resid", d, 4 * d, K.SK_RESID_F32)]:
        _run_skinny(f"{name}-d{d}", N, Kd, epi, WIDTH_ROWS)


def _kernel(R, N, Kd, epi, wt, ln=0):
    pl = K.skinny_plan(R, N, Kd, epi, wt, ln)
    return pl["kind"], pl["ncb"], pl["nt"], pl["ksplit"], pl["grid_y"]


def test_skinny_sweeps_reach_every_kernel():
    """what the sweeps of this file rely on reaching, asserted through skinny_plan: (kind, ncb, nt, ksplit, grid.y)"""
    G, LN, LDS, LDSP = K.SKP_GEMM, K.SKP_LN, K.SKP_LDS, K.SKP_LDSP
    f16, resid, gelu, f32 = K.SK_F16, K.SK_RESID_F32, K.SK_GELU_F16, K.SK_F32
    for wt in (0, 1):
        # up to 2560 tiles (QKV 3d, out-proj d, fc1 4d: 240 / 80 / 320 tiles)
        assert _kernel(16, 3 * D, D, f16, wt) == (G, 1, 1, 4, 1)               # one row block: K-sliced, 4 waves at K = 1280
        assert _kernel(16, D, 4 * D, resid, wt) == (G, 1, 1, 16, 1)            # fc2: 16 waves at K = 5120
        assert _kernel(33, D, D, resid, wt) == (G, 1, 1, 4, 3)                 # few tiles: rows split over grid.y
        assert _kernel(64, D, 4 * D, resid, wt) == (G, 1, 1, 16, 4)
        assert _kernel(33, 4 * D, D, gelu, wt) == (G, 3, 1, 4, 1)              # fc1: unsplit (tiles * NCB > 640)
        assert _kernel(64, 3 * D, D, f16, wt) == (G, 4, 1, 4, 1)
        for R in (65, 96):                                                      # more than 64 rows: always split
            assert _kernel(R, 4 * D, D, gelu, wt) == (G, 1, 1, 4, (R + 15) // 16)
        # the logits (>= 2048 tiles)
        assert _kernel(16, 51866, D, f32, wt) == (LDS, 1, 1, 1, 1) and _kernel(32, 51865, D, f32, wt) == (LDS, 2, 1, 1, 1)
    for R in (33, 48, 49, 64, 65, 96):
        assert _kernel(R, 51866, D, f32, 1) == (LDSP, (R + 15) // 16, 2, 1, 1)
    for R in (33, 64):
        assert _kernel(R, 51866, D, f32, 0) == (G, (R + 15) // 16, 2, 1, 1)    # full rows, two tiles per wave
    for R in (65, 80, 96):                                                      # the former hole: nothing was launched
        assert _kernel(R, 51866, D, f32, 0) == (G, 1, 1, 4, (R + 15) // 16)
    # the width sweep: fc2's K = 4 d takes 16 waves once it reaches 2560, 4 below
    assert _kernel(17, 768, 4 * 768, resid, 1)[:4] == (G, 1, 1, 16) and _kernel(17, 128, 4 * 128, resid, 1)[:4] == (G, 1, 1, 4)
    # the fused LayerNorm: one tile per workgroup up to 160 tiles, two beyond with more than one row block; the logits' staging
    for d in LN_WIDTHS:
        assert _kernel(17, d, d, f16, 1, ln=1) == (LN, 1, 1, d // 128, 2)
        assert _kernel(1, 4 * d, d, gelu, 1, ln=1) == (LN, 1, 1, d // 128, 1)
        assert _kernel(96, 4 * d, d, gelu, 0, ln=1) == (LN, 1, 2 if 4 * d // 16 > 160 else 1, d // 128, 6)
    assert _kernel(32, 51866, D, f32, 0, ln=1) == (LDS, 2, 1, 1, 1)


def _run_skinny(name, N, Kd, epi, rows, ln=False, bias=True):
    r = rng("skinny", name)
    x, W, b = _data(r, max(rows), N, Kd, bias)
    ldo = (N + 7) // 8 * 8 if epi == K.SK_F32 else N
    lnargs = None
    if ln:
        lx = K.f32(r.standard_normal((max(rows), Kd)) * 2.0 + 0.3)
        lx[-1] = np.float32(1000.0) + K.f32(r.standard_normal(Kd) * 1e-3)   # large mean, tiny variance
        if max(rows) > 1:
            lx[1] = np.float32(3.7)                                             # a constant row
        lw = K.f32(1.0 + 0.1 * r.standard_normal(Kd))
        lb = K.f32(0.1 * r.standard_normal(Kd))
        lnargs = (lx, lw, lb)
        a_err, a = K.ln_act_bound(lx, lw, lb)
        x = a   # fp64 activations: the reference multiplies the exact LayerNorm
    pre, absdot = K.linear(x, W, b)
    if ln:
        # the kernel's activations are fp16(LN_f32(x)): |a_k - a| <= 2^-11 |a| + 2^-25 + a_err, carried by |W|
        absdot = absdot * (1 + K.U16)
        extra = (K.U16 * np.abs(a) + K.SUB16 + a_err) @ np.abs(K.d64(W)).T
    else:
        extra = 0.0
    resid = K.f32(r.standard_normal((max(rows), N))) if epi == K.SK_RESID_F32 else None
    if epi == K.SK_F32:
        ref, bound, fn = pre, K.f32_out_bound(pre, absdot, Kd) + extra, (lambda v: v)
    elif epi == K.SK_F16:
        ref, bound, fn = pre, K.f16_out_bound(pre, absdot, Kd) + extra, (lambda v: v)
    elif epi == K.SK_GELU_F16:
        ref, bound, fn = K.gelu(pre), K.gelu_f16_bound(pre, absdot, Kd) + 1.13 * extra, K.gelu
    else:
        rr = K.d64(resid)
        ref, bound = pre + rr, K.f32_out_bound(pre + rr, absdot, Kd, extra=rr) + extra
        fn = None
    for R in rows:
        muts_pre = {"last k-step dropped": pre[:R] - K.d64(x[:R, Kd - 32:]) @ K.d64(W[:, Kd - 32:]).T}
        if b is not None:
            nb = pre[:R].copy()
            t0 = ((N - 1) // 16) * 16
            nb[:, t0:] -= K.d64(b[t0:])
            muts_pre["bias missing on the last tile"] = nb
        if R > 1 and R % 16 not in (0, 1):
            nr = pre[:R].copy()
            nr[R - 2] = pre[R - 1]
            muts_pre["ragged block: row reads the next row"] = nr
        muts = {k: (fn(v) if fn else v + K.d64(resid[:R])) for k, v in muts_pre.items()}
        K.discriminates(ref[:R], bound[:R], muts)
        for wt in (0, 1):
            if epi == K.SK_RESID_F32:
                out = resid[:R].copy()
            elif epi == K.SK_F32:
                out = np.full((R, ldo), np.float32(7.25), dtype=np.float32)
            else:
                out = np.full((R, N), np.float16(7.25), dtype=np.float16)
            got = _skinny(x if not ln else None, W, b, R, epi, out, wt, ldo, ln=lnargs)
            K.within(got[:, :N], ref[:R], bound[:R], f"{name} R={R} Wt={wt}")
            if ldo > N:
                assert np.all(got[:, N:] == np.float32(7.25)), f"{name} R={R}: wrote past N"


# LayerNorm fused into the activation load wherever skinny_ln_supported says so: STEPS = K / 128 in {1, 2, 3, 4, 6, 8, 10}
# (skinny_ln_kernel<STEPS, NT>), NT = 2 for > 160 tiles with more than one row block (fc1 at d >= 768), and the logits'
# skinny_lds_kernel with its LayerNorm staging (R <= 32).  Each case includes a constant row and a row 1000 + 1e-3 noise.
LN_WIDTHS = [128, 256, 384, 512, 768, 1024, 1280]


@pytest.mark.parametrize("d", LN_WIDTHS)
def test_skinny_fused_layernorm_matches_fp64(d):
    L = K.lib()
    for name, N, epi in [("q-f16", d, K.SK_F16), ("fc1-gelu", 4 * d, K.SK_GELU_F16)]:
        rows = [R for R in WIDTH_ROWS if L.kref_skinny_ln_supported(R, N, d)]
        assert rows == WIDTH_ROWS, (name, d, rows)
        _run_skinny(f"ln-{name}-d{d}", N, d, epi, rows, ln=True)


def test_skinny_fused_layernorm_logits_matches_fp64():
    L = K.lib()
    rows = [R for R in [1, 2, 17, 31, 32] if L.kref_skinny_ln_supported(R, 51866, D)]
    assert rows == [1, 2, 17, 31, 32]
    r = rng("ln-logits")
    N = 51866
    W = K.f16(r.standard_normal((N, D)) / np.sqrt(D))
    lx = K.f32(r.standard_normal((32, D)) * 2.0)
    lx[5] = np.float32(1000.0) + K.f32(r.standard_normal(D) * 1e-3)
    lw, lb = K.f32(1.0 + 0.1 * r.standard_normal(D)), K.f32(0.1 * r.standard_normal(D))
    a_err, a = K.ln_act_bound(lx, lw, lb)
    pre, absdot = K.linear(a, W)
    bound = K.f32_out_bound(pre, absdot * (1 + K.U16), D) + (K.U16 * np.abs(a) + K.SUB16 + a_err) @ np.abs(K.d64(W)).T
    ldo = (N + 7) // 8 * 8
    for R in rows:
        drop = pre[:R] - K.d64(a[:R, D - 32:]) @ K.d64(W[:, D - 32:]).T
        muts = {"last k-step dropped": drop}
        if R > 2:
            nr = pre[:R].copy(); nr[R - 2] = pre[R - 1]
            muts["ragged block: row reads the next row"] = nr
        K.discriminates(pre[:R], bound[:R], muts)
        for wt in (0, 1):
            out = np.full((R, ldo), np.float32(7.25), dtype=np.float32)
            got = _skinny(None, W, None, R, K.SK_F32, out, wt, ldo, ln=(lx, lw, lb))
            K.within(got[:, :N], pre[:R], bound[:R], f"ln-logits R={R} Wt={wt}")


def test_skinny_refuses_fused_layernorm_where_unsupported():
    """launch_skinny must not silently compute from x when ln_x is set on a shape skinny_ln_supported rejects"""
    L = K.lib()
    assert not L.kref_skinny_ln_supported(33, 51866, D)
    r = rng("refuse")
    W = K.f16(r.standard_normal((51866, 128)))
    lx = K.f32(r.standard_normal((33, 128)))
    lw = K.f32(np.ones(128)); lb = K.f32(np.zeros(128))
    out = np.full((33, 51872), np.float32(7.25), np.float32)
    rc = L.kref_skinny(None, 128, 33, 51866, 128, K.ptr(W), None, 0, K.SK_F32, K.ptr(out), out.nbytes, None, None, 0, 51872,
                       0, 0, 1, 0, None, 0, K.ptr(lx), K.ptr(lw), K.ptr(lb))
    assert rc == -1
    assert np.all(out == np.float32(7.25)), "a refused launch wrote to its output"
    # what the kernels cannot compute is refused too, with the output (poisoned; the wrapper copies it back) left alone:
    # K % 64 != 0 (the narrowest form cuts K into two slices of whole 32-deep k-steps: the tail of K would be dropped) and
    # N % 4 != 0 under an epilogue that stores four features at a time
    for R, N, Kd, epi in [(16, 1280, 96, K.SK_F16), (16, 6, 128, K.SK_F16)]:
        x, W, b = _data(r, R, N, Kd)
        for wt in (0, 1):
            assert K.skinny_plan(R, N, Kd, epi, wt, 0)["kind"] == K.SKP_NONE
            out = np.full((R, N), np.float16(7.25), np.float16)
            rc = L.kref_skinny(K.ptr(x), Kd, R, N, Kd, K.ptr(W), K.ptr(b), wt, epi, K.ptr(out), out.nbytes, None, None, 0, N,
                               0, 0, 1, 0, None, 0, None, None, None)
            assert rc == -1, (R, N, Kd, wt)
            assert np.all(out == np.float16(7.25)), "a refused launch wrote to its output"


# SK_QKV: q -> out0 [R][d]; k, v -> head-major caches [B][H][ctx][64] at t0 (or pos_ptr[b]); every other position untouched
@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("per_row", [False, True])
def test_skinny_qkv_writes_the_cache_position_only(d, per_row):
    r = rng("qkv", d, per_row)
    H, ctx = d // 64, 24
    x, W, b = _data(r, 96, 3 * d, d, True)
    pre, absdot = K.linear(x, W, b)
    bound = K.f16_out_bound(pre, absdot, d)
    for R in WIDTH_ROWS:
        t0 = 5
        pos = np.ascontiguousarray(r.integers(0, ctx, R), dtype=np.int32) if per_row else None
        kc0 = K.f16(r.standard_normal((R, H, ctx, 64)))
        vc0 = K.f16(r.standard_normal((R, H, ctx, 64)))
        q = np.full((R, d), np.float16(7.25), np.float16)
        kc, vc = kc0.copy(), vc0.copy()
        _skinny(x, W, b, R, K.SK_QKV, q, 1, d, qkv=(kc, vc, d, t0, ctx, pos))
        K.within(q, pre[:R, :d], bound[:R, :d], f"qkv q d={d} R={R}")
        at = pos if per_row else np.full(R, t0)
        for name, cache, cache0, seg in [("k", kc, kc0, 1), ("v", vc, vc0, 2)]:
            want = pre[:R, seg * d:(seg + 1) * d].reshape(R, H, 64)
            wb = bound[:R, seg * d:(seg + 1) * d].reshape(R, H, 64)
            got = cache[np.arange(R), :, at, :]
            K.within(got, want, wb, f"qkv {name} d={d} R={R}")
            mask = np.ones((R, ctx), bool)
            mask[np.arange(R), at] = False
            assert np.array_equal(cache.transpose(0, 2, 1, 3)[mask].view(np.uint16), cache0.transpose(0, 2, 1, 3)[mask].view(np.uint16)), \
                f"qkv {name}: positions other than the row's own were written"
            # discrimination: one row written at its position off by one would leave the bound (the random cache content)
            if R > 1:
                alt = cache0[np.arange(R), :, (at + 1) % ctx, :]
                assert K.violation(want, wb, alt) > 2


# ---- decoder attention -----------------------------------------------------------------------------------------------------
SELF_BH = [(1, 6), (5, 8), (33, 12), (96, 16), (5, 20)]
SELF_KEYS = [1, 2, 7, 8, 9, 31, 32, 33, 255, 447, 448]
CTX = 448


def _attn_case(r, B, H, T, scale=1.0):
    d = 64 * H
    q = K.f16(r.standard_normal((B, d)) * scale)
    k = K.f16(r.standard_normal((B, T, d)))
    v = K.f16(r.standard_normal((B, T, d)))
    return q, k, v


def _dec_run(q, k, v, H, Tk, pos=None, done=None, out=None):
    L = K.lib()
    B, d = q.shape
    ctx = k.shape[1]
    kk = K.head_major(k, H)
    vv = K.head_major(v, H)
    out = np.full((B, d), np.float16(7.25), np.float16) if out is None else out
    rc = L.kref_dec_attention(K.ptr(q), K.ptr(kk), K.ptr(vv), K.ptr(out), B, H, d, ctx, Tk, K.ptr(pos), 1, K.ptr(done))
    K.check_rc(rc, f"launch_dec_attention B={B} H={H} Tk={Tk}")
    return out


def _dec_mutations(q, k, v, H, nvis, ctx):
    B = q.shape[0]
    nvis = np.asarray(nvis)
    m = {}
    if (nvis > 1).all():
        m["one visible key too few"] = K.dec_attention(q, k, v, H, nvis - 1)[0]
    if (nvis < ctx).all():
        m["one visible key too many"] = K.dec_attention(q, k, v, H, nvis + 1)[0]
    if H > 1:
        o = K.dec_attention(q, k, v, H, nvis)[0]
        d = 64 * H
        vs = v.copy()
        vs[:, :, d - 64:] = v[:, :, d - 128:d - 64]
        m["last head reads the previous head's V"] = K.dec_attention(q, k, vs, H, nvis)[0]
    return m


# dec_attn_kernel, causal self-attention over the head-major cache (the product's layout): visible keys across the 8-key slot
# groups, the 4 waves' key ranges and the 448 cap; B and H across the grid
@pytest.mark.parametrize("B,H", SELF_BH)
def test_dec_attention_self_matches_fp64(B, H):
    r = rng("dec", B, H)
    q, k, v = _attn_case(r, B, H, CTX)
    for Tk in SELF_KEYS:
        ref, sabs, vst = K.dec_attention(q, k, v, H, [Tk] * B)
        bound = K.attn_bound(ref, sabs, [Tk] * B, vst)
        if Tk > 1 or H > 1:
            K.discriminates(ref, bound, _dec_mutations(q, k, v, H, [Tk] * B, CTX))
        got = _dec_run(q, k, v, H, Tk)
        K.within(got, ref, bound, f"dec self B={B} H={H} Tk={Tk}")


def test_dec_attention_per_row_positions_match_fp64():
    """pos_ptr (the pool / graph path): every row at a different position, 0 and 447 included"""
    r = rng("dec-pos")
    B, H = 33, 8
    q, k, v = _attn_case(r, B, H, CTX)
    pos = np.ascontiguousarray(np.concatenate([[0, 447], r.choice(np.arange(1, 447), B - 2, replace=False)]), dtype=np.int32)
    ref, sabs, vst = K.dec_attention(q, k, v, H, pos + 1)
    bound = K.attn_bound(ref, sabs, pos + 1, vst)
    for b0 in (1, 2):   # one pos_ptr row off by one (either way that stays inside the cache)
        pm = pos.copy(); pm[b0] += 1 if pm[b0] < 447 else -1
        K.discriminates(ref, bound, {f"pos_ptr row {b0} off by one": K.dec_attention(q, k, v, H, pm + 1)[0]})
    got = _dec_run(q, k, v, H, 0, pos=pos)
    K.within(got, ref, bound, "dec self pos_ptr")


@pytest.mark.parametrize("Tk", [1500, 750])
def test_dec_attention_cross_head_major_matches_fp64(Tk):
    r = rng("dec-cross", Tk)
    B, H = 5, 20
    q, k, v = _attn_case(r, B, H, Tk)
    ref, sabs, vst = K.dec_attention(q, k, v, H, [Tk] * B)
    bound = K.attn_bound(ref, sabs, [Tk] * B, vst)
    m = _dec_mutations(q, k, v, H, [Tk] * B, Tk)
    assert "one visible key too few" in m
    K.discriminates(ref, bound, m)
    K.within(_dec_run(q, k, v, H, Tk), ref, bound, f"dec cross Tk={Tk}")


def test_dec_attention_done_rows_are_untouched():
    r = rng("dec-done")
    B, H, Tk = 9, 6, 100
    q, k, v = _attn_case(r, B, H, 128)
    done = np.ascontiguousarray([0, 1, 0, 0, 1, 1, 0, 0, 1], dtype=np.int32)
    before = K.f16(r.standard_normal((B, 64 * H)))
    got = _dec_run(q, k, v, H, Tk, done=done, out=before.copy())
    assert np.array_equal(got[done == 1].view(np.uint16), before[done == 1].view(np.uint16))
    live = done == 0
    ref, sabs, vst = K.dec_attention(q[live], k[live], v[live], H, [Tk] * int(live.sum()))
    bound = K.attn_bound(ref, sabs, [Tk] * int(live.sum()), vst)
    K.discriminates(ref, bound, _dec_mutations(q[live], k[live], v[live], H, [Tk] * int(live.sum()), 128))
    K.within(got[live], ref, bound, "dec done: live rows")


def test_dec_attention_adversarial_scores():
    """row 0: all keys equal (uniform weights); row 1: the last visible key and the first invisible one score ~40 above the rest
    in every head (a key too few drops the dominating key, a key too many halves its weight).  The cache is 8 keys longer than
    the visible range, so a key too many is a real read.  Each adversarial row must catch both mutations on its own."""
    r = rng("dec-adv")
    B, H, T = 4, 8, 300
    q, k, v = _attn_case(r, B, H, T + 8)
    k[0, :, :] = k[0, 0, :]
    for h in range(H):
        qs = K.d64(q[1, 64 * h:64 * h + 64])
        k[1, T - 1:T + 1, 64 * h:64 * h + 64] = K.f16(qs / np.dot(qs, qs) * 8.0 * 40.0)
    ref, sabs, vst = K.dec_attention(q, k, v, H, [T] * B)
    bound = K.attn_bound(ref, sabs, [T] * B, vst)
    muts = _dec_mutations(q, k, v, H, [T] * B, T + 8)
    for row in (0, 1):
        K.discriminates(ref[row], bound[row], {name: m[row] for name, m in muts.items() if "key" in name})
    K.discriminates(ref, bound, muts)
    got = _dec_run(q, k, v, H, T)
    K.within(got, ref, bound, "dec adversarial")


# ---- absorbed cross-attention ----------------------------------------------------------------------------------------------
def _xabs_case(r, B, d, S):
    """q scaled by 3 (scores ~ N(0, 9): the weights concentrate on a few keys, so z and the value projection are O(1)); in head
    0 of every row the LAST key carries half the weight (its score = logsumexp of the others), so a key too few or one counted
    twice moves the output by O(1)"""
    H = d // 64
    q = K.f16(r.standard_normal((B, d)) * 3.0)
    Wkv = K.f16(r.standard_normal((2 * d, d)) / np.sqrt(d))
    bkv = K.f32(r.standard_normal(2 * d) * 0.5)
    xa = K.f16(r.standard_normal((B, S, d)))
    Wk0 = K.d64(Wkv[:64])
    for b in range(B):
        u0 = Wk0.T @ K.d64(q[b, :64]) / 8.0
        so = K.d64(xa[b, :S - 1]) @ u0
        target = so.max() + np.log(np.exp(so - so.max()).sum())
        xa[b, S - 1] = K.f16(target * u0 / np.dot(u0, u0))
    return q, Wkv, bkv, xa


def _xabs_run(q, Wkv, bkv, xa, H, fast, done=None, out=None):
    L = K.lib()
    B, d = q.shape
    S = xa.shape[1]
    out = np.full((B, d), np.float16(7.25), np.float16) if out is None else out
    rc = L.kref_xabs_attention(K.ptr(q), K.ptr(Wkv), K.ptr(bkv), K.ptr(xa), K.ptr(out), B, H, d, S, K.ptr(done), int(fast))
    K.check_rc(rc, f"xabs fast={fast} B={B} d={d} S={S}")
    return out


def _xabs_mutations(q, Wkv, bkv, xa, H):
    d = q.shape[1]
    Wm = Wkv.copy()
    Wm[2 * d - 64:] = Wkv[2 * d - 128:2 * d - 64]
    bm = bkv.copy()
    bm[2 * d - 16:] = 0
    return {"one key too few": K.xabs_attention(q, Wkv, bkv, xa[:, :-1], H),
            "the last key counted twice": K.xabs_attention(q, Wkv, bkv, np.concatenate([xa, xa[:, -1:]], axis=1), H),
            "last head reads the previous head's Wv": K.xabs_attention(q, Wm, bkv, xa, H),
            "bv missing on the last 16 columns": K.xabs_attention(q, Wkv, bm, xa, H)}


# launch_xabs_attention (xabs_u_kernel + xabs_attn_kernel) at every width, launch_xabs_attention_fast (xabs_u_fast_kernel,
# xabs_main_kernel<D>, xabs_zmerge_kernel, xabs_oproj_kernel<D>) at D = 512 .. 1280; rows 1, 31, 32, 33, 64, 96 (the fast form's
# 32-row blocks) and S = 1500, 750 spread over both forms
XABS_CASES = [(0, 384, 1500, 96), (0, 512, 750, 64), (0, 768, 1500, 33), (0, 1024, 750, 32), (0, 1280, 1500, 31), (0, 1280, 750, 1),
              (1, 512, 1500, 96), (1, 512, 750, 33), (1, 768, 750, 64), (1, 1024, 1500, 32), (1, 1280, 750, 31), (1, 1280, 1500, 1)]


@pytest.mark.parametrize("fast,d,S,B", XABS_CASES)
def test_xabs_attention_matches_fp64_formula(fast, d, S, B):
    r = rng("xabs", fast, d, S, B)
    H = d // 64
    q, Wkv, bkv, xa = _xabs_case(r, B, d, S)
    ref, bound = K.xabs_reference(q, Wkv, bkv, xa, H)
    K.discriminates(ref, bound, _xabs_mutations(q, Wkv, bkv, xa, H))
    K.within(_xabs_run(q, Wkv, bkv, xa, H, fast), ref, bound, f"xabs fast={fast} d={d} S={S} B={B}")


@pytest.mark.parametrize("d,S", [(768, 1500), (1280, 750)])
def test_dec_attention_on_projected_kv_matches_the_xabs_formula(d, S):
    """the absorbed forms' reference reached the other way: dec_attn_kernel on K / V projected in fp64 and rounded to fp16.  Its
    bound: attn_bound around the fp64 attention on the rounded K / V, plus the exact fp64 distance from that to the formula (the
    effect of rounding K and V), by the triangle inequality"""
    r = rng("xabs-vs-dec", d, S)
    B, H = 3, d // 64
    q, Wkv, bkv, xa = _xabs_case(r, B, d, S)
    ref = K.xabs_attention(q, Wkv, bkv, xa, H)
    Kp, Vp = K.xabs_projected(xa, Wkv, bkv, d)
    k16, v16 = K.f16(Kp), K.f16(Vp)
    ref16, sabs, vst = K.dec_attention(q, k16, v16, H, [S] * B)
    bound = K.attn_bound(ref16, sabs, [S] * B, vst) + np.abs(ref16 - ref)
    K.discriminates(ref, bound, _xabs_mutations(q, Wkv, bkv, xa, H))
    K.within(_dec_run(q, k16, v16, H, S), ref, bound, f"dec attention on fp16 projected K/V d={d} S={S}")


@pytest.mark.parametrize("fast", [0, 1])
def test_xabs_attention_done_rows_are_untouched(fast):
    r = rng("xabs-done", fast)
    B, d, S = 6, 512, 750
    H = d // 64
    q, Wkv, bkv, xa = _xabs_case(r, B, d, S)
    done = np.ascontiguousarray([1, 0, 0, 1, 0, 1], dtype=np.int32)
    before = K.f16(r.standard_normal((B, d)))
    got = _xabs_run(q, Wkv, bkv, xa, H, fast, done=done, out=before.copy())
    assert np.array_equal(got[done == 1].view(np.uint16), before[done == 1].view(np.uint16))
    live = done == 0
    ref, bound = K.xabs_reference(q[live], Wkv, bkv, xa[live], H)
    K.discriminates(ref, bound, _xabs_mutations(q[live], Wkv, bkv, xa[live], H))
    K.within(got[live], ref, bound, "xabs done: live rows")


# ---- encoder attention ------------------------------------------------------------------------------------------------------
ENC_CASES = [(1, 1500, 6), (1, 1500, 20), (3, 1500, 8), (1, 750, 12), (3, 750, 16), (3, 750, 20)]


def _enc_run(q, k, vt, B, S, H):
    L = K.lib()
    d = 64 * H
    out = np.full((B * S, d), np.float16(7.25), np.float16)
    rc = L.kref_enc_attention(K.ptr(q), K.ptr(k), d, K.ptr(vt), K.ptr(out), d, B, S, H)
    K.check_rc(rc, f"enc attention B={B} S={S} H={H}")
    return out


# enc_attn_kernel: q pre-scaled by NH_ENC_Q_SCALE, scores in log2 units, P in fp16 for the PV product, V^T pad columns S..1535
@pytest.mark.parametrize("B,S,H", ENC_CASES)
def test_enc_attention_matches_fp64(B, S, H):
    r = rng("enc", B, S, H)
    d = 64 * H
    q = K.f16(r.standard_normal((B * S, d)) * K.ENC_Q_SCALE)
    k = K.f16(r.standard_normal((B * S, d)))
    v = K.f16(r.standard_normal((B * S, d)))
    ref, sabs, vstat = K.enc_attention(q, k, v, B, S, H)
    bound = K.attn_bound(ref, sabs, np.full(B * S, S), vstat, p16=True, log2=True)
    # mutations: the last key dropped (a tile mask off by one), the last head reading the previous head's V
    vm = v.copy(); vm[:, d - 64:] = v[:, d - 128:d - 64]
    muts = {"last head reads the previous head's V": K.enc_attention(q, k, vm, B, S, H)[0]}
    qq, kk, vv = (a.reshape(B, S, d) for a in (q, k, v))
    muts["last key dropped"] = np.concatenate([_enc_ref_keys(qq[b], kk[b, :S - 1], vv[b, :S - 1], H) for b in range(B)])
    K.discriminates(ref, bound, muts)
    vt = K.vt_image(v, H, S)
    got = _enc_run(q, k, vt, B, S, H)
    K.within(got, ref, bound, f"enc attention B={B} S={S} H={H}")
    # the pad columns of V^T: the kernel masks keys >= S, so finite garbage there must not change a bit (the contract in
    # nh_kernels.h: the pad holds finite values -- the QKV GEMM's V^T epilogue never writes it, the context zeroes it once)
    vt2 = vt.copy()
    vt2[:, :, :, S:] = np.float16(1000.0)
    assert np.array_equal(_enc_run(q, k, vt2, B, S, H).view(np.uint16), got.view(np.uint16))
    # ... and the other half: the masked keys' zero weights still multiply the pad, so a NaN there reaches the output
    vt2[:, :, :, S:] = np.float16(np.nan)
    assert not np.isfinite(_enc_run(q, k, vt2, B, S, H)).all(), "a NaN pad left the output finite: the contract is not needed"


def _enc_ref_keys(q, k, v, H):
    """encoder attention of S queries over the first len(k) keys only"""
    q, k, v = K.d64(q), K.d64(k), K.d64(v)
    o = np.zeros_like(q)
    for h in range(H):
        c = slice(64 * h, 64 * h + 64)
        o[:, c] = K.softmax_attend((q[:, c] @ k[:, c].T) * np.log(2.0), v[:, c])
    return o


# ---- prefill attention (k_prefill.hip: the one-pass teacher-forced decoder forward) -----------------------------------------------
# prefill_attn_kernel<true> / <false> through launch_prefill_self_attention / launch_prefill_cross_attention: one workgroup per
# (256-query tile, head, clip), one wave per 16 queries, keys in blocks of 64, P.V in k-steps of 32 keys.  Reference and bound:
# kref.prefill_attention / prefill_bound.  Canaries (7.25, -3.5) fill everything the kernel must not write.
PF_C = 448
# the wave (16), k-step (32), key-block (64) and query-tile (256) edges; 300: a second tile of three waves; 448: a second tile
# of twelve live waves and four idle ones
PF_T = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 223, 255, 256, 257, 300, 448]
PF_SELF = [(1, 2, PF_T), (3, 6, [1, 17, 64, 65, 223, 257, 448]), (2, 20, [2, 33, 129, 300])]
PF_WORST = {}      # worst |err| / bound per section, printed by each test (reported, never asserted)


def _pf_report(section, got, ref, bound):
    PF_WORST[section] = max(PF_WORST.get(section, 0.0), K.violation(ref, bound, got))
    print(f"worst |err| / bound so far, {section}: {PF_WORST[section]:.3f}")


def _pf_self_run(q, k, v, ld, B, T, H, C=PF_C, ldo=None, expect=0):
    """one launch_prefill_self_attention; returns (out [B*T][ldo], ck, cv [B][H][C][64]); out is filled with 7.25, ck with
    7.25 and cv with -3.5 beforehand"""
    ldo = 64 * H if ldo is None else ldo
    out = np.full((max(B * T, 1), ldo), np.float16(7.25), np.float16)
    ck = np.full((B, H, C, 64), np.float16(7.25), np.float16)
    cv = np.full((B, H, C, 64), np.float16(-3.5), np.float16)
    rc = K.lib().kref_prefill_self_attention(K.ptr(q), K.ptr(k), K.ptr(v), ld, K.ptr(out), ldo, K.ptr(ck), K.ptr(cv), B, T, H, C)
    if expect == 0:
        K.check_rc(rc, f"launch_prefill_self_attention B={B} T={T} H={H}")
    else:
        assert rc == expect, rc
    return out, ck, cv


def _pf_cross_run(q, ck, cv, B, T, H, S, expect=0):
    """one launch_prefill_cross_attention on head-major K/V of exactly S keys per (clip, head); returns (out, ck, cv) as the
    wrapper copied them back"""
    out = np.full((max(B * T, 1), 64 * H), np.float16(7.25), np.float16)
    ck, cv = ck.copy(), cv.copy()
    rc = K.lib().kref_prefill_cross_attention(K.ptr(q), 64 * H, K.ptr(ck), K.ptr(cv), K.ptr(out), 64 * H, B, T, H, S)
    if expect == 0:
        K.check_rc(rc, f"launch_prefill_cross_attention B={B} T={T} H={H} S={S}")
    else:
        assert rc == expect, rc
    return out, ck, cv


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _pf_check_self_cache(ck, cv, k, v, B, T, H, what):
    """slots 0 .. T-1 bit-equal to the input k / v rows of every (clip, head), slots T .. C-1 untouched"""
    d = 64 * H
    for name, cache, src, canary in (("ck", ck, k, 7.25), ("cv", cv, v, -3.5)):
        want = K.head_major(np.ascontiguousarray(src).reshape(B, T, d), H)
        assert np.array_equal(_bits(cache[:, :, :T]), _bits(want)), f"{what}: {name} slots 0..T-1 are not the input rows"
        assert np.all(cache[:, :, T:] == np.float16(canary)), f"{what}: {name} written past slot T-1"


def _pf_self_mutations(q, k, v, B, T, H):
    d = 64 * H
    i = np.arange(T)

    def mut(kk=k, vv=v, **kw):
        return K.prefill_attention(q, kk, vv, B, T, H, T, True, stats=False, **kw)[0]

    m = {}
    if T >= 2:
        m["causal mask one key short (queries i >= 1)"] = mut(nvis=np.maximum(i, 1))
        m["causal mask one key long (queries i < T-1)"] = mut(nvis=np.minimum(i + 2, T))
    if H > 1:
        vs = v.copy(); vs[:, d - 64:] = v[:, d - 128:d - 64]
        m["last head reads the previous head's V"] = mut(vv=vs)
    if B > 1:
        m["clip b reads clip b-1's keys"] = mut(kk=np.roll(k.reshape(B, T, d), 1, axis=0), vv=np.roll(v.reshape(B, T, d), 1, axis=0))
    if T >= 5:       # keys 0 .. 3 of a k-step sit in their natural slots
        m["keys of a 32-key step reach V in natural order"] = mut(vperm=K.pf_natural_order(T))
    if T > 256:
        m["the second query tile ignores keys below 256"] = mut(first=np.where(i >= 256, 256, 0))
    return m


@pytest.mark.parametrize("B,H,Ts", PF_SELF, ids=[f"B{b}-H{h}" for b, h, _ in PF_SELF])
def test_prefill_self_attention_matches_fp64(B, H, Ts):
    """causal form, C = 448, separate q / k / v buffers (ld = ldo = 64 H): the output inside the bound, the self cache bit-equal
    at slots 0 .. T-1 and untouched beyond -- at T = 300 and 448 too, where only the clip's last tile writes it"""
    d = 64 * H
    for T in Ts:
        r = rng("pf-self", B, H, T)
        q, k, v = (K.f16(r.standard_normal((B * T, d))) for _ in range(3))
        ref, sabs, vst, n = K.prefill_attention(q, k, v, B, T, H, T, True)
        bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(q, k, v, B, T, H, T, True))
        muts = _pf_self_mutations(q, k, v, B, T, H)
        assert muts or (B, H, T) == (1, 1, 1)
        K.discriminates(ref, bound, muts)
        out, ck, cv = _pf_self_run(q, k, v, d, B, T, H)
        _pf_report("self", out, ref, bound)
        K.within(out, ref, bound, f"prefill self B={B} H={H} T={T}")
        _pf_check_self_cache(ck, cv, k, v, B, T, H, f"prefill self B={B} H={H} T={T}")


@pytest.mark.parametrize("T", [33, 300])
def test_prefill_self_attention_on_column_slices_of_one_qkv_buffer(T):
    """ld = 3 * 64 H: q, k and v are column slices of one [B*T][3 d] buffer, and ldo > 64 H: the pad columns of out stay"""
    B, H = 2, 6
    d = 64 * H
    r = rng("pf-self-qkv", T)
    qkv = K.f16(r.standard_normal((B * T, 3 * d)))
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    ref, sabs, vst, n = K.prefill_attention(q, k, v, B, T, H, T, True)
    bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(q, k, v, B, T, H, T, True))
    K.discriminates(ref, bound, _pf_self_mutations(np.ascontiguousarray(q), np.ascontiguousarray(k), np.ascontiguousarray(v), B, T, H))
    # a row stride mistaken for d: row r of q would be read at r * d of the buffer
    flat = qkv.reshape(-1)
    wrong_q = np.stack([flat[r_ * d:r_ * d + d] for r_ in range(B * T)])
    K.discriminates(ref, bound, {"q read with ld = d": K.prefill_attention(wrong_q, k, v, B, T, H, T, True, stats=False)[0]})
    ldo = d + 64
    out, ck, cv = _pf_self_run(q, k, v, 3 * d, B, T, H, ldo=ldo)
    _pf_report("self", out[:, :d], ref, bound)
    K.within(out[:, :d], ref, bound, f"prefill self on qkv slices T={T}")
    assert np.all(out[:, d:] == np.float16(7.25)), "the pad columns of out were written"
    _pf_check_self_cache(ck, cv, k, v, B, T, H, f"prefill self on qkv slices T={T}")


# every S has a ragged last block but 64; 750 = 11 * 64 + 46, 1500 = 23 * 64 + 28; T: one query, one wave + 1, the longest prefix
# of a decode (14 waves), two tiles
PF_CROSS = [(2, 3, 17, 1), (2, 3, 1, 63), (3, 6, 17, 64), (2, 3, 223, 65), (2, 6, 300, 750), (1, 20, 17, 1500), (3, 2, 223, 1500),
            (2, 3, 1, 750)]


@pytest.mark.parametrize("B,H,T,S", PF_CROSS)
def test_prefill_cross_attention_matches_fp64(B, H, T, S):
    r = rng("pf-cross", B, H, T, S)
    q, ck, cv = K.prefill_cross_case(r, B, T, H, S)
    U = B * H
    qu, ku, vu = K.pf_units(q, B, T, H), K.pf_from_head_major(ck, B, H, S), K.pf_from_head_major(cv, B, H, S)
    ref, sabs, vst, n = K.prefill_attention(qu, ku, vu, 1, T, U, S, False)
    bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(qu, ku, vu, 1, T, U, S, False))
    muts = K.prefill_cross_mutations(qu, ku, vu, B, T, H, S)
    assert "one key too many" in muts and ("one key too few" in muts or S == 1)
    K.discriminates(ref, bound, muts)
    out, ck2, cv2 = _pf_cross_run(q, ck, cv, B, T, H, S)
    _pf_report("cross", K.pf_units(out, B, T, H), ref, bound)
    K.within(K.pf_units(out, B, T, H), ref, bound, f"prefill cross B={B} H={H} T={T} S={S}")
    assert np.array_equal(_bits(ck2), _bits(ck)) and np.array_equal(_bits(cv2), _bits(cv)), "the cross K/V were written"


@pytest.mark.parametrize("causal", [True, False], ids=["self", "cross"])
def test_prefill_attention_adversarial_scores(causal):
    """kref.prefill_adversarial: one (clip, head) unit per family -- all keys equal; scores ascending by 0.2 per key over five
    64-key blocks, so every block rescales; one key 40 above the rest in the first block, so later blocks' P is zero in fp16
    while l still counts it; the dominating key last in sight with an equally loud one first out of sight.  Every unit must
    catch both mask errors by itself (the cross form's dominant-first unit: a key too many only -- its last key holds e^-40
    of the weight by construction)."""
    r = rng("pf-adv", causal)
    T, nk = (300, 300) if causal else (17, 300)
    qa, ka, va = K.prefill_adversarial(r, T, nk, causal)
    U = qa.shape[0]
    qu, ku, vu = (np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(a.shape[1], U * 64) for a in (qa, ka, va))
    ref, sabs, vst, n = K.prefill_attention(qu, ku, vu, 1, T, U, nk, causal)
    bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(qu, ku, vu, 1, T, U, nk, causal))
    muts = K.prefill_mask_mutations(qu, ku, vu, T, U, nk, causal)
    for u, fam in enumerate(K.PF_FAMILIES):
        c = slice(64 * u, 64 * u + 64)
        for name, m in muts.items():
            if (causal, fam, name) != (False, "dominant-first", "one key too few"):
                K.discriminates(ref[:, c], bound[:, c], {f"{fam}: {name}": m[:, c]})
    if causal:
        out, ck, cv = _pf_self_run(qu, ku, vu, 64 * U, 1, T, U)
        _pf_check_self_cache(ck, cv, ku, vu, 1, T, U, "prefill self adversarial")
    else:
        out = _pf_cross_run(qu, ka, va, 1, T, U, nk)[0]       # [U][nk][64] IS the head-major buffer of one clip
    _pf_report("adversarial", out, ref, bound)
    K.within(out, ref, bound, f"prefill adversarial causal={causal}")


def test_prefill_attention_refuses_empty_and_oversized_shapes():
    """T = 0, T > C and S = 0 return false (the wrapper: -1) and leave out, ck and cv bit-identical"""
    B, H = 2, 2
    r = rng("pf-refuse")
    for T, C in ((0, PF_C), (PF_C + 1, PF_C), (17, 16)):
        rows = max(B * T, 1)
        q, k, v = (K.f16(r.standard_normal((rows, 64 * H))) for _ in range(3))
        out, ck, cv = _pf_self_run(q, k, v, 64 * H, B, T, H, C=C, expect=-1)
        assert np.all(out == np.float16(7.25)) and np.all(ck == np.float16(7.25)) and np.all(cv == np.float16(-3.5)), (T, C)
    for T, S in ((0, 5), (3, 0)):
        q = K.f16(r.standard_normal((max(B * T, 1), 64 * H)))
        ck = K.f16(r.standard_normal((B, H, max(S, 1), 64))); cv = K.f16(r.standard_normal((B, H, max(S, 1), 64)))
        out, ck2, cv2 = _pf_cross_run(q, ck, cv, B, T, H, S, expect=-1)
        assert np.all(out == np.float16(7.25)) and np.array_equal(_bits(ck2), _bits(ck)) and np.array_equal(_bits(cv2), _bits(cv))


# ---- GEMM epilogues ---------------------------------------------------------------------------------------------------------
def _gemm(kernel128, A, lda, a_rpb, a_bstride, W, bias, M, epi, outs, seg_n, ldo, o_rpb=0, o_bstride=0, o_off=0, vt_seg=-1,
          head_major=0, seg0_scale=0.0, S=0, H=0, pos=None):
    L = K.lib()
    N, Kd = W.shape
    o = list(outs) + [None] * (3 - len(outs))
    rc = L.kref_gemm(int(kernel128), K.ptr(A), A.nbytes, lda, a_rpb or M, a_bstride, K.ptr(W), K.ptr(bias), M, N, Kd, epi,
                     K.ptr(o[0]), K.ptr(o[1]), K.ptr(o[2]), outs[0].nbytes, seg_n, ldo, o_rpb or M, o_bstride, o_off, vt_seg,
                     head_major, seg0_scale, S, H, K.ptr(pos))
    K.check_rc(rc, f"launch_gemm{'_128' if kernel128 else ''} M={M} N={N} K={Kd} epi={epi}")


def _gemm_muts(pre, Ar, W, bias, fn, M):
    Kd = W.shape[1]
    m = {"last k-step dropped": fn(pre - K.d64(Ar[:, Kd - 32:]) @ K.d64(W[:, Kd - 32:]).T)}
    if bias is not None:
        nb = pre.copy(); nb[:, -16:] -= K.d64(bias[-16:])
        m["bias missing on the last tile"] = fn(nb)
    if M >= 2:
        nr = pre.copy(); nr[M - 2] = pre[M - 1]
        m["ragged rows: row reads the next row"] = fn(nr)
    return m


# gemm256_f16_kernel<EPI> (launch_gemm: N % 256 == 0, K % 128 == 0, M >= 256) and gemm_f16_kernel (launch_gemm_128)
@pytest.mark.parametrize("kernel128", [0, 1])
def test_gemm_qkv_three_segments_vt_and_scaled_q(kernel128):
    """the encoder's q|k|v GEMM: q scaled by NH_ENC_Q_SCALE, k plain, v as the V^T image with its 1536-column padding"""
    r = rng("gemm-qkv", kernel128)
    B, S, d = 2, 750, 512
    H, M = d // 64, 2 * 750
    A = K.f16(r.standard_normal((M, d)))
    W = K.f16(r.standard_normal((3 * d, d)) / np.sqrt(d))
    bias = K.f32(r.standard_normal(3 * d) * 0.5)
    pre, absdot = K.linear(A, W, bias)
    q = np.full((M, d), np.float16(7.25), np.float16); k = q.copy()
    vt = np.full((B, H, 64, K.NH_SP), np.float16(-3.5), np.float16)
    size = max(q.nbytes, vt.nbytes)
    bufs = [np.zeros(size // 2, np.float16) for _ in range(3)]
    bufs[0][:q.size] = q.ravel(); bufs[1][:k.size] = k.ravel(); bufs[2][:vt.size] = vt.ravel()
    _gemm(kernel128, A, d, M, 0, W, bias, M, K.EPI_F16, bufs, d, d, vt_seg=2, seg0_scale=K.ENC_Q_SCALE, S=S, H=H)
    sc = float(np.float32(K.ENC_Q_SCALE))
    bq = K.f16_out_bound(pre[:, :d] * sc, absdot[:, :d] * sc, d) + K.U32 * np.abs(pre[:, :d] * sc)
    K.within(bufs[0][:q.size].reshape(M, d), pre[:, :d] * sc, bq, "q segment (scaled)")
    K.within(bufs[1][:k.size].reshape(M, d), pre[:, d:2 * d], K.f16_out_bound(pre[:, d:2 * d], absdot[:, d:2 * d], d), "k segment")
    got_vt = bufs[2][:vt.size].reshape(B, H, 64, K.NH_SP)
    ref_vt = K.vt_image(pre[:, 2 * d:], H, S)
    b_vt = K.vt_image(K.f16_out_bound(pre[:, 2 * d:], absdot[:, 2 * d:], d), H, S)
    K.within(got_vt[..., :S], ref_vt[..., :S], b_vt[..., :S], "V^T segment")
    # what the V^T epilogue leaves in the pad: it never writes columns S..1535 (the attention kernel masks them)
    assert np.all(got_vt[..., S:] == np.float16(-3.5)), "V^T epilogue wrote into the pad columns"
    muts = _gemm_muts(pre[:, :d], A, W[:d], bias[:d], lambda v: v, M)
    K.discriminates(pre[:, :d] * sc, bq, {k_: v * sc for k_, v in muts.items()})
    # head mapping of V^T: the last head read through the previous head's slice
    wrong = ref_vt.copy(); wrong[:, -1] = ref_vt[:, -2]
    assert K.violation(ref_vt[..., :S], b_vt[..., :S], wrong[..., :S]) > 2


@pytest.mark.parametrize("kernel128", [0, 1])
@pytest.mark.parametrize("M,S", [(750, 750), (1500, 750), (4500, 1500)])
def test_gemm_cross_kv_head_major(kernel128, M, S):
    r = rng("gemm-hm", kernel128, M)
    d = 384
    H, B = d // 64, M // S
    A = K.f16(r.standard_normal((M, d)))
    W = K.f16(r.standard_normal((2 * d, d)) / np.sqrt(d))
    bias = K.f32(r.standard_normal(2 * d) * 0.5)
    pre, absdot = K.linear(A, W, bias)
    ck = np.full((B, H, S, 64), np.float16(7.25), np.float16); cv = ck.copy()
    _gemm(kernel128, A, d, M, 0, W, bias, M, K.EPI_F16, [ck, cv], d, d, head_major=1, S=S, H=H)
    bound = K.f16_out_bound(pre, absdot, d)
    for name, got, sl in [("k", ck, slice(0, d)), ("v", cv, slice(d, 2 * d))]:
        ref = K.head_major(pre[:, sl].reshape(B, S, d), H)
        K.within(got, ref, K.head_major(bound[:, sl].reshape(B, S, d), H), f"cross {name} head-major M={M}")
        wrong = ref.copy(); wrong[:, -1] = ref[:, -2]
        assert K.violation(ref, K.head_major(bound[:, sl].reshape(B, S, d), H), wrong) > 2
    K.discriminates(pre, bound, _gemm_muts(pre, A, W, bias, lambda v: v, M))


@pytest.mark.parametrize("kernel128", [0, 1])
@pytest.mark.parametrize("M,d,mult", [(777, 384, 4), (750, 1280, 4), (4500, 512, 4)])
def test_gemm_gelu_and_residual(kernel128, M, d, mult):
    """fc1 (EPI_GELU_F16, N = 4 d) and fc2 (EPI_RESID_F32 onto a random residual, K = 4 d)"""
    r = rng("gemm-mlp", kernel128, M, d)
    A = K.f16(r.standard_normal((M, d)))
    W1 = K.f16(r.standard_normal((mult * d, d)) / np.sqrt(d))
    b1 = K.f32(r.standard_normal(mult * d) * 0.5)
    pre, absdot = K.linear(A, W1, b1)
    hid = np.full((M, mult * d), np.float16(7.25), np.float16)
    _gemm(kernel128, A, d, M, 0, W1, b1, M, K.EPI_GELU_F16, [hid], mult * d, mult * d)
    bound = K.gelu_f16_bound(pre, absdot, d)
    K.within(hid, K.gelu(pre), bound, f"fc1 gelu M={M} d={d}")
    K.discriminates(K.gelu(pre), bound, _gemm_muts(pre, A, W1, b1, K.gelu, M))
    W2 = K.f16(r.standard_normal((d, mult * d)) / np.sqrt(mult * d))
    b2 = K.f32(r.standard_normal(d) * 0.5)
    x0 = K.f32(r.standard_normal((M, d)))
    pre2, absdot2 = K.linear(hid, W2, b2)
    x = x0.copy()
    _gemm(kernel128, hid, mult * d, M, 0, W2, b2, M, K.EPI_RESID_F32, [x], d, d)
    ref2 = pre2 + K.d64(x0)
    bound2 = K.f32_out_bound(ref2, absdot2, mult * d, extra=x0)
    K.within(x, ref2, bound2, f"fc2 resid M={M} d={d}")
    K.discriminates(ref2, bound2, _gemm_muts(pre2, hid, W2, b2, lambda v: v + K.d64(x0), M))


@pytest.mark.parametrize("kernel128", [0, 1])
def test_gemm_conv_epilogues_with_row_maps(kernel128):
    """conv1 (EPI_GELU_F16, overlapping A rows inside the zero-framed mel image, output rows offset by one inside [F+2] frames)
    and conv2 (EPI_CONV2_F32: stride-2 A rows, gelu + pos[m % S]) with a_rpb / o_rpb as nh_encode_rows sets them; conv1 at
    M = 33 clips x 1500 frames = 49500 rows"""
    r = rng("gemm-conv", kernel128)
    d, B, F = 384, 33, 1500
    S = F // 2
    mel = np.zeros((B, F + 2, 128), np.float16)
    mel[:, 1:F + 1, :] = K.f16(r.standard_normal((B, F, 128)))   # all 128 channels: the last k-step carries data
    W1 = K.f16(r.standard_normal((d, 3 * 128)) / np.sqrt(384))
    b1 = K.f32(r.standard_normal(d) * 0.5)
    A1 = np.stack([mel[:, j:j + F, :] for j in range(3)], axis=2).reshape(B * F, 3 * 128)   # row (b, f) = frames f..f+2
    pre1, abs1 = K.linear(A1, W1, b1)
    h1 = np.full((B, F + 2, d), np.float16(7.25), np.float16)
    _gemm(kernel128, mel, 128, F, (F + 2) * 128, W1, b1, B * F, K.EPI_GELU_F16, [h1], d, d, o_rpb=F, o_bstride=F + 2, o_off=1)
    bound1 = K.gelu_f16_bound(pre1, abs1, 3 * 128)
    K.within(h1[:, 1:F + 1].reshape(B * F, d), K.gelu(pre1), bound1, "conv1")
    assert np.all(h1[:, 0] == np.float16(7.25)) and np.all(h1[:, F + 1] == np.float16(7.25)), "conv1 wrote a frame border"
    K.discriminates(K.gelu(pre1), bound1, _gemm_muts(pre1, A1, W1, b1, K.gelu, B * F))
    # conv2 on two clips of that image (frame borders zero)
    B2 = 2
    h = np.zeros((B2, F + 2, d), np.float16)
    h[:, 1:F + 1] = K.f16(r.standard_normal((B2, F, d)))
    W2 = K.f16(r.standard_normal((d, 3 * d)) / np.sqrt(3 * d))
    b2 = K.f32(r.standard_normal(d) * 0.5)
    pos = K.f32(r.standard_normal((S, d)))
    A2 = np.stack([h[:, 2 * np.arange(S) + j, :] for j in range(3)], axis=2).reshape(B2 * S, 3 * d)
    pre2, abs2 = K.linear(A2, W2, b2)
    x = np.full((B2 * S, d), np.float32(7.25), np.float32)
    _gemm(kernel128, h, 2 * d, S, (F + 2) * d, W2, b2, B2 * S, K.EPI_CONV2_F32, [x], d, d, S=S, pos=pos)
    posr = np.tile(K.d64(pos), (B2, 1))
    ref2 = K.gelu(pre2) + posr
    bound2 = K.gelu_f16_bound(pre2, abs2, 3 * d) - K.U16 * np.abs(K.gelu(pre2)) - K.SUB16 + K.U32 * (np.abs(ref2) + np.abs(posr))
    K.within(x, ref2, bound2, "conv2")
    muts = _gemm_muts(pre2, A2, W2, b2, lambda v: K.gelu(v) + posr, B2 * S)
    muts["pos[m] instead of pos[m % S]"] = K.gelu(pre2) + np.concatenate([K.d64(pos), np.roll(K.d64(pos), 1, axis=0)])
    K.discriminates(ref2, bound2, muts)


# launch_gemm as prefill_forward calls it (nh_prefill.hip pf_gemm): M = B * T rows from 1 upward, a_rpb = o_rpb = S = M, so all
# three nh_magic values are 0, the "quotient 0" encoding of nh_div.  Which kernel launch_gemm (kernel128 = 0) reaches, from
# its condition `N % 256 == 0 && K % 128 == 0 && seg_ok && M >= 256` (seg_ok: seg_n % 256 == 0 under the fp16 epilogues; every
# shape here has N, K and seg_n multiples of 256):
#   M = 1, 3, 127, 128, 129, 255   gemm_f16_kernel (128 x 128 tiles): one partial row tile up to 127, one full at 128, one full + one
#                                  ragged at 129 and 255
#   M = 256, 257, 511              gemm256_f16_kernel<EPI>: one full tile at 256, one full + one ragged at 257 (1 row) and 511 (255)
# From M = 256 on kernel128 = 1 runs the 128 x 128 kernel on the same shape too; below, both launchers reach that kernel.
PF_GEMM = [(M, 256) for M in (1, 3, 127, 128, 129, 255, 256, 257, 511)] + [(3, 1280), (257, 1280)]
PF_GEMM_CASES = [(k128, M, d) for M, d in PF_GEMM for k128 in ((0, 1) if M >= 256 else (0,))]


def _reaches_gemm256(M, N, Kd, epi, seg_n):
    """launch_gemm's dispatch condition (k_gemm.hip), restated"""
    seg_ok = epi not in (K.EPI_F16, K.EPI_GELU_F16) or seg_n % 256 == 0
    return N % 256 == 0 and Kd % 128 == 0 and seg_ok and M >= 256


def test_prefill_gemm_cases_sit_on_both_sides_of_the_dispatch_edge():
    through_launch_gemm = [(M, d) for k128, M, d in PF_GEMM_CASES if k128 == 0]
    for N_of, K_of, epi in ((lambda d: 3 * d, lambda d: d, K.EPI_F16), (lambda d: 4 * d, lambda d: d, K.EPI_GELU_F16),
                            (lambda d: d, lambda d: 4 * d, K.EPI_RESID_F32)):
        big = {M for M, d in through_launch_gemm if _reaches_gemm256(M, N_of(d), K_of(d), epi, d if epi == K.EPI_F16 else N_of(d))}
        small = {M for M, d in through_launch_gemm} - big
        assert {256, 257, 511} <= big and {1, 3, 127, 128, 129, 255} <= small and max(small) + 1 == min(big) == 256


def _canary_rows(M, n, dtype, value=7.25):
    """an output buffer of M + 1 rows: the row past M must come back untouched"""
    return np.full((M + 1, n), value, dtype=dtype)


@pytest.mark.parametrize("kernel128,M,d", PF_GEMM_CASES)
def test_gemm_at_prefill_shapes_plain_qkv_gelu_and_residual(kernel128, M, d):
    """the prefill's three epilogues: q | k | v as three plain row-major fp16 segments (EPI_F16, seg_n = ldo = d, no V^T, no
    head-major, no q scale), fc1 (EPI_GELU_F16, N = 4 d) and fc2 (EPI_RESID_F32, K = 4 d), every output with a canary row past M"""
    r = rng("pf-gemm", M, d)                     # both launchers see the same data
    H = d // 64
    A = K.f16(r.standard_normal((M, d)))
    W = K.f16(r.standard_normal((3 * d, d)) / np.sqrt(d))
    bias = K.f32(r.standard_normal(3 * d) * 0.5)
    pre, absdot = K.linear(A, W, bias)
    bound = K.f16_out_bound(pre, absdot, d)
    K.discriminates(pre, bound, _gemm_muts(pre, A, W, bias, lambda v: v, M))
    swapped = np.concatenate([pre[:, d:2 * d], pre[:, :d], pre[:, 2 * d:]], axis=1)
    K.discriminates(pre, bound, {"segments 0 and 1 swapped": swapped})
    outs = [_canary_rows(M, d, np.float16) for _ in range(3)]
    _gemm(kernel128, A, d, M, 0, W, bias, M, K.EPI_F16, outs, d, d, o_rpb=M, S=M, H=H)
    for s_, name in enumerate("qkv"):
        _pf_report("gemm qkv", outs[s_][:M], pre[:, s_ * d:(s_ + 1) * d], bound[:, s_ * d:(s_ + 1) * d])
        K.within(outs[s_][:M], pre[:, s_ * d:(s_ + 1) * d], bound[:, s_ * d:(s_ + 1) * d], f"prefill {name} segment M={M} d={d}")
        assert np.all(outs[s_][M] == np.float16(7.25)), f"prefill {name} segment M={M}: wrote the row past M"
    # fc1 / fc2
    W1 = K.f16(r.standard_normal((4 * d, d)) / np.sqrt(d))
    b1 = K.f32(r.standard_normal(4 * d) * 0.5)
    pre1, abs1 = K.linear(A, W1, b1)
    bound1 = K.gelu_f16_bound(pre1, abs1, d)
    K.discriminates(K.gelu(pre1), bound1, _gemm_muts(pre1, A, W1, b1, K.gelu, M))
    hid = _canary_rows(M, 4 * d, np.float16)
    _gemm(kernel128, A, d, M, 0, W1, b1, M, K.EPI_GELU_F16, [hid], 4 * d, 4 * d, o_rpb=M, S=M, H=H)
    _pf_report("gemm gelu", hid[:M], K.gelu(pre1), bound1)
    K.within(hid[:M], K.gelu(pre1), bound1, f"prefill fc1 M={M} d={d}")
    assert np.all(hid[M] == np.float16(7.25)), f"prefill fc1 M={M}: wrote the row past M"
    W2 = K.f16(r.standard_normal((d, 4 * d)) / np.sqrt(4 * d))
    b2 = K.f32(r.standard_normal(d) * 0.5)
    h_in = np.ascontiguousarray(hid[:M])
    x0 = K.f32(r.standard_normal((M, d)))
    pre2, abs2 = K.linear(h_in, W2, b2)
    ref2 = pre2 + K.d64(x0)
    bound2 = K.f32_out_bound(ref2, abs2, 4 * d, extra=x0)
    K.discriminates(ref2, bound2, _gemm_muts(pre2, h_in, W2, b2, lambda v: v + K.d64(x0), M))
    x = _canary_rows(M, d, np.float32)
    x[:M] = x0
    _gemm(kernel128, h_in, 4 * d, M, 0, W2, b2, M, K.EPI_RESID_F32, [x], d, d, o_rpb=M, S=M, H=H)
    _pf_report("gemm resid", x[:M], ref2, bound2)
    K.within(x[:M], ref2, bound2, f"prefill fc2 M={M} d={d}")
    assert np.all(x[M] == np.float32(7.25)), f"prefill fc2 M={M}: wrote the row past M"


# ---- LayerNorm and embed ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sliced", [0, 1])
@pytest.mark.parametrize("M", [1, 17, 96, 3000])
def test_layernorm_matches_fp64(sliced, M):
    """layernorm_kernel / layernorm_sliced_kernel (K % 128 == 0, <= 1280), fp16 and f32 outputs; rows with a large mean and a
    tiny variance (1000 + 1e-3 noise) and a constant row"""
    L = K.lib()
    for Kd in [128, 384, 640, 1280]:
        r = rng("ln", sliced, M, Kd)
        x = K.f32(r.standard_normal((M, Kd)) * 2.0 + 0.5)
        if M > 1:
            x[-1] = np.float32(1000.0) + K.f32(r.standard_normal(Kd) * 1e-3)
            x[M // 2] = np.float32(-2.75)
        w, b = K.f32(1.0 + 0.1 * r.standard_normal(Kd)), K.f32(0.1 * r.standard_normal(Kd))
        y = np.full((M, Kd), np.float16(7.25), np.float16)
        y32 = np.full((M, Kd), np.float32(7.25), np.float32)
        rc = L.kref_layernorm(sliced, K.ptr(x), K.ptr(w), K.ptr(b), K.ptr(y), K.ptr(y32), M, Kd)
        K.check_rc(rc, f"layernorm sliced={sliced} M={M} K={Kd}")
        b16, ref = K.ln_f16_bound(x, w, b)
        b32, _ = K.ln_act_bound(x, w, b)
        K.within(y, ref, b16, f"layernorm fp16 sliced={sliced} M={M} K={Kd}")
        K.within(y32, ref, b32, f"layernorm f32 sliced={sliced} M={M} K={Kd}")
        muts = {"last 128 columns left out of the statistics": _ln_partial(x, w, b, Kd - 128) if Kd > 128 else None,
                "gamma / beta of the last 4 columns missing": np.concatenate([ref[:, :-4], K.d64(np.broadcast_to(
                    (ref[:, -4:] - K.d64(b[-4:])) / K.d64(w[-4:]), (M, 4)))], axis=1)}
        if M > 1:
            nr = ref.copy(); nr[M - 2] = ref[M - 1]
            muts["row reads the next row"] = nr
        K.discriminates(ref, b16, {k: v for k, v in muts.items() if v is not None})


def _ln_partial(x, w, b, n):
    x = K.d64(x)
    m = x[:, :n].mean(axis=1, keepdims=True)
    var = ((x[:, :n] - m) ** 2).mean(axis=1, keepdims=True)
    return (x - m) / np.sqrt(var + 1e-5) * K.d64(w) + K.d64(b)


def test_embed_matches_fp64():
    """embed_kernel: x = E[token] + P[position] in f32; token ids 0 and V - 1; per-row positions through pos_ptr; and the
    prefill's call: Tn > 1 positions per clip from t0 = 0 without pos_ptr, row b * Tn + i = token (b, i) at position i"""
    L = K.lib()
    r = rng("embed")
    V, d, C, B = 51866, 384, 448, 7
    E = K.f16(r.standard_normal((V, d)))
    P = K.f16(r.standard_normal((C, d)))
    tokens = np.ascontiguousarray(r.integers(0, V, (B, C)), dtype=np.int32)
    pos = np.ascontiguousarray([0, 447, 3, 200, 1, 446, 17], dtype=np.int32)
    tokens[0, 0] = 0; tokens[1, 447] = V - 1; tokens[2, 3] = V - 1
    for pp, t0 in [(None, 5), (pos, 0)]:
        x = np.full((B, d), np.float32(7.25), np.float32)
        rc = L.kref_embed(K.ptr(tokens), C, K.ptr(E), V, K.ptr(P), C, K.ptr(x), B, 1, t0, K.ptr(pp), d)
        K.check_rc(rc, "embed")
        at = pos if pp is not None else np.full(B, t0)
        ref = K.d64(E[tokens[np.arange(B), at]]) + K.d64(P[at])
        bound = K.U32 * np.abs(ref)   # one f32 addition of two exact values
        K.within(x, ref, bound, f"embed pos_ptr={pp is not None}")
        off = at.copy(); off[1] = at[1] - 1
        wrong = K.d64(E[tokens[np.arange(B), off]]) + K.d64(P[off])
        assert K.violation(ref, bound + K.SUB16, wrong) > 2
    tokens[3, 1] = 0; tokens[B - 1, 222] = V - 1
    for Tn in (2, 33, 223):
        x = np.full((B * Tn + 1, d), np.float32(7.25), np.float32)      # one canary row past the last
        rc = L.kref_embed(K.ptr(tokens), C, K.ptr(E), V, K.ptr(P), C, K.ptr(x), B, Tn, 0, None, d)
        K.check_rc(rc, f"embed Tn={Tn}")
        i = np.arange(Tn)
        ref = (K.d64(E[tokens[:, :Tn]]) + K.d64(P[:Tn])[None]).reshape(B * Tn, d)
        bound = K.U32 * np.abs(ref)
        _pf_report("embed", x[:B * Tn], ref, np.maximum(bound, 1e-300))
        K.within(x[:B * Tn], ref, bound, f"embed Tn={Tn}")
        assert np.all(x[B * Tn] == np.float32(7.25)), f"embed Tn={Tn}: wrote past the last row"
        im = np.maximum(i - 1, 0)
        muts = {"row (b, i) takes clip b's token at i - 1": (K.d64(E[tokens[:, im]]) + K.d64(P[:Tn])[None]).reshape(B * Tn, d),
                "rows position-major (row r = clip r % B at position r // B)":
                    K.d64(E[tokens[np.arange(B * Tn) % B, np.arange(B * Tn) // B]]) + K.d64(P[np.arange(B * Tn) // B])}
        K.discriminates(ref, bound + K.SUB16, muts)
