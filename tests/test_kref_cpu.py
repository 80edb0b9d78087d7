"""CPU: the fp64 references of tests/kref.py against naive loops on small shapes, the layout maps, the discrimination logic,
and the build of tools/bin/libnh_kref.so (hipcc cross-compiles without a GPU)."""
import os
import subprocess

import numpy as np
import pytest

import kref as K


def _r(seed):
    return np.random.default_rng(seed)


def test_linear_and_gelu_match_naive_loops():
    r = _r(1)
    x, W, b = r.standard_normal((3, 40)), r.standard_normal((5, 40)), r.standard_normal(5)
    y, a = K.linear(x, W, b)
    for i in range(3):
        for n in range(5):
            assert abs(y[i, n] - (sum(x[i, k] * W[n, k] for k in range(40)) + b[n])) < 1e-12
            assert abs(a[i, n] - sum(abs(x[i, k] * W[n, k]) for k in range(40))) < 1e-12
    assert np.allclose(np.einsum("rk,nk->rn", x, W) + b, y, rtol=0, atol=1e-12)
    v = np.linspace(-6, 6, 101)
    assert np.allclose(K.gelu(v), v / (1 + np.exp(-2 * np.sqrt(2 / np.pi) * (v + 0.044715 * v ** 3))), rtol=1e-13, atol=1e-15)


def _naive_attn(q, k, v, scale):
    s = [scale * float(np.dot(q, kk)) for kk in k]
    m = max(s)
    p = [np.exp(x - m) for x in s]
    z = sum(p)
    return sum(pi * vv for pi, vv in zip(p, v)) / z


def test_dec_attention_is_an_explicit_softmax():
    r = _r(2)
    B, H, T = 3, 2, 11
    q, k, v = r.standard_normal((B, 128)), r.standard_normal((B, T, 128)), r.standard_normal((B, T, 128))
    nvis = [1, 5, 11]
    o, sabs, (vdev, pv) = K.dec_attention(q, k, v, H, nvis)
    for b in range(B):
        for h in range(H):
            c = slice(64 * h, 64 * h + 64)
            want = _naive_attn(q[b, c], k[b, :nvis[b], c], v[b, :nvis[b], c], 1 / 8)
            assert np.allclose(o[b, c], want, rtol=0, atol=1e-12)
            assert np.isclose(sabs[b, h], max(np.abs(q[b, c]) @ np.abs(k[b, j, c]) for j in range(nvis[b])) / 8)
            s_ = k[b, :nvis[b], c] @ q[b, c] / 8
            p_ = np.exp(s_ - s_.max()); p_ /= p_.sum()
            assert np.allclose(vdev[b, h], p_ @ np.abs(v[b, :nvis[b], c] - want), rtol=0, atol=1e-12)
            assert np.allclose(pv[b, h], p_ @ np.abs(v[b, :nvis[b], c]), rtol=0, atol=1e-12)


def test_enc_attention_uses_exp2_of_prescaled_scores():
    r = _r(3)
    B, S, H = 2, 9, 1
    q, k, v = r.standard_normal((B * S, 64)), r.standard_normal((B * S, 64)), r.standard_normal((B * S, 64))
    o, _, _ = K.enc_attention(q, k, v, B, S, H)
    for b in range(B):
        for i in range(S):
            rs = slice(b * S, (b + 1) * S)
            s = np.array([np.dot(q[b * S + i], kk) for kk in k[rs]])
            p = 2.0 ** (s - s.max())
            assert np.allclose(o[b * S + i], p @ v[rs] / p.sum(), rtol=0, atol=1e-12)


def test_xabs_reference_is_attention_on_projected_kv():
    r = _r(4)
    B, d, S = 2, 128, 13
    H = d // 64
    q, Wkv, bkv, xa = r.standard_normal((B, d)), r.standard_normal((2 * d, d)) / 10, r.standard_normal(2 * d), r.standard_normal((B, S, d))
    o = K.xabs_attention(q, Wkv, bkv, xa, H)
    Kp, Vp = xa @ Wkv[:d].T + bkv[:d], xa @ Wkv[d:].T + bkv[d:]
    for b in range(B):
        for h in range(H):
            c = slice(64 * h, 64 * h + 64)
            assert np.allclose(o[b, c], _naive_attn(q[b, c], Kp[b, :, c], Vp[b, :, c], 1 / 8), rtol=0, atol=1e-10)


def test_layout_maps():
    r = _r(5)
    B, T, H, S = 2, 5, 3, 7
    kv = r.standard_normal((B, T, 64 * H))
    hm = K.head_major(kv, H)
    for b, t, h, c in [(0, 0, 0, 0), (1, 4, 2, 63), (1, 2, 1, 17)]:
        assert hm[b, h, t, c] == kv[b, t, 64 * h + c]
    assert np.array_equal(hm.transpose(0, 2, 1, 3).reshape(B, T, 64 * H), kv)
    v = r.standard_normal((B * S, 64 * H))
    vt = K.vt_image(v, H, S)
    assert vt.shape == (B, H, 64, K.NH_SP)
    for b, s, h, c in [(0, 0, 0, 0), (1, 6, 2, 63), (1, 3, 1, 5)]:
        assert vt[b, h, c, s] == v[b * S + s, 64 * h + c]
    assert not vt[:, :, :, S:].any()


def test_layernorm_reference_and_bound():
    r = _r(6)
    x = r.standard_normal((4, 256)) * 3 + 1
    x[3] = 1000 + r.standard_normal(256) * 1e-3
    w, b = 1 + 0.1 * r.standard_normal(256), 0.1 * r.standard_normal(256)
    y, inv, t = K.layernorm(x, w, b)
    for i in range(4):
        m = sum(x[i]) / 256
        var = sum((xx - m) ** 2 for xx in x[i]) / 256
        assert np.allclose(y[i], (x[i] - m) / np.sqrt(var + 1e-5) * w + b, rtol=0, atol=1e-9)
    # an f32 evaluation of the same LayerNorm stays inside the f32 bound
    x32 = x.astype(np.float32)
    m = x32.mean(axis=1, keepdims=True, dtype=np.float32)
    tt = x32 - m
    inv32 = np.float32(1) / np.sqrt((tt * tt).mean(axis=1, keepdims=True, dtype=np.float32) + np.float32(1e-5))
    y32 = tt * inv32 * w.astype(np.float32) + b.astype(np.float32)
    e, yref = K.ln_act_bound(x32, w.astype(np.float32), b.astype(np.float32))
    assert np.all(np.abs(y32 - yref) <= e)


def test_fp16_rounding_stays_inside_the_output_bound():
    """the bound's first term is the output rounding: rounding the exact reference to fp16 must stay inside it"""
    r = _r(7)
    x, W = r.standard_normal((6, 96)).astype(np.float16), (r.standard_normal((50, 96)) / 10).astype(np.float16)
    ref, a = K.linear(x, W)
    b = K.f16_out_bound(ref, a, 96)
    assert np.all(np.abs(ref.astype(np.float16).astype(np.float64) - ref) <= b)
    acc = (x.astype(np.float32) @ W.astype(np.float32).T).astype(np.float16)   # an f32 accumulation, then fp16
    assert np.all(np.abs(acc - ref) <= b)


def test_discrimination_flags_each_mutation():
    r = _r(8)
    R, N, Kd = 17, 48, 256
    x = r.standard_normal((R, Kd)).astype(np.float16)
    W = (r.standard_normal((N, Kd)) / 16).astype(np.float16)
    bias = (r.standard_normal(N) * 0.5).astype(np.float32)
    ref, a = K.linear(x, W, bias)
    bound = K.f16_out_bound(ref, a, Kd)
    drop = ref - K.d64(x[:, -32:]) @ K.d64(W[:, -32:]).T
    nb = ref.copy(); nb[:, 32:] -= bias[32:]
    nr = ref.copy(); nr[R - 2] = ref[R - 1]
    got = K.discriminates(ref, bound, {"drop": drop, "bias": nb, "row": nr})
    assert all(v > 2 for v in got.values())
    with pytest.raises(AssertionError, match="too loose"):
        K.discriminates(ref, bound, {"harmless": ref + 0.5 * bound})
    # attention: one key too few / too many, the wrong head's V
    q, k, v = r.standard_normal((3, 128)), r.standard_normal((3, 40, 128)), r.standard_normal((3, 40, 128))
    o, sabs, vst = K.dec_attention(q, k, v, 2, [30] * 3)
    ab = K.attn_bound(o, sabs, [30] * 3, vst)
    vs = v.copy(); vs[:, :, 64:] = v[:, :, :64]
    K.discriminates(o, ab, {"few": K.dec_attention(q, k, v, 2, [29] * 3)[0], "many": K.dec_attention(q, k, v, 2, [31] * 3)[0],
                            "head": K.dec_attention(q, k, vs, 2, [30] * 3)[0]})
    with pytest.raises(AssertionError, match="outside the bound"):
        K.within(o + 3 * ab, o, ab, "shifted")


def _make_wrapper_library():
    root = K.ROOT
    if not os.path.exists(os.path.join(root, "norma_amd", "csrc", "build", "k_skinny.o")):
        subprocess.check_call(["make", "-C", os.path.join(root, "norma_amd", "csrc"), "-j8"])
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", ), "bin/libnh_kref.so"], stdout=subprocess.DEVNULL)


def test_make_builds_the_wrapper_library_with_every_entry_point():
    import pool_ref
    _make_wrapper_library()
    subprocess.check_call(["make", "-C", os.path.join(K.ROOT, "tools"), "bin/libnh_kref_pool.so"], stdout=subprocess.DEVNULL)
    for path, wrappers in ((K.LIB_PATH, K.WRAPPERS), (pool_ref.LIB_PATH, pool_ref.WRAPPERS)):   # the pool step's library too
        assert os.path.exists(path)
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
        assert set(wrappers) <= exported, set(wrappers) - exported


# ---- the decode GEMV dispatch (norma_amd/csrc/skinny_plan.h), asked through the wrapper library: pure host code, no GPU ------
PLAN_WIDTHS = [128, 256, 384, 512, 640, 768, 1024, 1280]


def _plan_shapes(d):
    return [(d, d), (3 * d, d), (4 * d, d), (d, 4 * d), (51864, d), (51865, d), (51866, d)]


def _plan_epilogues(N, d):
    """every epilogue valid for the shape: all but SK_F32 store 4 features at a time, SK_QKV cuts N into q | k | v of width d"""
    epis = [K.SK_F32]
    if N % 4 == 0:
        epis += [K.SK_F16, K.SK_GELU_F16, K.SK_RESID_F32]
    if N == 3 * d:
        epis.append(K.SK_QKV)
    return epis


def _ln_expected(R, N, Kd):
    """where a fused LayerNorm exists, written out independently of the plan: below 2048 weight tiles skinny_ln_kernel for
    K = 128 STEPS, STEPS in {1, 2, 3, 4, 6, 8, 10}, any R <= 96; for the logits the staging pass of skinny_lds_kernel, R <= 32,
    K = 128 steps with steps <= 10"""
    if (N + 15) // 16 < 2048:
        return R <= 96 and Kd % 128 == 0 and Kd // 128 in (1, 2, 3, 4, 6, 8, 10)
    return R <= 32 and Kd % 128 == 0 and Kd <= 1280


def _check_launchable(pl, R, N, Kd, wt, ln, what):
    tiles = (N + 15) // 16
    assert pl["grid_x"] >= 1 and pl["grid_y"] >= 1, what
    assert pl["block"] in (128, 256, 512, 1024), what
    assert 0 <= pl["lds_used"] <= 160 * 1024, what
    assert pl["ksplit"] >= 1 and Kd % (pl["ksplit"] * 32) == 0, what
    assert pl["grid_y"] * 16 * pl["ncb"] >= R, what
    kind = pl["kind"]
    if kind == K.SKP_GEMM:
        # K-sliced: one tile per workgroup, its ksplit waves split K; full rows (ksplit 1): 2 waves of nt tiles each
        per_wg = pl["nt"] if pl["ksplit"] > 1 else 2 * pl["nt"]
        assert pl["block"] == (128 if pl["ksplit"] == 1 else 64 * pl["ksplit"]), what
        assert 1 <= pl["ncb"] <= 4 and pl["lds_used"] == 0 and not pl["lds_exclusive"] and not ln, what
    elif kind == K.SKP_LN:
        per_wg = pl["nt"]
        assert ln and pl["block"] == 256 and pl["ncb"] == 1 and pl["ksplit"] * 128 == Kd and pl["nt"] in (1, 2), what
    elif kind == K.SKP_LDS:
        per_wg = tiles                     # its 8 waves per workgroup walk the tiles grid-stride: any grid covers N
        assert pl["block"] == 512 and pl["ncb"] in (1, 2) and pl["lds_exclusive"], what
        assert pl["lds_used"] == (Kd // 32) * 16 * pl["ncb"] * 64 <= 96 * 1024, what
    else:
        assert kind == K.SKP_LDSP, what
        per_wg = 8 * pl["nt"]              # 8 waves of at most LP_MT = nt tiles each
        assert wt and not ln and pl["block"] == 512 and 3 <= pl["ncb"] <= 6 and pl["lds_exclusive"], what
        assert 1 <= pl["sp"] and pl["lds_used"] == pl["sp"] * 16 * pl["ncb"] * 64 <= 144 * 1024, what
    assert pl["grid_x"] * per_wg >= tiles, what


def test_skinny_plan_covers_every_decoder_shape_and_is_launchable():
    """the sweep of every row count x width x decoder shape x weight layout x epilogue, with and without the fused LayerNorm:
    without LayerNorm nothing is refused (the hole 9a04a41 closed: 65-96 rows on >= 2048 tiles without tile-major weights had
    no kernel); with it, exactly the shapes _ln_expected names are planned, whatever the layout and the epilogue; and every
    plan can be launched as it stands"""
    _make_wrapper_library()
    L = K.lib()
    n_plans, ln_yes, ln_no, kinds = 0, 0, 0, set()
    for d in PLAN_WIDTHS:
        for N, Kd in _plan_shapes(d):
            for R in range(1, 97):
                want_ln = _ln_expected(R, N, Kd)
                assert bool(L.kref_skinny_ln_supported(R, N, Kd)) == want_ln, (R, N, Kd)
                ln_yes, ln_no = ln_yes + want_ln, ln_no + (not want_ln)
                for wt in (0, 1):
                    for epi in _plan_epilogues(N, d):
                        for ln in (0, 1):
                            what = f"R={R} N={N} K={Kd} epi={epi} wt={wt} ln={ln}"
                            pl = K.skinny_plan(R, N, Kd, epi, wt, ln)
                            if ln:
                                assert (pl["kind"] != K.SKP_NONE) == want_ln, what
                                if not want_ln:
                                    continue
                                assert pl["kind"] in (K.SKP_LN, K.SKP_LDS), what
                            else:
                                assert pl["kind"] != K.SKP_NONE, what
                            _check_launchable(pl, R, N, Kd, wt, ln, what)
                            n_plans += 1
                            kinds.add((pl["kind"], pl["ncb"], pl["nt"], pl["ksplit"]))
    assert ln_yes > 0 and ln_no > 0, (ln_yes, ln_no)      # the sweep holds both outcomes (d = 640 has no skinny_ln_kernel)
    assert not L.kref_skinny_ln_supported(17, 640, 640) and not L.kref_skinny_ln_supported(33, 51866, 1280)
    assert L.kref_skinny_ln_supported(32, 51866, 1280) and L.kref_skinny_ln_supported(96, 3840, 1280)
    assert {k[0] for k in kinds} == {K.SKP_GEMM, K.SKP_LN, K.SKP_LDS, K.SKP_LDSP}, kinds
    # the former hole: K-sliced rows split over grid.y
    for R in (65, 80, 96):
        pl = K.skinny_plan(R, 51866, 1280, K.SK_F32, 0, 0)
        assert (pl["kind"], pl["ncb"], pl["ksplit"], pl["grid_x"], pl["grid_y"]) == (K.SKP_GEMM, 1, 4, 3242, (R + 15) // 16), pl
    print(f"{n_plans} plans, {len(kinds)} distinct (kind, ncb, nt, ksplit)")


def test_skinny_plan_refuses_what_the_kernels_cannot_compute():
    _make_wrapper_library()
    none = K.SKP_NONE
    assert K.skinny_plan(16, 1280, 96, K.SK_F16, 0, 0)["kind"] == none          # K % 64 != 0: the tail of K would be dropped
    assert K.skinny_plan(16, 1280, 96, K.SK_F32, 1, 0)["kind"] == none
    assert K.skinny_plan(16, 6, 128, K.SK_F16, 0, 0)["kind"] == none            # 4 features per store: N % 4 != 0
    assert K.skinny_plan(16, 6, 128, K.SK_F32, 0, 0)["kind"] == K.SKP_GEMM      # SK_F32 stores the ragged tail one by one
    assert K.skinny_plan(16, 1280, 192, K.SK_F16, 0, 0)["ksplit"] == 2          # K % 64 == 0 is enough: two slices of 3 k-steps
    for R in (0, -1, 97):
        assert K.skinny_plan(R, 1280, 1280, K.SK_F16, 1, 0)["kind"] == none
    assert K.skinny_plan(33, 51866, 1280, K.SK_F32, 1, 1)["kind"] == none       # no fused LayerNorm for the phased logits kernel
    assert K.skinny_plan(17, 640, 640, K.SK_F16, 1, 1)["kind"] == none          # K / 128 = 5: no such skinny_ln_kernel


def test_xabs_bound_holds_for_an_f32_fp16_emulation_of_the_kernels():
    """xabs_reference: the formula, and a bound that an emulation of the kernels' roundings (u, P, z and the output in fp16,
    sums in f32) stays inside, while it is no looser than needed to catch a key too few"""
    r = _r(9)
    B, d, S = 2, 128, 50
    H = d // 64
    q = (r.standard_normal((B, d)) * 3).astype(np.float16)
    Wkv = (r.standard_normal((2 * d, d)) / np.sqrt(d)).astype(np.float16)
    bkv = (r.standard_normal(2 * d) * 0.5).astype(np.float32)
    xa = r.standard_normal((B, S, d)).astype(np.float16)
    ref, bound = K.xabs_reference(q, Wkv, bkv, xa, H)
    assert np.allclose(ref, K.xabs_attention(q, Wkv, bkv, xa, H), rtol=0, atol=1e-12)
    f = np.float32
    out = np.zeros((B, d))
    for b in range(B):
        for h in range(H):
            Wk, Wv = Wkv[64 * h:64 * h + 64].astype(f), Wkv[d + 64 * h:d + 64 * h + 64].astype(f)
            u = (f(0.125) * (Wk.T @ q[b, 64 * h:64 * h + 64].astype(f))).astype(np.float16).astype(f)
            s = xa[b].astype(f) @ u
            p = np.exp(s - s.max()).astype(np.float16).astype(f)
            z = ((p @ xa[b].astype(f)) / p.sum()).astype(np.float16).astype(f)
            out[b, 64 * h:64 * h + 64] = (Wv @ z + bkv[d + 64 * h:d + 64 * h + 64]).astype(np.float16)
    K.within(out, ref, bound, "emulated absorbed attention")
    assert K.violation(ref, bound, K.xabs_attention(q, Wkv, bkv, xa[:, :-1], H)) > 0


# ---- enc_attn_kernel's deferred-maximum rebase: replay, cases, bound, emulation, mutations -----------------------------------
def test_enc_rebase_replay_is_the_per_query_rule():
    """the vectorised replay against a loop over queries, tiles and keys on a small ramp (rebases, quiet tiles, a partial tile)"""
    r = _r(20)
    S, H = 150, 2
    u = r.standard_normal((H, 64)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
    q = r.standard_normal((S, H, 64)) * K.ENC_Q_SCALE + np.array([11.0, 3.0, 0.0, -11.0])[np.arange(S) % 4][:, None, None] * u
    k = r.standard_normal((S, H, 64)) + (np.arange(S) // 64)[:, None, None] * u
    q, k = K.f16(q.reshape(S, 128)), K.f16(k.reshape(S, 128))
    rep = K.enc_rebase_replay(q, k, S, H)
    assert rep["rebase"].shape == (S, H, 3) and rep["rebase"][:, :, 0].all()
    seen = set()
    for i in range(S):
        for h in range(H):
            s = [float(np.dot(K.d64(q[i, 64 * h:64 * h + 64]), K.d64(kk[64 * h:64 * h + 64]))) for kk in k]
            m = max(s[:64])
            pmax, mabs = 0.0, abs(m)
            for t in (1, 2):
                tile = s[64 * t:64 * t + 64]
                gap = max(tile) - m
                assert np.isclose(rep["gap"][i, h, t], gap, rtol=0, atol=1e-9) and rep["pos"][i, h, t] == int(np.argmax(tile))
                assert rep["rebase"][i, h, t] == (gap > 8.0)
                seen.add(bool(gap > 8.0))
                if gap > 8.0:
                    m = max(tile)
                elif rep["decided"][i, h, t]:
                    pmax = max(pmax, 2.0 ** gap)
                mabs = max(mabs, abs(m))
            assert np.isclose(rep["m_final"][i, h], m) and np.isclose(rep["m_absmax"][i, h], mabs)
            assert np.isclose(rep["p_max"][i, h], pmax)
            assert rep["top_tile"][i, h] == int(np.argmax(s)) // 64
            assert np.isclose(rep["margin"][i, h], sorted(s)[-1] - sorted(s)[-2])
    assert seen == {True, False}
    # near / decided: a gap within 2 e of the threshold is undecided, and so is every later tile of that query.  Two keys that
    # score 16 and 24 + 2^-13 for every query (e = 64 u 24 + ..: 1e-4): tile 1 is near, tile 2 (gap -8 or 8 - 1e-4) inherits it
    q2, k2 = np.zeros((130, 64), np.float16), np.zeros((130, 64), np.float16)
    q2[:, 0], k2[5, 0], k2[70, 0], k2[70, 1] = 4.0, 4.0, 6.0, 1.0
    q2[:, 1] = 2.0 ** -13
    rep2 = K.enc_rebase_replay(q2, k2, 130, 1)
    assert np.allclose(rep2["gap"][:, 0, 1], 8.0 + 2.0 ** -13) and 2.0 ** -13 < 2 * rep2["e"].min()
    assert rep2["near"][:, 0, 1].all() and not rep2["near"][:, 0, 2].any() and not rep2["near"][:, 0, 0].any()
    assert rep2["decided"][:, 0, 0].all() and not rep2["decided"][:, 0, 1:].any() and (rep2["p_max"] == 0).all()


def test_gaussian_inputs_never_rebase_after_tile_0():
    """why the adversarial cases exist: on the inputs of test_gpu_kernel_ref.py::test_enc_attention_matches_fp64[1-1500-6] m_ref is
    set on tile 0 and never moves again, so the rescale of O and l and the rewrite of the fp16 pair run on no query"""
    B, S, H = 1, 1500, 6
    r = np.random.default_rng(K.zlib_key("enc", B, S, H))
    q = K.f16(r.standard_normal((B * S, 64 * H)) * K.ENC_Q_SCALE)
    k = K.f16(r.standard_normal((B * S, 64 * H)))
    rep = K.enc_rebase_replay(q, k, S, H)
    assert rep["rebase"][:, :, 0].all() and not rep["rebase"][:, :, 1:].any()
    assert not rep["near"].any() and rep["p_max"].max() < 64 and rep["m_absmax"].max() < 16
    print("Gaussian (1, 1500, 6): largest p", rep["p_max"].max(), "largest |m_ref|", rep["m_absmax"].max())


@pytest.mark.parametrize("name", K.ENC_REBASE_CASES)
def test_enc_rebase_cases_reach_their_paths_and_the_emulation_meets_the_bound(name):
    """per adversarial case of tests/test_gpu_enc_attn_ref.py, without a GPU: the replay's coverage conditions hold at every
    shape; at (1, 750) an emulation of the kernel's arithmetic lies inside the bound while each of its four rebase bugs, a
    dropped last key and the wrong head's V leave it by more than 2x"""
    for B, S in K.ENC_REBASE_SHAPES[1:]:
        q, k, _ = K.enc_rebase_case(name, B, S)
        print(name, B, S, K.enc_rebase_coverage(name, K.enc_rebase_replay(q, k, S, 2), S))
    B, S = K.ENC_REBASE_SHAPES[0]
    c = K.enc_rebase_reference(name, B, S)
    print(name, B, S, K.enc_rebase_coverage(name, c["rep"], S))
    got = K.enc_emulate(c["q"], c["k"], c["v"], B, S, 2)
    print("emulation, |err| / bound:", K.violation(c["ref"], c["bound"], got))
    K.within(got, c["ref"], c["bound"], f"emulated encoder attention, {name}")
    assert set(c["mutations"]) == set(K.ENC_BUGS) | {"last key dropped", "last head reads the previous head's V"}
    print(K.discriminates(c["ref"], c["bound"], c["mutations"]))
    if name == "offset":
        # the kernel's former arithmetic: alpha = exp2(-maximum) on tile 0 too, inf below -128, times O = l = 0
        former = K.enc_emulate(c["q"], c["k"], c["v"], B, S, 2, tile0_rescale=True)
        assert np.isnan(former[1::2].astype(np.float64)).all() and np.array_equal(former[0::2], got[0::2])


def test_enc_bound_terms_for_the_deferred_maximum():
    """attn_bound's mref and p_floor: each adds exactly its documented amount, and the floor counts the keys it should"""
    r = _r(21)
    B, S, H = 1, 130, 1
    q, k, v = K.f16(r.standard_normal((S, 64)) * 0.5), K.f16(r.standard_normal((S, 64))), K.f16(r.standard_normal((S, 64)))
    k[70] = K.f16(40.0 * K.d64(q[3]) / np.dot(K.d64(q[3]), K.d64(q[3])))          # query 3: key 70 scores 40
    ref, sabs, vst = K.enc_attention(q, k, v, B, S, H)
    base = K.attn_bound(ref, sabs, np.full(S, S), vst, p16=True, log2=True)
    mref = np.full((S, H), 100.0)
    with_m = K.attn_bound(ref, sabs, np.full(S, S), vst, p16=True, log2=True, mref=mref)
    assert np.allclose(with_m - base, 2 * np.log(2.0) * (2.0 ** -24 + 2.0 ** -22) * 100.0 * vst[0].reshape(S, 64), rtol=1e-9, atol=1e-15)
    floor = K.enc_p16_floor(q, k, v, B, S, H)
    assert np.array_equal(K.attn_bound(ref, sabs, np.full(S, S), vst, p16=True, log2=True, p_floor=floor), base + floor.reshape(S, 64))
    # query 3, by hand: tile 0's keys are rounded against tile 0's maximum, tile 1 and 2 against the running maximum 40
    s = K.d64(k) @ K.d64(q[3])
    run = np.where(np.arange(S) < 64, s[:64].max(), max(s[:64].max(), s[64:128].max()))
    run[128:] = max(run[127], s[128:].max())
    assert np.isclose(run[70], s[70]) and abs(s[70] - 40) < 0.1
    want = 2.0 ** -25 * np.abs(K.d64(v))[s - run < -14].sum(axis=0)
    assert np.allclose(floor[3, 0], want, rtol=1e-12, atol=0) and (s - run < -14)[64:].sum() > 50


# ---- the one-pass prefill attention (prefill_attn_kernel): reference, bound, discrimination ---------------------------------
def test_prefill_attention_is_a_per_query_softmax():
    r = _r(10)
    B, T, H = 2, 7, 2
    for causal, nk in ((True, T), (False, 11)):
        q, k, v = r.standard_normal((B * T, 128)), r.standard_normal((B * nk, 128)), r.standard_normal((B * nk, 128))
        o, sabs, (vdev, pv), n = K.prefill_attention(q, k, v, B, T, H, nk, causal)
        assert n.tolist() == ([1, 2, 3, 4, 5, 6, 7] * B if causal else [nk] * (B * T))
        perm = r.permutation(nk)
        op = K.prefill_attention(q, k, v, B, T, H, nk, causal, vperm=perm, stats=False)[0]
        first = np.minimum(np.arange(T), 2)
        of = K.prefill_attention(q, k, v, B, T, H, nk, causal, first=first, stats=False)[0]
        for b in range(B):
            for i in range(T):
                for h in range(H):
                    c = slice(64 * h, 64 * h + 64)
                    vis = i + 1 if causal else nk
                    kk, vv = k[b * nk:b * nk + vis, c], v[b * nk:b * nk + vis, c]
                    want = _naive_attn(q[b * T + i, c], kk, vv, 1 / 8)
                    assert np.allclose(o[b * T + i, c], want, rtol=0, atol=1e-12)
                    s_ = kk @ q[b * T + i, c] / 8
                    p_ = np.exp(s_ - s_.max()); p_ /= p_.sum()
                    assert np.isclose(sabs[b * T + i, h], (np.abs(kk) @ np.abs(q[b * T + i, c])).max() / 8)
                    assert np.allclose(vdev[b * T + i, h], p_ @ np.abs(vv - want), rtol=0, atol=1e-12)
                    assert np.allclose(pv[b * T + i, h], p_ @ np.abs(vv), rtol=0, atol=1e-12)
                    assert np.allclose(op[b * T + i, c], p_ @ v[b * nk:(b + 1) * nk, c][perm][:vis], rtol=0, atol=1e-12)
                    f0 = int(first[i])
                    assert np.allclose(of[b * T + i, c], _naive_attn(q[b * T + i, c], kk[f0:], vv[f0:], 1 / 8), rtol=0, atol=1e-12)
    # the natural-order map: keys 0 .. 3 of a 32-key step keep their slot, key 4 sits in slot 8, key 16 in slot 4 (k_prefill.hip)
    no = K.pf_natural_order(70)
    assert no[:4].tolist() == [0, 1, 2, 3] and no[4] == 8 and no[16] == 4 and no[20] == 12 and no[31] == 31 and no[36] == 40
    assert no[64 + 4] == 69 and no[64 + 5] == 69                      # past the last key: the clamped last row
    assert sorted(K.pf_natural_order(64).tolist()) == list(range(64))  # a permutation of each whole step


def _emulate_prefill(q, k, v, B, T, H, nk, causal, l_rounded=True):
    """prefill_attn_kernel's arithmetic in NumPy f32 / fp16: 64-key blocks, the running maximum, alpha, P rounded to fp16, l
    summed from the rounded weights (l_rounded=False: from the unrounded ones), O in f32, one final rounding"""
    f, LOG2E = np.float32, np.float32(1.4426950408889634)
    q, k, v = (a.astype(f) for a in (q.reshape(B, T, H, 64), k.reshape(B, nk, H, 64), v.reshape(B, nk, H, 64)))
    out = np.zeros((B, T, H, 64), np.float16)
    nvis = np.arange(T) + 1 if causal else np.full(T, nk)
    for b in range(B):
        for h in range(H):
            m, l, o = np.full(T, -np.inf, f), np.zeros(T, f), np.zeros((T, 64), f)
            for k0 in range(0, nk, 64):
                k1 = min(nk, k0 + 64)
                s = (q[b, :, h] @ k[b, k0:k1, h].T) * f(0.125)
                s = np.where(np.arange(k0, k1)[None, :] < nvis[:, None], s, f(-np.inf))
                mn = np.maximum(m, s.max(axis=-1))
                live = np.isfinite(mn)                              # causal rows ahead of this block: the wave skips it
                mn_ = np.where(live, mn, f(0))
                alpha = np.exp2((np.where(live, m, f(0)) - mn_) * LOG2E).astype(f)
                e = np.exp2((s - mn_[:, None]) * LOG2E).astype(f)
                p16 = e.astype(np.float16).astype(f)
                l = np.where(live, l * alpha + (p16 if l_rounded else e).sum(axis=-1, dtype=f), l)
                o = np.where(live[:, None], o * alpha[:, None] + p16 @ v[b, k0:k1, h], o)
                m = np.where(live, mn, m)
            out[b, :, h] = (o * (f(1) / l)[:, None]).astype(np.float16)
    return out.reshape(B * T, H * 64)


def _prefill_families():
    """(name, q, k, v, B, T, H, nk, causal): every data family of the GPU suite's prefill attention section, small"""
    r = _r(11)
    out = []
    for name, scale in (("random", 1.0), ("loud", 4.0)):
        B, T, H = 2, 130, 2
        out.append((f"self {name}", K.f16(r.standard_normal((B * T, 128)) * scale), K.f16(r.standard_normal((B * T, 128))),
                    K.f16(r.standard_normal((B * T, 128))), B, T, H, T, True))
        nk = 1500 if name == "random" else 750
        out.append((f"cross {name}", K.f16(r.standard_normal((B * 17, 128)) * scale), K.f16(r.standard_normal((B * nk, 128))),
                    K.f16(r.standard_normal((B * nk, 128))), B, 17, H, nk, False))
    # the GPU suite's own B = 1, H = 2, T = 127 self case (test_gpu_kernel_ref.rng("pf-self", 1, 2, 127)): the input on which
    # l summed from the unrounded weights left the bound (row 1: two visible keys whose V nearly agree in one dimension)
    r127 = np.random.default_rng(K.zlib_key("pf-self", 1, 2, 127))
    out.append(("self T=127 of the GPU suite",) + tuple(K.f16(r127.standard_normal((127, 128))) for _ in range(3)) + (1, 127, 2, 127, True))
    for causal, nq, nk in ((True, 300, 300), (False, 17, 300)):
        q, k, v = K.prefill_adversarial(r, nq, nk, causal)
        U = q.shape[0]
        qq, kk, vv = (np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(a.shape[1], U * 64) for a in (q, k, v))
        out.append((f"{'self' if causal else 'cross'} adversarial", qq, kk, vv, 1, nq, U, nk, causal))
    return out


def test_prefill_bound_holds_for_an_f32_fp16_emulation_of_the_kernel():
    """on every data family of the GPU tests: the fp16 subnormal floor of P fits into what attn_bound(p16) grants beyond need
    (kref.prefill_bound asserts it on the data), and an emulation of the kernel's roundings stays inside the bound -- while the
    same emulation with l summed from the UNROUNDED weights, the kernel's former arithmetic, does not"""
    worst, former = {}, {}
    for name, q, k, v, B, T, H, nk, causal in _prefill_families():
        ref, sabs, vst, n = K.prefill_attention(q, k, v, B, T, H, nk, causal)
        bound = K.prefill_bound(ref, sabs, n, vst, floor=K.prefill_p16_floor(q, k, v, B, T, H, nk, causal))
        got = _emulate_prefill(q, k, v, B, T, H, nk, causal)
        worst[name] = K.violation(ref, bound, got)
        former[name] = K.violation(ref, bound, _emulate_prefill(q, k, v, B, T, H, nk, causal, l_rounded=False))
        K.within(got, ref, bound, f"emulated prefill attention, {name}")
    print("emulation, worst |err| / bound:", worst)
    print("... with l from the unrounded weights:", former)
    assert max(worst.values()) > 0.05, worst        # the bound is not orders of magnitude away from the arithmetic
    assert former["self T=127 of the GPU suite"] > 1.0, former


def test_prefill_mutations_leave_the_bound_on_their_designated_cases():
    """each named bug of the GPU section, as the same reference with a changed argument, leaves the bound by more than 2x on the
    case that is there to catch it (random data alone would not do: behind a loud q, or among 1500 keys, a key too few moves
    the output by next to nothing, so the mask errors have designated cases: few keys, equal keys, ascending scores)"""
    r = _r(12)
    fams = {f[0]: f[1:] for f in _prefill_families()}
    # mask errors: unit-variance q at few keys, equal keys, ascending scores; NOT the loud q
    B, T, H = 2, 17, 2
    q, k, v = (K.f16(r.standard_normal((B * T, 128))) for _ in range(3))
    ref, sabs, vst, n = K.prefill_attention(q, k, v, B, T, H, T, True)
    bound = K.prefill_bound(ref, sabs, n, vst)
    i = np.arange(T)

    def mut(**kw):
        return K.prefill_attention(q, k, v, B, T, H, T, True, stats=False, **kw)[0]

    vs = v.copy(); vs[:, 64:] = v[:, :64]
    got = K.discriminates(ref, bound, {
        "mask one key short": mut(nvis=np.maximum(i, 1)), "mask one key long": mut(nvis=np.minimum(i + 2, T)),
        "natural key order": mut(vperm=K.pf_natural_order(T)),
        "last head reads the previous head's V": K.prefill_attention(q, k, vs, B, T, H, T, True, stats=False)[0],
        "clip b reads clip b-1's keys": K.prefill_attention(q, np.roll(k.reshape(B, T, 128), 1, 0), np.roll(v.reshape(B, T, 128), 1, 0),
                                                            B, T, H, T, True, stats=False)[0]})
    print("self, 17 keys:", got)
    # the adversarial units: every family catches both mask errors alone (cross dominant-first: a key too many only -- its
    # last key holds e^-40 of the weight by construction)
    for form, causal in (("self", True), ("cross", False)):
        qa, ka, va, Ba, Ta, Ha, nka, _ = fams[f"{form} adversarial"]
        refa, sabsa, vsta, na = K.prefill_attention(qa, ka, va, Ba, Ta, Ha, nka, causal)
        ba = K.prefill_bound(refa, sabsa, na, vsta)
        for name, m in K.prefill_mask_mutations(qa, ka, va, Ta, Ha, nka, causal).items():
            for u, fam in enumerate(K.PF_FAMILIES):
                c = slice(64 * u, 64 * u + 64)
                f = K.violation(refa[:, c], ba[:, c], m[:, c])
                if (form, fam, name) == ("cross", "dominant-first", "one key too few"):
                    assert f < 2
                else:
                    assert f > 2, (form, fam, name, f)
    # the cross form on random data with its planted keys (kref.prefill_cross_case): both mask errors, the wrong head slab, the
    # wrong clip slab, at a key count where random data alone would hide a key too few
    Bc, Hc, Tc, Sc = 2, 2, 5, 750
    qc, ckc, cvc = K.prefill_cross_case(r, Bc, Tc, Hc, Sc)
    qu, ku, vu = K.pf_units(qc, Bc, Tc, Hc), K.pf_from_head_major(ckc, Bc, Hc, Sc), K.pf_from_head_major(cvc, Bc, Hc, Sc)
    refc, sabsc, vstc, nc = K.prefill_attention(qu, ku, vu, 1, Tc, Bc * Hc, Sc, False)
    mc = K.prefill_cross_mutations(qu, ku, vu, Bc, Tc, Hc, Sc)
    assert len(mc) == 4, sorted(mc)
    print("cross, 750 keys:", K.discriminates(refc, K.prefill_bound(refc, sabsc, nc, vstc), mc))
    # T = 300: the second query tile ignores keys below 256
    qa, ka, va, Ba, Ta, Ha, nka, _ = fams["self adversarial"]
    refa, sabsa, vsta, na = K.prefill_attention(qa, ka, va, Ba, Ta, Ha, nka, True)
    K.discriminates(refa, K.prefill_bound(refa, sabsa, na, vsta),
                    {"second tile ignores keys below 256": K.prefill_attention(qa, ka, va, Ba, Ta, Ha, nka, True, stats=False,
                                                                               first=np.where(np.arange(Ta) >= 256, 256, 0))[0]})


# ---- token selection -------------------------------------------------------------------------------------------------------
def _oracle(layout_name):
    import common
    from norma_amd import vocab
    from oracle import oracle as O
    tk = vocab.VOCABS[layout_name]
    name = "test-d128" if layout_name == "EnV1" else "test-d256-mel128"
    cfg = common.make_config(name, encoder_layers=0, decoder_layers=0)
    return O, O.OracleModel(cfg, tk, tk.en, tk.transcribe)


def _f32_softmax(l):
    l = np.asarray(l, np.float32)
    e = np.exp(l - l.max())
    return e / e.sum(dtype=np.float32)


@pytest.mark.parametrize("lname", ["EnV1", "V2"])
def test_token_reference_at_f32_agrees_with_the_oracle_rules(lname):
    """the fp64 restatement, with the margin of an f32 evaluation (numpy softmax, the oracle's sequential timestamp sum),
    picks what oracle.apply_rules + wo_argmax_total pick on every decided case, and the sampler's draw what
    oracle.sample_token draws"""
    import ctypes as C
    O, om = _oracle(lname)
    layout = [l for l in K.token_layouts() if l[0] == lname][0]
    V, tk = layout[1], layout[2]
    path = K.PATHS["f32"] + (float(V - tk.no_timestamps),)
    first = om.mask(3)
    n_dec = 0
    for c in K.greedy_cases(layout)[:4]:
        for b in range(c.B):
            n = int(c.n_tokens[b])
            toks, l = c.tokens[b, :n], c.logits[0, b, :V]
            s = K.step_ref(l, list(toks), int(c.have_last[b]), int(c.last_ts[b]), c.sup, c.tk, path)
            p32 = _f32_softmax(l)
            q = om.apply_rules(p32, toks, int(c.last_ts[b])) if c.have_last[b] else p32 + first
            got = O.lib().wo_argmax_total(q.ctypes.data_as(C.POINTER(C.c_float)), V)
            assert got in s.ok, (c.labels[b], got, s.ok)
            if s.decided:
                n_dec += 1
                assert got == s.next, (c.labels[b], got, s.next)
    assert n_dec >= 100, n_dec
    n_dec = 0
    for c in K.sample_cases(layout):
        t = 1.0 / float(np.float32(c.inv_t))
        for b in range(c.B):
            n = int(c.n_tokens[b])
            toks, l = c.tokens[b, :n], c.logits[0, b, :V]
            s = K.step_ref(l, list(toks), int(c.have_last[b]), int(c.last_ts[b]), c.sup, c.tk, path)
            p32 = _f32_softmax(l)
            q = om.apply_rules(p32, toks, int(c.last_ts[b])) if c.have_last[b] else p32 + first
            p, x = K.softmax64(l)
            allowed = np.isfinite(q)
            rel = K._rel(K._eps_se(p, x, path, V), x)
            u = K._philox_u(c.seed, c.clip0 + b, n, c.attempt)
            j, ok, dec = K.sample_ref(np.where(allowed, p, -np.inf), rel, t, u)
            got = O.sample_token(q, t, c.seed, c.clip0 + b, n, c.attempt)
            assert got in ok, (c.labels[b], got, ok)
            if dec and s.decided:
                n_dec += 1
                assert got == j
    assert n_dec >= 20, n_dec
    om.close()


def _outcome(st, b):
    return (tuple(st["tokens"][b, :st["n_tokens"][b]].tolist()), int(st["n_tokens"][b]), int(st["done"][b]),
            int(st["have_last"][b]), int(st["last_ts"][b]), None if st["pos"] is None else int(st["pos"][b]))


def test_token_mutations_change_a_decided_outcome_of_the_suite():
    """each plausible bug of MUTATIONS, applied to the reference, changes the outcome of at least one decided case of the GPU
    suite's own data (kref.greedy_cases / sequence_cases / lang cases), so a kernel with that bug fails the suite"""
    caught = {m: 0 for m in K.MUTATIONS}
    for layout in [l for l in K.token_layouts() if l[0] in ("V2", "small")]:
        cases = []
        for c in K.greedy_cases(layout) + K.sequence_cases(layout):
            cases += [c] + ([c.extra] if c.extra is not None else [])
        for c in cases:
            ref, info = K.logit_step_ref(c)
            for m in K.MUTATIONS:
                mst, minfo = K.logit_step_ref(c, mut=(m,))
                for b in range(c.B):
                    if info[b]["decided"] and info[b]["ns_decided"] and _outcome(ref, b) != _outcome(mst, b):
                        caught[m] += 1
    # language detection: ties go to the FIRST index; the mutation sends them to the last
    lt = np.array([5, 3, 9, 1], np.int32)
    l = np.zeros(12, np.float32); l[[3, 1]] = 2.0
    assert K.lang_ref(l, lt)[2] == 3 and K.lang_ref(l, lt, mut=("tie_low",))[2] == 1
    missed = [m for m, v in caught.items() if not v]
    print("mutations caught (decided rows changed):", caught)
    assert not missed, f"no decided case of the suite distinguishes {missed}"


def test_token_margins_flag_near_ties_and_accept_exact_ties():
    from norma_amd import vocab
    tk = vocab.VOCABS["V2"]
    V = tk.n_vocab
    sup = K.sup_array(V, vocab.default_suppress_tokens("V2"), tk.no_timestamps).astype(bool)
    l = np.zeros(V, np.float32)
    l[100] = l[200] = 5.0
    s = K.step_ref(l, [tk.sot, tk.en, tk.transcribe, tk.zero_sec, 11, tk.zero_sec + 3], 1, tk.zero_sec + 3, sup,
                   K.tk_array(tk), K.PATHS["logit_step"])
    assert s.state == K.NON_TS
    l2 = np.zeros(V, np.float32)
    l2[400] = 5.0
    l2[300] = np.nextafter(np.float32(5.0), np.float32(0))        # one ulp apart: not decidable
    s = K.step_ref(l2, [tk.sot, tk.en, tk.transcribe], 0, 0, sup, K.tk_array(tk), K.PATHS["logit_step"])
    assert s.state == K.FIRST and s.next == tk.one_sec              # the window only: flat -> the last index wins
    t = K.tk_array(tk)
    l[tk.no_timestamps + 1:] = -10.0                                 # TEXT -> PAST: max_text beats the timestamps' sum
    s = K.step_ref(l, [tk.sot, tk.en, tk.transcribe, tk.zero_sec, 11], 1, tk.zero_sec, sup, t, K.PATHS["logit_step"])
    assert s.next == 200 and s.decided                               # exact tie: the higher index, decided
    l[200] = np.nextafter(np.float32(5.0), np.float32(0))
    s = K.step_ref(l, [tk.sot, tk.en, tk.transcribe, tk.zero_sec, 11], 1, tk.zero_sec, sup, t, K.PATHS["logit_step"])
    assert s.next == 100 and not s.decided and s.ok == {100, 200}


# ---- log-mel (k_mel.hip): the product's tables, the effective DFT matrix, the bound against an f32 emulation ------------------
def _mel_setup(n_mel):
    from norma_amd import assets_io
    _make_wrapper_library()
    t = K.mel_tables()
    filt = assets_io.mel_filters(n_mel)
    return t, filt, K.mel_groups(filt)


def test_mel_tables_are_one_rounding_from_fp64_of_their_f32_angles():
    """kref_mel_tables answers without a GPU with the product's tables (mel_host.h); every cos / sin entry lies within 2^-23 of
    fp64 cos / sin of the same f32 angle, the window within 2^-23 of 0.5 (1 - cos) (cosf, the subtraction, an exact halving)"""
    t, filt, grp = _mel_setup(80)
    leaf, tw, hann = K.mel_table_angles()
    ulp = 2.0 ** -23
    assert np.abs(K.d64(t["dft_cos"]) - np.cos(K.d64(leaf))).max() <= ulp
    assert np.abs(K.d64(t["dft_sin"]) - np.sin(K.d64(leaf))).max() <= ulp
    assert np.abs(K.d64(t["tw_cos"]) - np.cos(K.d64(tw))).max() <= ulp
    assert np.abs(K.d64(t["tw_sin"]) + np.sin(K.d64(tw))).max() <= ulp
    assert np.abs(K.d64(t["hann"]) - 0.5 * (1 - np.cos(K.d64(hann)))).max() <= ulp
    assert np.abs(K.d64(t["dft_cos"])).max() <= 1 and np.abs(K.d64(t["tw_sin"])).max() <= 1
    assert t["hann"][0] == 0 and t["tw_cos"][0] == 1 and t["tw_sin"][0] == 0
    # the f32 angles reach 145 rad: the tables are off the IDEAL angles by about 1e-5, which is part of the contract
    k = np.arange(25)
    off = np.abs(K.d64(t["dft_cos"]) - np.cos(2 * np.pi * np.outer(k, k) / 25)).max()
    assert 1e-6 < off < K.mel_matrix_bound()


@pytest.mark.parametrize("n_mel", [80, 128])
def test_mel_groups_are_the_tap_ranges(n_mel):
    t, filt, grp = _mel_setup(n_mel)
    assert grp.shape == (n_mel, 2) and (filt >= 0).all()
    for m in range(n_mel):
        nz = np.flatnonzero(filt[m, :200])
        want = (nz[0] // 4, nz[-1] // 4 + 1) if nz.size else (0, 0)
        assert tuple(grp[m]) == want, m
    assert (grp[:, 1] - grp[:, 0]).max() <= 50
    assert tuple(K.mel_groups(np.zeros((2, 201), np.float32))[1]) == (0, 0)


def test_mel_effective_matrix_is_the_dft_within_the_derived_distance():
    """the recursion on the 400 unit impulses gives the effective matrix T of the table-defined map; it must be the DFT within
    mel_matrix_bound (derived from the roundings of the angles and the entries, not from this measurement)"""
    t, filt, grp = _mel_setup(80)
    T = K.mel_spectrum(np.eye(400), t)                   # T[n][k]: input n -> bin k
    n = np.arange(400)
    exact = np.exp(-2j * np.pi * np.outer(n, n) / 400)
    dev = np.abs(T - exact).max()
    print(f"max |T - exp(-2 pi i n k / 400)| = {dev:.3e} (derived limit {K.mel_matrix_bound():.3e})")
    assert dev <= K.mel_matrix_bound() < 5e-5
    # the map is what the reference applies: a random frame through mel_spectrum equals x . T
    x = _r(40).standard_normal((3, 400))
    assert np.abs(K.mel_spectrum(x, t) - x @ T).max() < 1e-10
    # and the whole operation reference against a naive evaluation with numpy's FFT, up to the tables' distance from it
    S, X, xw, Pf = K.mel_power_sums(x, t, filt)
    P = np.abs(np.fft.fft(x * K.d64(t["hann"]), axis=-1)) ** 2
    naive = np.stack([[sum(filt[m, k] * (P[f, k] + (P[f, 400 - k] if 1 <= k <= 199 else 0)) for k in range(201)) for m in range(80)]
                      for f in range(3)])
    assert np.abs(S - naive).max() <= 3 * K.mel_matrix_bound() * np.abs(naive).max()


def _mel_mutations(fx, t, filt):
    return {"leaf term dropped": K.mel_power_sums(fx, t, filt, drop_leaf_term=24)[0],
            "last-level twiddle off by one": K.mel_power_sums(fx, t, filt, tw_shift_last=1)[0],
            "fold omitted": K.mel_power_sums(fx, t, filt, fold=False)[0]}


@pytest.mark.parametrize("n_mel", [80, 128])
def test_mel_f32_emulation_stays_inside_the_bound_and_bugs_leave_it(n_mel):
    """the NumPy f32 emulation of logmel_kernel's arithmetic on every family of the GPU test: its spectrum within c u A, its
    sums within dS, its logs inside the interval.  On the broadband families at least 99 % of the intervals are narrower than
    1e-3 in log10, and three plausible bugs leave dS by more than 2x (kref.discriminates) on the same data."""
    t, filt, grp = _mel_setup(n_mel)
    worst_x = worst_s = 0.0
    for family in K.MEL_FAMILIES:
        narrow, total, left = 0, 0, {}
        for frames in K.MEL_FRAMES:
            pcm, ns = K.mel_case(family, frames, 4 if family == "noise-0.1" else 3)
            fx = K.mel_frames(pcm, ns, frames).reshape(-1, 400)
            assert np.abs(fx).max() < K.MEL_CANARY                            # no canary inside a frame
            S, X, xw, Pf = K.mel_power_sums(fx, t, filt)
            dS = K.mel_bound(X, xw, Pf, filt, grp)
            lo, hi = K.mel_interval(S, dS)
            X32, S32 = K.mel_emulate_f32(K.f32(fx), t, filt, grp)
            A = np.abs(xw).sum(axis=-1, keepdims=True)
            xerr = np.abs((K.d64(X32[..., 0]) + 1j * K.d64(X32[..., 1])) - X)
            assert (xerr <= K.MEL_C * K.U32 * A).all(), (family, frames)
            assert (np.abs(K.d64(S32) - S) <= dS).all(), (family, frames)
            live = A[:, 0] > 0
            if live.any():
                worst_x = max(worst_x, float((xerr[live] / (K.U32 * A[live])).max()))
                worst_s = max(worst_s, float((np.abs(K.d64(S32) - S) / dS).max()))
            K.mel_inside(K.mel_log_f32(S32), lo, hi, f"f32 emulation {family} frames={frames}")
            narrow += int(((hi - lo) < 1e-3).sum()); total += lo.size
            if family in K.MEL_BROADBAND:
                for k, v in K.discriminates(S, dS, _mel_mutations(fx, t, filt)).items():
                    left[k] = max(left.get(k, 0.0), v)
                if frames == 33:                                               # how many outputs each bug moves out, as information
                    for k, m in _mel_mutations(fx, t, filt).items():
                        print(f"  {family} n_mel={n_mel}: {k}: {100 * (np.abs(m - S) > 2 * dS).mean():.1f} % of the outputs leave 2 dS")
        print(f"{family} n_mel={n_mel}: {100 * narrow / total:.2f} % of the intervals narrower than 1e-3")
        if family in K.MEL_BROADBAND:
            assert narrow >= 0.99 * total, (family, narrow, total)
    print(f"n_mel={n_mel}: f32 emulation spectrum error up to {worst_x:.2f} u A, |S32 - S64| / dS up to {worst_s:.3f}")
    # the conditions on the data that the GPU cases rely on: the quiet noise is negative throughout and (all but the odd output
    # of a narrow filter) above the floor; the burst's quiet frames lie more than 8 below its maximum
    pcm, ns = K.mel_case("noise-3e-4", 33, 3)
    lo, hi, ref = K.mel_reference(pcm, ns, 33, t, filt, grp)
    assert (hi < 0).all() and (lo > -10).mean() > 0.99
    pcm, ns = K.mel_case("burst", 33, 3)
    lo, hi, ref = K.mel_reference(pcm, ns, 33, t, filt, grp)
    assert (ref.max(axis=(1, 2)) > 0).all() and ((hi < ref.max(axis=(1, 2), keepdims=True) - 8.01).mean(axis=(1, 2)) > 0.5).all()


def test_mel_impulse_identity_and_ordered_encoding():
    """one unit sample at offset o: the fp64 table map gives hann_o^2 sum_k w_k f[m][k] within the stated relative distance; the
    ordered encoding is monotone and keeps -10, negative and positive values apart"""
    t, filt, grp = _mel_setup(80)
    offs = np.arange(400)
    S, dS = K.mel_impulse_expected(offs, t, filt)
    got = K.mel_power_sums(np.eye(400), t, filt)[0]
    assert (np.abs(got - S) <= dS).all()
    assert S[0].max() == 0 and S[200].min() > 0
    # an impulse that misses the fold loses about half of every interior weight: far outside
    assert (np.abs(K.mel_power_sums(np.eye(400), t, filt, fold=False)[0] - S)[1:] > 100 * dS[1:]).all()
    v = np.array([-np.inf, -10.0, -9.999999, -1.0, -0.0, 0.0, 1e-30, 0.5, 3.25, np.inf], np.float32)
    enc = K.f32_ordered(v).astype(np.int64)
    assert (np.diff(enc) >= 0).all() and (np.diff(enc)[[0, 1, 2, 3, 5, 6, 7, 8]] > 0).all()
    assert enc[1] == 0x3EDFFFFF and enc[7] == 0xBF000000
