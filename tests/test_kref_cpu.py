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


def test_make_builds_the_wrapper_library_with_every_entry_point():
    root = K.ROOT
    if not os.path.exists(os.path.join(root, "norma_amd", "csrc", "build", "k_decode.o")):
        subprocess.check_call(["make", "-C", os.path.join(root, "norma_amd", "csrc"), "-j8"])
    subprocess.check_call(["make", "-C", os.path.join(root, "tools", ), "bin/libnh_kref.so"], stdout=subprocess.DEVNULL)
    assert os.path.exists(K.LIB_PATH)
    syms = subprocess.run(["nm", "-D", "--defined-only", K.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert set(K.WRAPPERS) <= exported, set(K.WRAPPERS) - exported


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
