"""GPU: token-level timestamps (nh_align).  Kernel level: the launchers of k_align.hip on planted data (tools/kref.hip) against
the float64 / float32 references of tests/align_ref.py, each bound derived from the arithmetic and shown to catch plausible
bugs on the case's own data.  C ABI level: the staged check on test-d128 (weights against a float64 decoder chain, the matrix
against float64 stages 3 - 5 of the GPU's own weights, the path against the float32 DTW of the GPU's own matrix), batch
invariance, the untouched context, every refusal, and the host layer."""
import zlib

import numpy as np
import pytest

import align_ref as AR
import common
import kref as K

pytestmark = pytest.mark.gpu

S_CACHE = 1500


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- weights ----------------------------------------------------------------------------------------------------------------
ROW_SETS = {1: [(1,), (15,), (16,), (17,), (33,)], 3: [(1, 15, 16), (17, 33, 1)]}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("nk", [4, 63, 64, 65, 750, 1500])
def test_weights_kernel_matches_fp64(nk, H, B):
    """rows n - 1 in {1, 15, 16, 17, 33} (one row block, its edges, more than two), nk at the 16-key tile and 64-key wave-round
    edges, half and all of the cache; the first and the last head of H.  Keys at or beyond nk hold values that would own the
    softmax if they were read."""
    r = rng("aw", nk, H, B)
    heads = [0, H - 1]
    A, S = len(heads), S_CACHE
    for rows in ROW_SETS[B]:
        max_rows = max(rows)
        q = K.f16(r.standard_normal((A, max_rows, B, 64)))
        k = K.f16(r.standard_normal((B, H, S, 64)))
        k[:, :, nk:] = K.f16(20.0 * r.standard_normal((B, H, S - nk, 64)))
        W = AR.gpu_weights(q, k, heads, rows, [nk] * B)
        for b in range(B):
            n = rows[b]
            for a, h in enumerate(heads):
                got = W[b, a]
                assert np.isnan(got[n:]).all() and np.isnan(got[:, nk:]).all(), "wrote outside [rows][nk]"
                ref, sabs, x = AR.weights(q[a, :n, b], k[b, h], nk)
                bound = AR.weights_bound(ref, sabs, x)
                K.within(got[:n, :nk], ref, bound, f"weights nk={nk} H={H} B={B} rows={rows} clip {b} head {h}")
                mut = {"one key too few": np.pad(AR.weights(q[a, :n, b], k[b, h], nk - 1)[0], [(0, 0), (0, 1)]),
                       "scale dropped": AR.weights(q[a, :n, b], k[b, h], nk, scale=1.0)[0],
                       "neighbouring head": AR.weights(q[a, :n, b], k[b, h + 1 if h == 0 else h - 1], nk)[0]}
                if n > 1:
                    mut["row p - 1"] = np.roll(ref, 1, axis=0)
                if nk < S:
                    mut["keys past nk read"] = AR.weights(q[a, :n, b], k[b, h], min(S, nk + 16))[0][:, :nk]
                K.discriminates(ref, bound, mut)


# ---- reduce -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("nk", [3, 4, 8, 65])
def test_reduce_kernels_match_fp64(nk, A):
    """clip 0: 9 rows, clip 1: one row (std == 0 everywhere: all zeros out); prompt lengths 1 and 3"""
    r = rng("ar", nk, A)
    S, max_rows, B = 80, 9, 2
    rows = [9, 1]
    W = np.full((B, A, max_rows, S), np.nan, dtype=np.float32)
    for b in range(B):
        s = r.standard_normal((A, rows[b], nk)) * 2
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        W[b, :, :rows[b], :nk] = e / e.sum(axis=-1, keepdims=True)
    for P in (1, 3):
        use = [b for b in range(B) if rows[b] + 1 - P >= 1]
        M = AR.gpu_reduce(W, [rows[b] if b in use else 0 for b in range(B)], [nk] * B, P)
        for b in range(B):
            R = rows[b] + 1 - P if b in use else 0
            assert np.isnan(M[b, R:]).all() and np.isnan(M[b, :, nk:]).all(), "wrote outside [R][nk]"
            if not R:
                continue
            Wb = W[b, :, :rows[b], :nk]
            ref, bound = AR.matrix(Wb, P), AR.matrix_bound(Wb, P)
            K.within(M[b, :R, :nk], ref, bound, f"matrix nk={nk} A={A} P={P} clip {b}")
            if rows[b] == 1:
                assert not M[b, :R, :nk].any()
                continue
            mut = {"sample std": AR.matrix(Wb, P, ddof=1)}
            if nk > 3:   # nk <= 3 is not filtered: the window mutations are the identity there
                mut["edge-repeating padding"] = AR.matrix(Wb, P, edge=True)
                mut["window 5"] = AR.matrix(Wb, P, width=5)
            if A > 1:
                mut["a head left out"] = AR.matrix(Wb, P, heads=list(range(A - 1)))
            K.discriminates(ref, bound, mut)


# ---- DTW --------------------------------------------------------------------------------------------------------------------
def _dtw_mats(R, nk, r):
    planted, pf, pl = AR.planted_path(R, nk, r)
    return [("random", r.standard_normal((R, nk)).astype(np.float32), None),
            ("all equal", np.full((R, nk), 0.25, np.float32), None),
            ("ties", r.integers(-2, 3, (R, nk)).astype(np.float32), None),
            ("planted", planted, (pf, pl))]


@pytest.mark.parametrize("R,nk", [(1, 1), (1, 9), (9, 1), (20, 7), (17, 64), (64, 65)])
@pytest.mark.parametrize("P", [1, 3])
def test_dtw_kernel_is_integer_exact(R, nk, P):
    r = rng("dtw", R, nk)
    mats = _dtw_mats(R, nk, r)
    B, S, max_rows = len(mats), nk + 3, R + P - 1
    M = np.full((B, max_rows, S), np.nan, dtype=np.float32)
    for b, (_, m, _) in enumerate(mats):
        M[b, :R, :nk] = m
    first, last = AR.gpu_dtw(M, [R + P - 1] * B, [nk] * B, P)
    for b, (name, m, known) in enumerate(mats):
        f, l, _ = AR.dtw(m)
        if known is not None:
            assert f.tolist() == known[0].tolist() and l.tolist() == known[1].tolist()
        assert first[b, P:P + R].tolist() == f.tolist() and last[b, P:P + R].tolist() == l.tolist(), name
        assert (first[b, :P] == -1).all() and (last[b, :P] == -1).all() and (first[b, P + R:] == -1).all() and (last[b, P + R:] == -1).all()


def test_dtw_kernel_full_size():
    R, nk = 447, 1500
    m = rng("dtw-full").standard_normal((R, nk)).astype(np.float32)
    first, last = AR.gpu_dtw(m[None], [R], [nk], 1)
    f, l, _ = AR.dtw_diagonals(m)
    assert first[0, 1:].tolist() == f.tolist() and last[0, 1:].tolist() == l.tolist()


# ---- through the C ABI ------------------------------------------------------------------------------------------------------
NAME = "test-d128"
P_LEN = 3
N_TOKENS = (5, 21, 40)
N_KEYS = (1500, 750, 37)
HEADS = [(0, 1), (1, 0)]


def _overrides(cfg):
    """the synthetic checkpoint with a conv stem 8 x stronger (encoder outputs of different clips differ visibly) and cross-attention
    q / k projections 16 x / 8 x larger: scores with a spread of a few units, so that the softmax is peaked like a trained
    model's instead of flat (largest weight 0.07 over 1500 keys, smallest 2e-9: far from f32 underflow) and a wrong head, layer,
    position or clip moves the weights by 8 x the bar or more; powers of two keep every value fp16-representable"""
    from norma_amd import synth
    over = {}
    for n, f in [("model.encoder.conv1.weight", 8.0), ("model.encoder.conv2.weight", 8.0)] + \
                [(f"model.decoder.layers.{l}.encoder_attn.{p}_proj.weight", f) for l in range(cfg.decoder_layers) for p, f in (("q", 16.0), ("k", 8.0))]:
        over[n] = synth.synth_tensor_by_name(cfg, n) * np.float32(f)
    return over


class Fixture:
    """one model, three encoded clips, their token sequences, and the float64 chains (exact and fp16-rounded) -- computed once"""

    def __init__(self):
        from norma_amd import hip, synth
        self.hip = hip
        self.cfg, self.tk = common.make_config(NAME), common.tokens_for(NAME)
        tk = self.tk
        self.over = _overrides(self.cfg)
        self.hm = common.build_hip(self.cfg, tk, overrides=self.over, max_batch=3)
        self.clips = [synth.synth_pcm(0), synth.synth_pcm(1), synth.synth_pcm(2, 400000)]
        r = rng("tokens")
        self.tokens = []
        for n in N_TOKENS:
            body = [int(t) for t in r.integers(300, 40000, n - P_LEN - 1)]
            if len(body) > 4:
                body[0], body[-1] = tk.zero_sec, tk.zero_sec + 100          # the sequence as decoded: timestamp tokens included
            self.tokens.append([tk.sot, tk.en, tk.transcribe] + body + [tk.eot])
        self.encode_all()
        self.xa = [self.hm.encoder_output(b) for b in range(3)]
        wts = AR.decoder_weights(self.cfg, overrides=self.over)
        self.exact = [AR.chain(self.cfg, wts, t[:-1], xa) for t, xa in zip(self.tokens, self.xa)]
        self.rounded = [AR.chain(self.cfg, wts, t[:-1], xa, rounded=True) for t, xa in zip(self.tokens, self.xa)]

    def encode_all(self):
        self.hm.logmel(self.clips)
        self.hm.encode()

    def align_all(self, keep=1):
        self.hm.set_option(self.hip.NH_OPT_ALIGN_KEEP, keep)
        return self.hm.align(self.tokens, prompt_len=P_LEN, heads=HEADS, n_keys=N_KEYS)


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    yield f
    f.hm.close()


def test_staged_check(fx):
    """(a) weights against the float64 chain within 4 e, e = what rounding the activations to fp16 moves the chain's weights by;
    (b) the matrix against float64 stages 3 - 5 of the GPU's own weights; (c) the path against the float32 DTW of the GPU's
    own matrix.  Before the alignment runs, the CPU shows that the bar separates a wrong head, a wrong layer, position p - 1 and
    another clip's K from the right answer by a factor of two on this data."""
    ref = [[AR.chain_weights(fx.exact[b], l, h, N_KEYS[b]) for l, h in HEADS] for b in range(3)]
    rnd = [[AR.chain_weights(fx.rounded[b], l, h, N_KEYS[b]) for l, h in HEADS] for b in range(3)]
    e = max(np.abs(ref[b][a] - rnd[b][a]).max() for b in range(3) for a in range(len(HEADS)))
    bar = 4 * e
    print(f"\nstaged check: e = {e:.3e}, bar 4 e = {bar:.3e}")
    H = fx.cfg.decoder_attention_heads
    for b in range(3):
        for a, (l, h) in enumerate(HEADS):
            ex, nk = fx.exact[b], N_KEYS[b]
            c = slice(h * 64, h * 64 + 64)
            other = fx.exact[(b + 1) % 3]["k"][l][:, c]
            wrong = {"wrong head": AR.chain_weights(ex, l, (h + 1) % H, nk),
                     "wrong layer": AR.chain_weights(ex, 1 - l, h, nk),
                     "position p - 1": np.roll(ref[b][a], 1, axis=0),
                     "another clip's K": AR.weights(ex["q"][l][:, c], other, nk)[0]}
            for name, w in wrong.items():
                assert np.abs(w - ref[b][a]).max() > 2 * bar, (name, b, a, np.abs(w - ref[b][a]).max(), bar)
    first, last = fx.align_all(keep=1)
    worst = 0.0
    for b in range(3):
        n, nk = N_TOKENS[b], N_KEYS[b]
        Wg = np.stack([fx.hm.align_weights(b, a) for a in range(len(HEADS))])
        for a in range(len(HEADS)):
            worst = max(worst, np.abs(Wg[a] - ref[b][a]).max())
        print(f"clip {b}: max |W_gpu - W_chain| = {max(np.abs(Wg[a] - ref[b][a]).max() for a in range(len(HEADS))):.3e}")
        for a in range(len(HEADS)):
            assert np.abs(Wg[a] - ref[b][a]).max() <= bar, (b, a)                                           # (a)
        Mg = fx.hm.align_matrix(b)
        K.within(Mg, AR.matrix(Wg, P_LEN), AR.matrix_bound(Wg, P_LEN), f"matrix view of clip {b}")           # (b)
        f, l, _ = AR.dtw(Mg)
        assert first[b, P_LEN:n].tolist() == f.tolist() and last[b, P_LEN:n].tolist() == l.tolist()          # (c)
        assert (first[b, :P_LEN] == -1).all() and (last[b, :P_LEN] == -1).all() and (first[b, n:] == -1).all() and (last[b, n:] == -1).all()
        assert first[b, P_LEN] == 0 and last[b, n - 1] == nk - 1
    print(f"measured GPU error {worst:.3e} against the bar {bar:.3e}")


@pytest.mark.parametrize("keep", [1, 0])
def test_each_clip_alone_is_bit_identical(fx, keep):
    fx.encode_all()
    first, last = fx.align_all(keep)
    views = [([fx.hm.align_weights(b, a) for a in range(len(HEADS))], fx.hm.align_matrix(b)) for b in range(3)] if keep else None
    for b in range(3):
        fx.hm.logmel([fx.clips[b]])
        fx.hm.encode()
        f1, l1 = fx.hm.align([fx.tokens[b]], prompt_len=P_LEN, heads=HEADS, n_keys=[N_KEYS[b]])
        assert np.array_equal(f1[0], first[b]) and np.array_equal(l1[0], last[b])
        if keep:
            for a in range(len(HEADS)):
                assert np.array_equal(fx.hm.align_weights(0, a), views[b][0][a])
            assert np.array_equal(fx.hm.align_matrix(0), views[b][1])
        else:
            with pytest.raises(fx.hip.HipError) as ei:
                fx.hm.align_matrix(0)
            assert ei.value.code == 3
    fx.encode_all()


def test_align_path_is_the_dtw_alone(fx):
    r = rng("path")
    for R, nk in [(1, 1), (20, 7), (64, 65)]:
        for name, m, _ in _dtw_mats(R, nk, r):
            f, l, _ = AR.dtw(m)
            gf, gl = fx.hm.align_path(m)
            assert gf.tolist() == f.tolist() and gl.tolist() == l.tolist(), (R, nk, name)


def test_context_is_unharmed(fx):
    """greedy tokens and avg_logprob on the same encoder output, before and after an alignment"""
    fx.encode_all()
    before = fx.hm.decode_greedy(max_new_tokens=24)
    fx.align_all(keep=0)
    after = fx.hm.decode_greedy(max_new_tokens=24)
    bits = lambda v: np.float64(v).tobytes()          # identical means the same bits (a NaN equals itself here)
    for b in range(3):
        assert before[b]["tokens"] == after[b]["tokens"] and bits(before[b]["avg_logprob"]) == bits(after[b]["avg_logprob"])
        assert bits(before[b]["no_speech_prob"]) == bits(after[b]["no_speech_prob"])
    # the alignment of what was decoded, on the state the decode left
    first, last = fx.hm.align([r["tokens"] for r in after], prompt_len=P_LEN, heads=HEADS)
    for b in range(3):
        n = len(after[b]["tokens"])
        assert first[b, P_LEN] == 0 and last[b, n - 1] == S_CACHE - 1 and (first[b, P_LEN:n] <= last[b, P_LEN:n]).all()


def _refused(hm, code, **kw):
    from norma_amd import hip
    args = dict(tokens=[[1, 2, 3, 4, 5]] * hm.batch, prompt_len=P_LEN, heads=HEADS, n_keys=None)
    args.update(kw)
    with pytest.raises(hip.HipError) as ei:
        hm.align(**args)
    assert ei.value.code == code, (kw, str(ei.value))
    first, last = hm._align_out
    assert (first == -2).all() and (last == -2).all(), "a refused call wrote its outputs"


def test_refusals(fx):
    from norma_amd import hip
    INVALID, STATE = 1, 3
    hm, V, C = fx.hm, fx.cfg.vocab_size, fx.cfg.max_target_positions
    fx.encode_all()
    _refused(hm, INVALID, heads=[])
    _refused(hm, INVALID, heads=[(0, 0)] * 33)
    for bad in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        _refused(hm, INVALID, heads=[(0, 0), bad])
    hm.set_option(hip.NH_OPT_DECODER_LAYER_LIMIT, 1)
    _refused(hm, INVALID, heads=[(1, 0)])
    hm.set_option(hip.NH_OPT_DECODER_LAYER_LIMIT, 0)
    _refused(hm, INVALID, tokens=[[1, 2, 3, 4, 5], [1, 2, 3, V, 5], [1, 2, 3, 4, 5]])
    _refused(hm, INVALID, tokens=[[1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [1, -1, 3, 4, 5]])
    _refused(hm, INVALID, tokens=[[1, 2, 3, 4, 5], [1, 2, 3], [1, 2, 3, 4, 5]])                 # n_tokens == prompt_len
    _refused(hm, INVALID, tokens=[[1] * C] * 3, n_tokens=[C, C + 1, C])
    _refused(hm, INVALID, prompt_len=0)
    _refused(hm, INVALID, prompt_len=5)
    _refused(hm, INVALID, n_keys=[1500, 0, 1500])
    _refused(hm, INVALID, n_keys=[1500, 1500, 1501])
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 1)
    _refused(hm, STATE)
    hm.set_option(hip.NH_OPT_ABSORBED_XATTN, 0)
    # a context with nothing encoded, then the same context running a pool
    h2 = common.build_hip(fx.cfg, fx.tk, overrides=fx.over, max_batch=2)
    try:
        h2.batch = 1
        _refused(h2, STATE)
        h2.pool_begin(1)
        _refused(h2, STATE)
    finally:
        h2.close()
    # and the context still aligns
    first, _ = fx.align_all(keep=0)
    assert first[0, P_LEN] == 0


# ---- the workspace after a larger one ---------------------------------------------------------------------------------------
HEADS3 = [(0, 1), (1, 0), (0, 0)]
# (heads, batch) of the calls one context takes in turn: one head, three, one again; then one clip, three, one again
CALLS = [(HEADS3[:1], 3), (HEADS3, 3), (HEADS3[:1], 3), (HEADS, 1), (HEADS, 3), (HEADS, 1)]


class Scripted:
    """test-d128 with scripted weights, three clips, and given tokens of three lengths over three key counts; every context is
    a fresh one over the weights of `base`"""

    def __init__(self):
        from norma_amd import hip, synth
        self.hip = hip
        self.cfg, self.tk = common.make_config(NAME), common.tokens_for(NAME)
        script = common.transcript_script(self.tk, n_segments=3, words_per_segment=6)
        self.base = common.build_hip(self.cfg, self.tk, overrides=common.scripted_overrides(self.cfg, self.tk, script), max_batch=1)
        self.clips = [synth.synth_pcm(0), synth.synth_pcm(1), synth.synth_pcm(2, 400000)]
        seq = [self.tk.sot, self.tk.en, self.tk.transcribe] + script
        self.tokens = [seq[:6], seq[:14], seq]
        self.fresh = {}

    def context(self):
        hm = self.hip.HipWhisper(self.cfg, max_batch=3, share_with=self.base)
        hm.set_tokens(self.tk, self.tk.en, self.tk.transcribe)
        return hm

    def call(self, hm, heads, B, keep):
        """(first, last, views or None) of one nh_align over the first B clips"""
        hm.set_option(self.hip.NH_OPT_ALIGN_KEEP, keep)
        hm.logmel(self.clips[:B])
        hm.encode()
        first, last = hm.align(self.tokens[:B], prompt_len=P_LEN, heads=heads, n_keys=N_KEYS[:B])
        views = [([hm.align_weights(b, a) for a in range(len(heads))], hm.align_matrix(b)) for b in range(B)] if keep else None
        return first, last, views

    def fresh_answer(self, heads, B, keep):
        key = (len(heads), B, keep)
        if key not in self.fresh:
            hm = self.context()
            self.fresh[key] = self.call(hm, heads, B, keep)
            hm.close()
        return self.fresh[key]


@pytest.fixture(scope="module")
def sc():
    s = Scripted()
    yield s
    s.base.close()


@pytest.mark.parametrize("keep", [0, 1])
def test_a_smaller_shape_after_a_larger_one_equals_a_fresh_context(sc, keep):
    """One context takes CALLS in turn: the workspace of a small shape is cut out of the buffer a larger shape sized (fewer
    heads after more; fewer clips after more reuses the larger carve as it is).  After every call the paths are integer-equal
    to what a context that never aligned before gives for the same call, and under NH_OPT_ALIGN_KEEP = 1 so are the views, as
    bit patterns."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    hm = sc.context()
    try:
        for i, (heads, B) in enumerate(CALLS):
            first, last, views = sc.call(hm, heads, B, keep)
            f0, l0, v0 = sc.fresh_answer(heads, B, keep)
            assert first.dtype == np.int32 and np.array_equal(first, f0) and np.array_equal(last, l0), (i, len(heads), B)
            for b in range(B):
                n = len(sc.tokens[b])
                assert first[b, P_LEN] == 0 and last[b, n - 1] == N_KEYS[b] - 1 and (first[b, n:] == -1).all()
            if keep:
                for b in range(B):
                    for a in range(len(heads)):
                        assert views[b][0][a].shape == v0[b][0][a].shape and np.array_equal(bits(views[b][0][a]), bits(v0[b][0][a])), (i, b, a)
                    assert views[b][1].shape == v0[b][1].shape and np.array_equal(bits(views[b][1]), bits(v0[b][1])), (i, b)
    finally:
        hm.close()


# ---- the host layer ---------------------------------------------------------------------------------------------------------
def _scripted_model(script):
    from norma_amd import host, synth
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    over = common.scripted_overrides(cfg, tk, script)
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    model = d.blocking_try_to_model(cfg, tk, tk.en, tk.transcribe, ((n, a.astype(np.float16)) for n, a in synth.synth_weights(cfg, 0, over)))
    return cfg, tk, over, model


def test_host_transcribe_gives_a_time_per_token():
    """host.Model.transcribe with alignment heads: one (start, end) per segment token, inside the slice, non-decreasing, and
    equal to HipWhisper.align on the same slice over the frames that hold audio; with the heads unset, what it returns today"""
    from norma_amd import synth
    tk = common.tokens_for(NAME)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=4)
    cfg, tk, over, model = _scripted_model(script)
    pcm = synth.synth_pcm(1, 400000)                                     # 25 s: 1250 of the 1500 frames hold audio
    plain = model.transcribe(pcm, final_chunk=True)
    assert len(plain) == 3 and model.last_token_times() == []
    model.set_alignment_heads(HEADS)
    segs = model.transcribe(pcm, final_chunk=True)
    times = model.last_token_times()
    assert segs == plain
    assert [len(t) for t in times] == [len(s) for s in segs]
    flat = [p for t in times for p in t]
    for (s0, e0), (s1, e1) in zip(flat, flat[1:]):
        assert s0 <= s1 and e0 <= e1
    assert all(0 <= s <= e <= 30 for s, e in flat)
    # the same slice through the C ABI
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=1)
    hm.logmel([pcm])
    hm.encode()
    toks = hm.decode_greedy()[0]["tokens"]
    assert toks == [tk.sot, tk.en, tk.transcribe] + script
    first, last = hm.align([toks], prompt_len=3, heads=HEADS, n_keys=[1250])
    hm.close()
    text = [i for i in range(3, len(toks)) if toks[i] < tk.eot]          # what the segments hold: neither timestamps nor eot
    assert [toks[i] for i in text] == [t for s in segs for t in s]
    want = [(float(np.float32(0.02) * np.float32(first[0, i])), float(np.float32(0.02) * np.float32(last[0, i] + 1))) for i in text]
    assert flat == want
    assert flat[-1][1] <= 25.0
    # and off again
    model.set_alignment_heads([])
    assert model.transcribe(pcm, final_chunk=True) == plain and model.last_token_times() == []
    model.close()


def test_checkpoint_alignment_heads_are_remembered_not_enabled(tmp_path):
    import json
    import os
    from norma_amd import host, synth
    from test_gpu_transcribe import _write_checkpoint_dir
    cfg, tk = common.make_config(NAME), common.tokens_for(NAME)
    script = common.transcript_script(tk, n_segments=2, words_per_segment=3)
    over = common.scripted_overrides(cfg, tk, script)
    _write_checkpoint_dir(str(tmp_path), cfg, tk, synth.synth_weights(cfg, 0, over))
    d = host.Definition(host.ModelType.TinyEn, host.SelectedDevice.Rocm(0))
    model = d.blocking_try_to_model_from_dir(str(tmp_path))
    assert model.checkpoint_alignment_heads() == []
    model.close()
    with open(os.path.join(tmp_path, "generation_config.json"), "w") as f:
        json.dump(dict(alignment_heads=[[1, 0], [0, 1]], max_length=448), f)
    model = d.blocking_try_to_model_from_dir(str(tmp_path))
    assert model.checkpoint_alignment_heads() == [(1, 0), (0, 1)]
    pcm = synth.synth_pcm(0, 200000)
    segs = model.transcribe(pcm, final_chunk=True)
    assert len(segs) == 2 and model.last_token_times() == []            # remembered, not enabled
    model.set_alignment_heads(model.checkpoint_alignment_heads())
    assert model.transcribe(pcm, final_chunk=True) == segs
    assert [len(t) for t in model.last_token_times()] == [len(s) for s in segs]
    model.close()
