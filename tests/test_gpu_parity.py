"""GPU parity tests: the HIP path (through the C ABI, norma_amd/hip.py -> libnorma_hip.so) against
the CPU oracle on the same seeded inputs, and against the committed golden fixtures.

Bars (DESIGN.md "Parity"):
  * token ids, masks, argmax decisions: bit-exact;
  * log-mel: |d| <= 2e-5 (same operation order as the reference's f32 FFT; libm log10/cos differ by ulps);
  * encoder output (unit-variance LayerNorm output): max |d| <= 2e-3 for the reduced configs and
    tiny.en (fp16 operands with fp32 accumulation vs f32);
  * decoder logits: max |d| <= 4e-3 * logit std;
  * greedy tokens identical to the oracle wherever the oracle's own top-2 relative margin is above
    the stated fp tolerance (golden `first_risky_step`); the scripted fixtures have margins ~1 at
    every step, so identity is asserted over the whole transcript there.
"""
import json
import math
import os

import numpy as np
import pytest

import common
from norma_amd import assets_io, config, synth, vocab

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_golden.json")))


def _hip():
    from norma_amd import hip
    assert hip.device_count() >= 1, "no MI355X visible: the GPU tests need the HIP path, there is no fallback"
    return hip


def _oracle():
    from oracle import oracle as O
    return O


# --------------------------------------------------------------------------------------------------- mel
@pytest.mark.parametrize("name", ["test-d128", "test-d256-mel128"])
def test_logmel_matches_oracle_including_ragged_clips(name):
    O = _oracle()
    _hip()
    cfg = common.make_config(name, encoder_layers=0, decoder_layers=0)
    tk = common.tokens_for(name)
    hm = common.build_hip(cfg, tk, max_batch=4)
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    clips = [synth.synth_pcm(0), synth.synth_pcm(1, 400000), synth.synth_pcm(2, 16000), np.zeros(480000, np.float32)]
    hm.logmel(clips)
    for b, c in enumerate(clips):
        ref = O.pcm_to_mel(c, filt)[:, :3000]
        got = hm.get_mel(b)
        assert np.abs(got - ref).max() <= 2e-5, (name, b)
    # all-silent clip: every bin sits at the 1e-10 floor -> (-10 max -8 clamp)/4 + 1 = -1.5
    assert np.all(hm.get_mel(3) == np.float32(-1.5))
    hm.close()


def test_logmel_golden_and_mixed_frame_counts_rejected():
    hip = _hip()
    cfg = common.make_config("test-d128", encoder_layers=0, decoder_layers=0)
    hm = common.build_hip(cfg, common.tokens_for("test-d128"), max_batch=2)
    for key, g in GOLDEN["mel"].items():
        n_mel, n = (int(x) for x in key.split("/"))
        if n_mel != cfg.num_mel_bins:
            continue
        hm.logmel([synth.synth_pcm(2, n)])
        mel = hm.get_mel(0)
        for c, col in g["cols"].items():
            assert np.abs(mel[:, int(c)] - np.array(col)).max() <= 2e-5
        assert abs(mel.astype(np.float64).sum() - g["sum"]) < 1.0
    with pytest.raises(hip.HipError):  # a 100-sample clip yields 1500 frames, a 30 s clip 3000
        hm.logmel([synth.synth_pcm(0), synth.synth_pcm(1, 100)])
    with pytest.raises(hip.HipError):
        hm.logmel([np.zeros(480001, np.float32)])
    hm.close()


# --------------------------------------------------------------------------------------------------- layers
def _stage_parity(name, enc, dec, B, seed=0):
    O = _oracle()
    cfg = common.make_config(name, encoder_layers=enc, decoder_layers=dec)
    tk = common.tokens_for(name)
    om = common.build_oracle(cfg, tk, seed=seed)
    hm = common.build_hip(cfg, tk, seed=seed, max_batch=B)
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    clips = [synth.synth_pcm(k) for k in range(B)]
    mels = np.stack([O.pcm_to_mel(c, filt)[:, :3000] for c in clips])
    hm.set_mel(mels)   # encoder in isolation: identical mel on both sides
    hm.encode()
    toks = np.array([[tk.sot, tk.en, tk.transcribe, tk.zero_sec, 100 + b, 2000, 30000, tk.zero_sec + 40] for b in range(B)],
                    dtype=np.int32)
    hid = hm.decoder_forward(toks)
    out = []
    for b in range(B):
        xa = om.encoder_forward(mels[b])
        enc_err = np.abs(hm.encoder_output(b) - xa).max()
        ref_h = om.decoder_forward(toks[b], xa, True)
        ref_l = om.final_linear(ref_h)
        got_l = hm.final_linear(hid[b])
        out.append(dict(enc_err=enc_err, hid_err=np.abs(hid[b] - ref_h).max(),
                        logit_err=np.abs(got_l - ref_l).max(), logit_std=ref_l.std(),
                        top1=(got_l.argmax(1) == ref_l.argmax(1)).mean()))
    hm.close(); om.close()
    return out


# the last case is distil-large-v3 at full WIDTH (d = 1280, 20 heads, V = 51866) with one layer each: the shapes the bench
# runs -- persistent 256 x 256 GEMM with every epilogue, head-major cross K/V, tile-major GEMV weights, 10-step fused
# LayerNorm -- checked against the oracle, not only for self-consistency
@pytest.mark.parametrize("name,enc,dec,B", [("test-d128", 0, 1, 2), ("test-d128", 2, 2, 3), ("test-d256-mel128", 2, 2, 2),
                                            ("distil-large-v3", 1, 1, 2),
                                            # the remaining widths of the reference's model table (d = 512, 768, 1024), one layer each
                                            ("base.en", 1, 1, 1), ("small.en", 1, 1, 2), ("medium.en", 1, 1, 1)])
def test_encoder_and_decoder_layers_match_oracle(name, enc, dec, B):
    for r in _stage_parity(name, enc, dec, B):
        assert r["enc_err"] <= 2e-3, r
        assert r["hid_err"] <= 5e-3, r
        assert r["logit_err"] <= 4e-3 * max(r["logit_std"], 0.1), r


def test_tiny_en_layers_match_oracle():
    for r in _stage_parity("tiny.en", 4, 4, 1):
        assert r["enc_err"] <= 2e-3, r
        assert r["logit_err"] <= 4e-3 * r["logit_std"], r


# --------------------------------------------------------------------------------------------------- rules
def test_logit_rules_kernel_is_bit_exact_with_oracle_rules():
    O = _oracle()
    from test_oracle import _rule_cases
    for name in ("test-d128", "test-d256-mel128"):
        cfg = common.make_config(name, encoder_layers=0, decoder_layers=0)
        tk = common.tokens_for(name)
        om = O.OracleModel(cfg, tk, tk.en, tk.transcribe)
        hm = common.build_hip(cfg, tk, max_batch=2)
        rng = np.random.default_rng(11)
        cases = _rule_cases(tk, cfg.vocab_size, rng)
        # NaN handling of total_cmp: a positive NaN beats every probability
        p_nan = cases[0][1].copy(); p_nan[tk.zero_sec + 5] = np.nan
        cases.append(("nan", p_nan, cases[0][2], cases[0][3]))
        # exact ties resolve to the highest index (Iterator::max_by keeps the last maximum)
        p_tie = np.zeros(cfg.vocab_size, np.float32); p_tie[[500, 900]] = 0.5
        cases.append(("tie", p_tie, [tk.sot, tk.en, tk.transcribe, tk.zero_sec, tk.zero_sec + 1], tk.zero_sec + 1))
        for label, p, toks, last in cases:
            ref = om.apply_rules(p, toks, last)
            got, am = hm.apply_rules(p, toks, last)
            assert np.array_equal(got, ref, equal_nan=True), (name, label)
            import ctypes as C
            ref_am = O.lib().wo_argmax_total(ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref))
            assert am == ref_am, (name, label)
        hm.close(); om.close()


# --------------------------------------------------------------------------------------------------- decode
def _check_decode_against_golden(m, B):
    cfg = config.preset(m["config"])
    tk = common.tokens_for(m["config"])
    over = None
    if m["scripted"]:
        over = common.scripted_overrides(cfg, tk, common.transcript_script(tk, n_segments=5, words_per_segment=8))
    hm = common.build_hip(cfg, tk, seed=m["seed"], overrides=over, max_batch=B)
    ks = sorted(int(k) for k in m["clips"])
    clips = [synth.synth_pcm(k) for k in ks] * (B // len(ks))
    hm.logmel(clips)
    hm.encode()
    res = hm.decode_greedy()
    for i, r in enumerate(res):
        c = m["clips"][str(ks[i % len(ks)])]
        ref = c["tokens"]
        risky = c["first_risky_step"]
        n_strict = len(ref) if risky < 0 else 3 + risky
        assert r["tokens"][:n_strict] == ref[:n_strict], (m["config"], m["scripted"], i)
        assert abs(r["no_speech_prob"] - c["no_speech_prob"]) <= 0.02 * c["no_speech_prob"] + 1e-9
        if risky < 0:
            assert r["tokens"] == ref
            if c["avg_logprob"] is None:
                assert math.isnan(r["avg_logprob"])
            else:
                assert abs(r["avg_logprob"] - c["avg_logprob"]) <= 5e-3
        xa = hm.encoder_output(i)
        for row, vals in c["enc_rows"].items():
            assert np.abs(xa[int(row)][:len(vals)] - np.array(vals)).max() <= 2e-3
    hm.close()
    return res


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_greedy_tokens_match_golden_reduced_configs(idx):
    _hip()
    _check_decode_against_golden(GOLDEN["models"][idx], B=2)


def test_greedy_tokens_match_golden_tiny_en():
    _hip()
    _check_decode_against_golden(GOLDEN["models"][3], B=2)


def test_scripted_tiny_en_full_transcript_identical_to_oracle_and_batch_invariant():
    """Config 2 of BASELINE.json (tiny.en fp16 b1, token-match vs CPU) on a non-degenerate decode:
    a 100+-token scripted transcript; also the same clips at B=4 vs B=1 give identical outputs."""
    O = _oracle()
    name = "tiny.en"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=10, words_per_segment=10, seed=9)
    over = common.scripted_overrides(cfg, tk, script)
    om = common.build_oracle(cfg, tk, overrides=over)
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    clips = [synth.synth_pcm(k) for k in range(4)]
    hm4 = common.build_hip(cfg, tk, overrides=over, max_batch=4)
    hm4.logmel(clips); hm4.encode()
    r4 = hm4.decode_greedy()
    hm1 = common.build_hip(cfg, tk, overrides=over, max_batch=1)
    for b in range(4):
        if b < 2:
            xa = om.encoder_forward(O.pcm_to_mel(clips[b], filt))
            ref = om.decode(xa)
            assert ref["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
            assert r4[b]["tokens"] == ref["tokens"]
            assert abs(r4[b]["avg_logprob"] - ref["avg_logprob"]) <= 5e-3
            assert abs(r4[b]["no_speech_prob"] - ref["no_speech_prob"]) <= 0.02 * ref["no_speech_prob"] + 1e-9
        hm1.logmel([clips[b]]); hm1.encode()
        r1 = hm1.decode_greedy()[0]
        assert r1["tokens"] == r4[b]["tokens"]
        assert r1["avg_logprob"] == r4[b]["avg_logprob"] and r1["no_speech_prob"] == r4[b]["no_speech_prob"]
    hm1.close(); hm4.close(); om.close()


def test_no_speech_early_exit_and_max_new_tokens_knob():
    """model.rs:308-315: no_speech_prob > 0.6 returns the bare prompt with avg_logprob 0."""
    name = "test-d128"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    # positional row 0 carries the no-speech token: the position-0 logits put their mass there
    over = common.scripted_overrides(cfg, tk, [tk.zero_sec, 500, tk.eot])
    emb = over["model.decoder.embed_tokens.weight"]
    pos = over["model.decoder.embed_positions.weight"].copy()
    pos[0] += np.float32(4.0) * emb[tk.no_speech]
    over["model.decoder.embed_positions.weight"] = pos.astype(np.float16).astype(np.float32)
    om = common.build_oracle(cfg, tk, overrides=over)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=1)
    O = _oracle()
    clip = synth.synth_pcm(0)
    xa = om.encoder_forward(O.pcm_to_mel(clip, assets_io.mel_filters(cfg.num_mel_bins)))
    ref = om.decode(xa)
    hm.logmel([clip]); hm.encode()
    got = hm.decode_greedy()[0]
    assert ref["no_speech_prob"] > 0.6 and ref["tokens"] == [tk.sot, tk.en, tk.transcribe]
    assert got["tokens"] == ref["tokens"] and got["no_speech_exit"] and got["avg_logprob"] == 0.0
    assert abs(got["no_speech_prob"] - ref["no_speech_prob"]) < 1e-3
    hm.close(); om.close()
    # bench knob: max_new_tokens caps the generated tokens and appends eot, same as the oracle's knob
    om = common.build_oracle(cfg, tk)
    hm = common.build_hip(cfg, tk, max_batch=1)
    xa = om.encoder_forward(O.pcm_to_mel(clip, assets_io.mel_filters(cfg.num_mel_bins)))
    hm.logmel([clip]); hm.encode()
    a, b = om.decode(xa, max_new_tokens=6), hm.decode_greedy(max_new_tokens=6)[0]
    assert len(b["tokens"]) == len(a["tokens"]) and b["tokens"][-1] == tk.eot
    hm.close(); om.close()


# --------------------------------------------------------------------------------------------------- full size
def test_distil_large_v3_b32_size_independent_properties():
    """BASELINE.json config 3 at full size (the oracle needs minutes per chunk there): determinism,
    batch invariance (chunk k alone == chunk k inside the batch of 32), and well-formedness."""
    _hip()
    name = "distil-large-v3"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=8, words_per_segment=12, seed=3)
    over = common.scripted_overrides(cfg, tk, script)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=32)
    clips = [synth.synth_pcm(k) for k in range(32)]
    hm.logmel(clips); hm.encode()
    r32 = hm.decode_greedy()
    hm.logmel(clips); hm.encode()
    again = hm.decode_greedy()
    for a, b in zip(r32, again):
        assert a["tokens"] == b["tokens"] and a["avg_logprob"] == b["avg_logprob"]
    for r in r32:
        assert r["tokens"] == [tk.sot, tk.en, tk.transcribe] + script   # margins ~1: audio-independent argmax
        assert r["avg_logprob"] > -1.0 and 0.0 <= r["no_speech_prob"] < 0.6
    enc5 = hm.encoder_output(5)
    hm.logmel([clips[5], clips[17]]); hm.encode()
    r2 = hm.decode_greedy()
    assert np.array_equal(hm.encoder_output(0), enc5)          # bit-exact batch invariance
    assert r2[0]["tokens"] == r32[5]["tokens"] and r2[0]["avg_logprob"] == r32[5]["avg_logprob"]
    assert r2[1]["tokens"] == r32[17]["tokens"] and r2[1]["no_speech_prob"] == r32[17]["no_speech_prob"]
    assert np.isfinite(enc5).all() and abs(float(enc5.std()) - 1.0) < 0.25
    hm.close()


def test_batch_64_paths_are_batch_invariant_and_match_the_oracle():
    """max_batch = 64 (BASELINE.json config 5 uses b64): exercises the 4-column-block decoder kernels; every clip must
    give exactly what it gives alone, and clip 0 must match the oracle."""
    O = _oracle()
    name = "test-d256-mel128"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=6, seed=21)
    over = common.scripted_overrides(cfg, tk, script)
    hm = common.build_hip(cfg, tk, seed=1, overrides=over, max_batch=64)
    clips = [synth.synth_pcm(k, 480000 if k % 3 else 320000) for k in range(64)]
    hm.logmel(clips); hm.encode()
    r64 = hm.decode_greedy()
    h1 = common.build_hip(cfg, tk, seed=1, overrides=over, max_batch=1)
    for b in (0, 17, 63):
        h1.logmel([clips[b]]); h1.encode()
        r1 = h1.decode_greedy()[0]
        assert r1["tokens"] == r64[b]["tokens"] and r1["avg_logprob"] == r64[b]["avg_logprob"]
    om = common.build_oracle(cfg, tk, seed=1, overrides=over)
    ref = om.decode(om.encoder_forward(O.pcm_to_mel(clips[0], assets_io.mel_filters(cfg.num_mel_bins))))
    assert r64[0]["tokens"] == ref["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
    assert abs(r64[0]["avg_logprob"] - ref["avg_logprob"]) <= 5e-3
    hm.close(); h1.close(); om.close()


def test_clip_shorter_than_one_hop_uses_the_1500_frame_path():
    """pcm_to_mel yields 1500 frames (not 3000) for a clip shorter than one hop (160 samples), so the encoder sees
    750 positions (SURVEY.md 3.3[A]-2); 750 is not a multiple of 4, which exercises the scalar V^T tail stores."""
    O = _oracle()
    name = "test-d128"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=2, words_per_segment=3)
    over = common.scripted_overrides(cfg, tk, script)
    om = common.build_oracle(cfg, tk, overrides=over)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=2)
    filt = assets_io.mel_filters(cfg.num_mel_bins)
    clips = [synth.synth_pcm(0, 100), synth.synth_pcm(1, 159)]
    hm.logmel(clips)
    hm.encode()
    res = hm.decode_greedy()
    for b, c in enumerate(clips):
        mel = O.pcm_to_mel(c, filt)
        assert mel.shape[1] == 1500
        assert np.abs(hm.get_mel(b, frames=1500) - mel).max() <= 2e-5
        xa = om.encoder_forward(mel)
        assert xa.shape[0] == 750
        assert np.abs(hm.encoder_output(b, S=750) - xa).max() <= 2e-3
        ref = om.decode(xa)
        assert res[b]["tokens"] == ref["tokens"]
    # and the context goes back to full-length clips afterwards (the zero framing rows move with the frame count)
    full = synth.synth_pcm(2)
    hm.logmel([full]); hm.encode()
    xa = om.encoder_forward(O.pcm_to_mel(full, filt))
    assert np.abs(hm.encoder_output(0) - xa).max() <= 2e-3
    hm.close(); om.close()


@pytest.mark.gpu
def test_fused_layernorm_decode_and_graph_replay_are_bit_identical_to_the_plain_path():
    """The decode step fuses every LayerNorm into the projection that consumes it (skinny_ln_kernel, the logits staging
    pass) and is replayed from a hipGraph.  nh_set_option switches either off (stand-alone sliced LayerNorm + plain GEMV;
    eager launches with the position passed by value); all four combinations must give the same tokens and bit-identical
    log-probabilities (one summation tree, one rounding sequence: nh_kernels.h)."""
    from norma_amd import hip
    name = "test-d256-mel128"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=6, seed=21)
    hm = common.build_hip(cfg, tk, seed=1, overrides=common.scripted_overrides(cfg, tk, script), max_batch=3)
    hm.logmel([synth.synth_pcm(k, 480000) for k in (17, 4, 9)]); hm.encode()
    outs = []
    for graphs in (1, 0):
        for fuse in (1, 0):
            hm.set_option(hip.NH_OPT_DECODE_GRAPHS, graphs)
            hm.set_option(hip.NH_OPT_FUSE_DECODE_LAYERNORM, fuse)
            r = hm.decode_greedy()
            outs.append([[x["tokens"], x["avg_logprob"].hex(), x["no_speech_prob"].hex()] for x in r])
    assert outs[0] == outs[1] == outs[2] == outs[3]
    assert len(outs[0][0][0]) > 10
    hm.close()


@pytest.mark.gpu
def test_set_tokens_after_a_decode_recaptures_the_step_graph():
    """The captured decode step carries the rule token ids by value: a second nh_set_tokens must not replay the old ids
    (ADVICE r01).  Decode, re-declare the special tokens with a different eot / timestamp origin, decode again: both
    passes must match the oracle configured the same way."""
    import dataclasses
    O = _oracle()
    name = "test-d128"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=2, words_per_segment=4, seed=8)
    over = common.scripted_overrides(cfg, tk, script)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=1)
    clip = synth.synth_pcm(3)
    mel = O.pcm_to_mel(clip, assets_io.mel_filters(cfg.num_mel_bins))
    hm.logmel([clip]); hm.encode()
    first = hm.decode_greedy()[0]
    om = common.build_oracle(cfg, tk, overrides=over)
    xa = om.encoder_forward(mel)
    assert first["tokens"] == om.decode(xa)["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
    om.close()
    # new ids: the FIRST text token of the script becomes eot -> the transcript must now stop there
    tk2 = dataclasses.replace(tk, eot=script[1])
    hm.set_tokens(tk2, tk2.en, tk2.transcribe)
    second = hm.decode_greedy()[0]
    om2 = O.OracleModel(cfg, tk2, tk2.en, tk2.transcribe)
    for n, a in synth.synth_weights(cfg, 0, over):
        om2.set_tensor(n, a)
    ref2 = om2.decode(om2.encoder_forward(mel))
    assert second["tokens"] == ref2["tokens"]
    assert second["tokens"] != first["tokens"] and second["tokens"][-1] == script[1]
    hm.close(); om2.close()


@pytest.mark.gpu
def test_distil_large_v3_full_depth_one_clip_matches_the_oracle():
    """The bench model at FULL size (32 encoder layers, 2 decoder layers, d = 1280, V = 51866), one clip, against the oracle
    end to end: encoder output, every greedy token of a scripted transcript, avg_logprob, no_speech_prob.  (~10 s of
    oracle time on the box's host cores; the b32 test above then carries this single-clip result to the whole batch by
    bit-exact batch invariance.)"""
    O = _oracle()
    name = "distil-large-v3"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=6, seed=5)
    over = common.scripted_overrides(cfg, tk, script)
    hm = common.build_hip(cfg, tk, overrides=over, max_batch=1)
    om = common.build_oracle(cfg, tk, overrides=over)
    clip = synth.synth_pcm(7)
    hm.logmel([clip]); hm.encode()
    got = hm.decode_greedy()[0]
    xa = om.encoder_forward(O.pcm_to_mel(clip, assets_io.mel_filters(cfg.num_mel_bins)))
    enc_err = np.abs(hm.encoder_output(0) - xa).max()
    assert enc_err <= 4e-3, enc_err          # 32 layers of fp16-operand GEMMs on a unit-variance output
    ref = om.decode(xa)
    assert got["tokens"] == ref["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
    assert abs(got["avg_logprob"] - ref["avg_logprob"]) <= 5e-3
    assert abs(got["no_speech_prob"] - ref["no_speech_prob"]) <= 0.02 * ref["no_speech_prob"] + 1e-9
    # The same clip with cross-attention computed on the encoder output itself (NH_OPT_ABSORBED_XATTN, a numerics prototype of
    # u = Wk^T q, z = p^T xa, o = Wv z + bv, fp16 roundings on u, p and z instead of on K and V): the same
    # bars against the oracle.  (The whole parity suite passes with it switched on: profiles/r03_pytest_absorbed_xattn.log;
    # large-v3 at 32 decoder layers: hidden 1.88e-3 against 1.78e-3, logits 1.75e-3 sigma against 1.85e-3.)
    hip = _hip()
    for form in (1, 2):      # 1: the slow prototype, 2: the one-pass kernels (xa streamed once per layer, MFMA, transposed LDS reads)
        hm.set_option(hip.NH_OPT_ABSORBED_XATTN, form)
        hm.logmel([clip]); hm.encode()
        alt = hm.decode_greedy()[0]
        assert alt["tokens"] == ref["tokens"], form
        assert abs(alt["avg_logprob"] - ref["avg_logprob"]) <= 5e-3, form
        assert abs(alt["no_speech_prob"] - ref["no_speech_prob"]) <= 0.02 * ref["no_speech_prob"] + 1e-9, form
        assert alt["avg_logprob"] != got["avg_logprob"]      # it really is another arithmetic
    hm.close(); om.close()


def test_absorbed_cross_attention_one_pass_kernels_are_batch_invariant_bit_for_bit():
    """NH_OPT_ABSORBED_XATTN = 2 keeps the invariant the lockstep / joint / pool machinery rests on: a clip alone == the clip in a
    batch (the key ranges and every summation order are fixed, whatever the number of rows): 1 row against 37 (base.en, d = 512,
    8 heads) and against 5 (distil-large-v3, d = 1280, 20 heads)."""
    hip = _hip()
    for name, nb in (("base.en", 37), ("distil-large-v3", 5)):
        cfg = config.preset(name)
        tk = common.tokens_for(name)
        script = common.transcript_script(tk, n_segments=2, words_per_segment=5, seed=3)
        over = common.scripted_overrides(cfg, tk, script)
        hm = common.build_hip(cfg, tk, overrides=over, max_batch=nb)
        h1 = hip.HipWhisper(cfg, device=0, max_batch=1, share_with=hm)
        h1.set_tokens(tk, tk.en, tk.transcribe)
        for h in (hm, h1):
            h.set_option(hip.NH_OPT_ABSORBED_XATTN, 2)
        clips = np.stack([synth.synth_pcm(k) for k in range(nb)])
        hm.logmel_array(clips); hm.encode()
        batch = hm.decode_greedy()
        for k in (0, nb // 2, nb - 1):
            h1.logmel_array(np.ascontiguousarray(clips[k:k + 1])); h1.encode()
            one = h1.decode_greedy()[0]
            assert one["tokens"] == batch[k]["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
            assert one["avg_logprob"] == batch[k]["avg_logprob"] and one["no_speech_prob"] == batch[k]["no_speech_prob"]
        hm.close(); h1.close()


def test_encoder_batches_decoded_together_give_what_they_give_alone():
    """nh_logmel_device_rows / nh_encode_rows + one nh_decode_greedy over all rows (r03: the decoder weights and the tied
    embedding are streamed once per token for several encoder batches).  Rows filled 32 + 32 (distil-large-v3: the 64-row
    logits run through two K-phases of skinny_ldsp_kernel) and 8 + 8 + 5 on a small model (ragged last group, 96-row
    dispatch with 6 row blocks at 16 + 40 + 40): every clip's tokens, log-probs and encoder output must equal, bit for bit,
    what the same clip gives in a batch of its own."""
    hip = _hip()
    for name, groups, script_seed in (("test-d256-mel128", (8, 8, 5), 17), ("test-d256-mel128", (16, 40, 40), 18),
                                      ("distil-large-v3", (32, 32), 3)):
        cfg = config.preset(name)
        tk = common.tokens_for(name)
        script = common.transcript_script(tk, n_segments=3, words_per_segment=5, seed=script_seed)
        over = common.scripted_overrides(cfg, tk, script)
        total = sum(groups)
        hm = common.build_hip(cfg, tk, overrides=over, max_batch=total)
        h1 = hip.HipWhisper(cfg, device=0, max_batch=max(groups), share_with=hm)
        h1.set_tokens(tk, tk.en, tk.transcribe)
        clips = np.stack([synth.synth_pcm(k) for k in range(total)])
        row0, alone = 0, []
        for g in groups:
            part = np.ascontiguousarray(clips[row0:row0 + g])
            hm.logmel_array_rows(part, row0)
            hm.encode_rows(row0, g)
            h1.logmel_array(part); h1.encode()
            alone.extend(h1.decode_greedy())
            if row0 == 0:
                enc_alone = h1.encoder_output(g - 1)
                enc_row = g - 1
            row0 += g
        joint = hm.decode_greedy()
        assert len(joint) == total == len(alone)
        for a, b in zip(joint, alone):
            assert a["tokens"] == b["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
            assert a["avg_logprob"] == b["avg_logprob"] and a["no_speech_prob"] == b["no_speech_prob"]
        assert np.array_equal(hm.encoder_output(enc_row), enc_alone)
        assert len({r["avg_logprob"] for r in joint}) > 1
        # a new set of rows starts over at row 0; a gap is refused
        hm.logmel_array_rows(np.ascontiguousarray(clips[:groups[0]]), 0)
        with pytest.raises(hip.HipError):
            hm.logmel_array_rows(np.ascontiguousarray(clips[:2]), groups[0] + 1)
        hm.close(); h1.close()


def test_refilling_a_middle_row_keeps_the_batch_the_library_decodes():
    """HipWhisper.batch sizes every output array, so it has to be the library's own count of rows (commit_batch of
    nh_encode.hip: rows above 0 only ever extend the batch; nh_pool_begin: the pool's rows).  Rows [0,1), [1,3), then [1,2)
    again: the library decodes 3 rows, clips 0, 3 and 2, each bit for bit what it gives alone."""
    hip = _hip()
    name = "test-d256-mel128"
    cfg = config.preset(name)
    tk = common.tokens_for(name)
    script = common.transcript_script(tk, n_segments=3, words_per_segment=5, seed=17)
    hm = common.build_hip(cfg, tk, overrides=common.scripted_overrides(cfg, tk, script), max_batch=3)
    h1 = hip.HipWhisper(cfg, device=0, max_batch=1, share_with=hm)
    h1.set_tokens(tk, tk.en, tk.transcribe)
    clips = np.stack([synth.synth_pcm(k) for k in range(4)])
    alone, enc_alone = [], []
    for k in range(4):
        h1.logmel_array(np.ascontiguousarray(clips[k:k + 1])); h1.encode()
        alone.extend(h1.decode_greedy())
        enc_alone.append(h1.encoder_output(0))
    for row0, first, n in ((0, 0, 1), (1, 1, 2), (1, 3, 1)):
        hm.logmel_array_rows(np.ascontiguousarray(clips[first:first + n]), row0)
        hm.encode_rows(row0, n)
    assert hm.batch == 3
    joint = hm.decode_greedy()
    assert len(joint) == 3
    for row, clip in enumerate((0, 3, 2)):
        a, b = joint[row], alone[clip]
        assert a["tokens"] == b["tokens"] == [tk.sot, tk.en, tk.transcribe] + script
        assert a["avg_logprob"] == b["avg_logprob"] and a["no_speech_prob"] == b["no_speech_prob"]
        assert np.array_equal(hm.encoder_output(row), enc_alone[clip])
    assert not np.array_equal(enc_alone[1], enc_alone[3])   # row 1 does hold the refill, not what it held before
    # the same shadow under a pool: its rows, then the staging rows above them
    hm.pool_begin(1)
    assert hm.batch == 1
    hm.logmel_array_rows(np.ascontiguousarray(clips[1:3]), 1)
    assert hm.batch == 3
    hm.logmel_array_rows(np.ascontiguousarray(clips[3:4]), 1)
    assert hm.batch == 3
    hm.close(); h1.close()
