"""Token-level timestamps, the part that needs no GPU: the references of tests/align_ref.py are checked against independent
formulations (brute force, np.median, the C oracle), and the library must declare, list and export nh_align."""
import itertools

import numpy as np
import pytest

import align_ref as AR
import common
from norma_amd import hip


@pytest.mark.parametrize("R,nk", list(itertools.product(range(1, 6), range(1, 6))))
def test_reference_dtw_is_optimal_and_well_formed(R, nk):
    """the recurrence's end cost equals the least cost over all monotone paths; first / last are contiguous, monotone and
    cover 0 .. nk - 1.  (Without ties among c0, c1, c2: where c0 == c1 < c2 the contract's rule -- the usual recipe's --
    takes c2, which is not the least; the matrices here have no such tie.)"""
    rng = np.random.default_rng([R, nk])
    for trial in range(4):
        # multiples of 2^-14 in [-16, 16]: every sum of <= 9 cells is exact in f32, so the f32 recurrence and the f64 brute force
        # agree exactly, and equal partial sums do not occur
        M = rng.integers(-2 ** 18, 2 ** 18 + 1, size=(R, nk)).astype(np.float32) / 2 ** 14
        first, last, cost = AR.dtw(M)
        assert float(cost) == AR.dtw_brute(M)
        assert first[0] == 0 and last[-1] == nk - 1
        assert (first <= last).all()
        assert ((first[1:] == last[:-1]) | (first[1:] == last[:-1] + 1)).all()     # contiguous: no key skipped, none revisited


@pytest.mark.parametrize("R,nk", [(1, 1), (1, 6), (6, 1), (4, 7), (7, 4)])
def test_reference_dtw_tie_rule_on_an_equal_matrix(R, nk):
    """all costs equal: c0 is never strictly least, c1 wins over c2 only where the row above is cheaper, so the path stays on
    key 0 down to the last row and runs along it"""
    first, last, _ = AR.dtw(np.zeros((R, nk), np.float32))
    assert first.tolist() == [0] * R
    assert last.tolist() == [0] * (R - 1) + [nk - 1]


@pytest.mark.parametrize("R,nk", [(1, 1), (3, 9), (9, 3), (20, 7), (33, 40)])
def test_reference_dtw_by_diagonals_is_the_same_recurrence(R, nk):
    rng = np.random.default_rng([7, R, nk])
    planted, pf, pl = AR.planted_path(R, nk, rng)
    assert AR.dtw(planted)[0].tolist() == pf.tolist() and AR.dtw(planted)[1].tolist() == pl.tolist()
    for M in (rng.standard_normal((R, nk)), np.zeros((R, nk)), rng.integers(-2, 3, (R, nk)), planted):   # integers: many exact ties
        a, b = AR.dtw(M), AR.dtw_diagonals(M)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2]


@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 8, 64])
def test_reference_median_is_numpy_median_over_reflect_padding(nk):
    z = np.random.default_rng(nk).standard_normal((3, 5, nk))
    got = AR.median_filter(z)
    if nk <= 3:
        assert np.array_equal(got, z)
        return
    pad = np.pad(z, [(0, 0), (0, 0), (3, 3)], mode="reflect")
    want = np.stack([np.median(pad[..., s:s + 7], axis=-1) for s in range(nk)], axis=-1)
    assert np.array_equal(got, want)
    assert not np.array_equal(AR.median_filter(z, edge=True), want)            # the edge-repeating mutation is a different filter


def test_median_selection_network_of_the_kernel():
    """the 13 exchanges align_reduce_kernel uses put the median of 7 in the middle: by the zero-one principle it is enough
    that they do so for all 128 inputs of zeros and ones"""
    net = [(0, 5), (0, 3), (1, 6), (2, 4), (0, 1), (3, 5), (2, 6), (2, 3), (3, 6), (4, 5), (1, 4), (1, 3), (3, 4)]
    for bits in itertools.product((0, 1), repeat=7):
        z = list(bits)
        for a, b in net:
            z[a], z[b] = min(z[a], z[b]), max(z[a], z[b])
        assert z[3] == sorted(bits)[3], bits


def test_zscore_reference():
    W = np.random.default_rng(0).random((2, 9, 5))
    z, mean, sd = AR.zscore(W)
    assert np.allclose(z, (W - W.mean(axis=1, keepdims=True)) / W.std(axis=1, keepdims=True), rtol=1e-12, atol=0)
    assert np.array_equal(AR.zscore(W[:, :1])[0], np.zeros((2, 1, 5)))         # one row: std == 0 -> 0


def test_chain_matches_the_oracle_decoder():
    """the float64 chain's final hidden state against OracleModel.decoder_forward (f32 C) on test-d128: proves the chain"""
    name = "test-d128"
    cfg, tk = common.make_config(name), common.tokens_for(name)
    om = common.build_oracle(cfg, tk)
    rng = np.random.default_rng(3)
    xa = rng.standard_normal((40, cfg.d_model)).astype(np.float32)
    tokens = [tk.sot, tk.en, tk.transcribe, tk.zero_sec] + [int(t) for t in rng.integers(300, 40000, 8)]
    want = om.decoder_forward(tokens, xa, True)
    om.close()
    got = AR.chain(cfg, AR.decoder_weights(cfg), tokens, xa)
    assert got["q"].shape == (cfg.decoder_layers, len(tokens), cfg.d_model) and got["k"].shape == (cfg.decoder_layers, 40, cfg.d_model)
    assert np.abs(got["hidden"] - want).max() <= 1e-5
    # the fp16-rounded evaluation is a different, nearby function
    r = AR.chain(cfg, AR.decoder_weights(cfg), tokens, xa, rounded=True)
    assert 0 < np.abs(r["hidden"] - got["hidden"]).max() < 2e-2


def test_library_declares_lists_and_exports_nh_align():
    with open(hip.HEADER_PATH) as f:
        header = f.read()
    L = hip.load_library()
    for s in ("nh_align", "nh_align_weights", "nh_align_matrix", "nh_align_path"):
        assert f"int {s}(" in header, s
        assert s in hip.declared_symbols(), s
        assert hasattr(L, s), s
    assert "#define NH_OPT_ALIGN_KEEP 4" in header and hip.NH_OPT_ALIGN_KEEP == 4
    assert "#define NH_ALIGN_MAX_HEADS 32" in header and hip.NH_ALIGN_MAX_HEADS == 32
