"""GPU: the two scoring kernels (score_logits_kernel, score_merge_kernel; norma_amd/csrc/k_score.hip) on raw device buffers
through tools/bin/libnh_kref_score.so, against the fp64 log-softmax of the same fp16 operands within the bound tests/score_ref.py
derives.  The operands are followed by NaN rows (the rows M .. of xn, the rows V .. of E): a kernel that reads past either, or
lets a column >= V into a statistic, returns NaN."""
import functools

import numpy as np
import pytest

import score_ref as SR

pytestmark = pytest.mark.gpu

M_MAX = 300
# one valid row; a row guard either side of a tile; two row tiles plus a part tile
ROWS = [1, 127, 129, 300]
# a column tile with two valid columns; an exact multiple; the two real vocabularies
VOCABS = [130, 384, 51864, 51866]
WIDTHS = [128, 384]


@functools.lru_cache(maxsize=None)
def operands(d, V):
    """xn [M_MAX][d] and E [V][d] in fp16 (LayerNorm-sized rows, logits of a few units' spread), their guarded device images
    and the shared fp64 reference.  Row m of a case with M rows is row m here: a row's result does not depend on M."""
    rng = np.random.default_rng([d, V])
    xn = rng.standard_normal((M_MAX, d)).astype(np.float16)
    E = (0.25 * rng.standard_normal((V, d))).astype(np.float16)
    return xn, E, SR.guarded(E, 128), SR.Reference(xn, E)


def targets_for(M, V, seed):
    """columns 0, 127, 128, V - 1 and random ones, rotated by M so that a one-row case does not always take column 0"""
    rng = np.random.default_rng([M, V, seed])
    fixed = [0, 127, 128, V - 1]
    return np.array([fixed[(r + M) % 5] if (r + M) % 5 < 4 else int(rng.integers(0, V)) for r in range(M)], dtype=np.int32)


def check(out, ref, M, targets):
    assert np.isfinite(out).all(), np.flatnonzero(~np.isfinite(out))[:8]
    worst = 0.0
    for m in range(M):
        want, bound = ref.at(m, int(targets[m]))
        err = abs(float(out[m]) - want)
        worst = max(worst, err / bound)
        assert err <= bound, (m, int(targets[m]), float(out[m]), want, err, bound)
    return worst


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_rows_match_the_fp64_log_softmax(d, M, V):
    xn, E, E_img, ref = operands(d, V)
    x_img = SR.guarded(xn[:M], 256)   # rows M .. are NaN, up to and past the end of the last row tile
    t = targets_for(M, V, 0)
    out = SR.score_rows(x_img, M, d, E_img, V, t)
    worst = check(out, ref, M, t)
    print(f"d={d} M={M} V={V}: worst error / bound = {worst:.3f}")


def test_unscored_rows_are_left_alone():
    """target < 0: the merge writes nothing for the row"""
    d, V, M = 128, 130, 129
    xn, E, E_img, ref = operands(d, V)
    t = targets_for(M, V, 1)
    t[::3] = -1
    out = SR.score_rows(SR.guarded(xn[:M], 256), M, d, E_img, V, t, fill=7.25)
    assert (out[::3] == 7.25).all()
    keep = np.flatnonzero(t >= 0)
    for m in keep:
        want, bound = ref.at(int(m), int(t[m]))
        assert abs(float(out[m]) - want) <= bound


def test_a_target_120_below_the_maximum_stays_finite():
    """One row whose logits run from -60 to +60 with the target at the bottom: log p is about -120, where expf(l[t] - m)
    underflows and a log(expf(..) / se) form returns -inf."""
    d, V, M = 128, 384, 3
    rng = np.random.default_rng(60)
    xn = rng.standard_normal((M, d)).astype(np.float16)
    E = (0.25 * rng.standard_normal((V, d))).astype(np.float16)
    xn[1] = 0
    xn[1, 0] = 8.0
    E[:, 0] = np.linspace(-7.5, 7.5, V).astype(np.float16)   # row 1: l[v] = 8 E[v][0], -60 .. 60
    ref = SR.Reference(xn, E)
    t = np.array([5, 0, 383], dtype=np.int32)
    out = SR.score_rows(SR.guarded(xn, 256), M, d, SR.guarded(E, 128), V, t)
    want, bound = ref.at(1, 0)
    assert -121.5 < want < -119.5, want
    assert np.exp(np.float32(-120.0)) == 0.0   # f32 underflow: the other form takes log(0)
    check(out, ref, M, t)


def test_a_row_has_the_same_bits_whatever_the_rows_around_it():
    """300 rows at once, as three calls of 100, and cut into panels of 128: the same bits"""
    d, V = 128, 51866
    xn, E, E_img, _ = operands(d, V)
    t = targets_for(M_MAX, V, 2)
    whole = SR.score_rows(SR.guarded(xn, 256), M_MAX, d, E_img, V, t)
    parts = np.concatenate([SR.score_rows(SR.guarded(xn[a:a + 100], 256), 100, d, E_img, V, t[a:a + 100]) for a in (0, 100, 200)])
    assert whole.tobytes() == parts.tobytes()
    panels = SR.score_rows(SR.guarded(xn, 256), M_MAX, d, E_img, V, t, panel_rows=128)
    assert whole.tobytes() == panels.tobytes()


def test_the_partials_of_a_panel_stay_within_64_mb():
    L = SR.lib()
    for V in (1, 130, 51864, 51866, 65536):
        rows = L.kref_score_panel_rows(V)
        assert rows >= 128 and rows % 128 == 0
        assert rows * ((V + 127) // 128) * 8 <= 64 << 20
