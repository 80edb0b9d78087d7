"""CPU: tests/score_ref.py itself -- the blocked fp64 reference against the direct formula, and its derived bound against
plausible kernel bugs on the data of tests/test_gpu_score_kernel.py: each must leave the bound by a factor of two on at least a
quarter of the rows, so that a kernel with that bug would fail the GPU cases."""
import numpy as np

import kref
import score_ref as SR


def data(d, V, M=40):
    rng = np.random.default_rng([d, V])
    return rng.standard_normal((M, d)).astype(np.float16), (0.25 * rng.standard_normal((V, d))).astype(np.float16)


def f32_device_model(x, E, t, drop_tile=None, pad_as_zero=0, shift=0):
    """the kernel's formula in fp64 with a planted mistake: a 128-column tile left out of the statistics, `pad_as_zero` columns
    past V counted with logit 0, the target read `shift` columns off"""
    l = x.astype(np.float64) @ E.astype(np.float64).T
    keep = np.ones(l.shape[1], dtype=bool)
    if drop_tile is not None:
        keep[128 * drop_tile:128 * drop_tile + 128] = False
    out = np.empty(len(x))
    for m in range(len(x)):
        v = np.concatenate([l[m, keep], np.zeros(pad_as_zero)])
        mx = v.max()
        out[m] = l[m, (t[m] + shift) % l.shape[1]] - mx - np.log(np.exp(v - mx).sum())
    return out


def test_reference_equals_the_direct_log_softmax():
    x, E = data(128, 384)
    ref = SR.Reference(x, E)
    t = np.arange(len(x)) * 7 % 384
    want = f32_device_model(x, E, t)
    for m in range(len(x)):
        got, bound = ref.at(m, int(t[m]))
        assert abs(got - want[m]) < 1e-12
        assert 0 < bound < 5e-3


def test_the_bound_catches_planted_mistakes_at_the_small_vocabularies():
    for d, V, bugs in ((128, 130, (dict(drop_tile=1), dict(pad_as_zero=126), dict(shift=1))),
                       (384, 384, (dict(drop_tile=2), dict(drop_tile=0), dict(shift=-1)))):
        x, E = data(d, V)
        ref = SR.Reference(x, E)
        t = np.arange(len(x)) * 5 % V
        for bug in bugs:
            wrong = f32_device_model(x, E, t, **bug)
            caught = sum(abs(wrong[m] - ref.at(m, int(t[m]))[0]) > 2 * ref.at(m, int(t[m]))[1] for m in range(len(x)))
            assert caught >= len(x) // 4, (d, V, bug, caught)   # one row out of bound fails a GPU case; they have 1 .. 300


def test_guarded_images_end_in_nan_rows():
    a = np.ones((3, 8), dtype=np.float16)
    g = SR.guarded(a, 2)
    assert g.shape == (5, 8) and g.dtype == np.uint16
    assert (g[:3].view(np.float16) == 1).all() and np.isnan(g[3:].view(np.float16)).all()
    assert kref.U32 == 2.0 ** -24
