"""CPU: token-level timestamps through the decode pool (norma_amd/pool.py, align_heads=...) against the scripted stand-in for
the engine (tests/pool_standin.py): the pool tells the engine the heads once, after pool_begin and before anything is admitted; it aligns exactly the
attempts it accepts -- never a rejected or a dropped one, never a no-speech exit --, while the row still holds the clip (before
anything is admitted into it or it is retried), with the clip's own n_keys; without the keyword it calls neither method.  The
GPU side is tests/test_gpu_align_live.py."""
import numpy as np
import pytest

from norma_amd import hip, pool
from pool_standin import BAD, GOOD, MUTE, Encoder, Engine, feeder
from test_pool_fallback_cpu import make_script

HEADS = [(1, 0), (0, 1)]


def _run(kind, N, script, rows, feed, check, n_keys, **kw):
    lengths = [3 + (5 * c) % 11 for c in range(N)]
    e = Engine(lengths, script, align="align_heads" in kw)
    if kind == "plain":
        p = pool.DecodePool(e, rows=rows, staging=feed, check_every=check, **kw)
        return e, p, p.run(N, e.encode, n_keys=n_keys)
    encs = [Encoder(), Encoder()]
    p = pool.FedDecodePool(e, encs, rows=rows, batch=feed, check_every=check, **kw)
    return e, p, p.run(N, feeder(encs), n_keys=n_keys)


@pytest.mark.parametrize("kind", ["plain", "fed"])
@pytest.mark.parametrize("rows,feed,check", [(4, 3, 2), (2, 5, 1), (8, 8, 16)])
def test_the_pool_aligns_exactly_the_accepted_attempts_before_the_row_is_used_again(kind, rows, feed, check):
    N = 40
    script, want = make_script(N, np.random.default_rng(rows))
    for c in range(5, N, 11):
        script[c], want[c] = [MUTE] * 6, (0, True)
    n_keys = [1500 - 7 * c for c in range(N)]
    e, p, res = _run(kind, N, script, rows, feed, check, n_keys, fallback=True, align_heads=HEADS)
    # the heads: once, right after pool_begin
    assert [x[0] for x in e.log[:2]] == ["begin", "capture"] and e.log[1][1] == tuple(HEADS)
    assert sum(1 for x in e.log if x[0] == "capture") == 1
    timed = 0
    for c, r in enumerate(res):
        attempt, accepted = want[c]
        assert (r["attempt"], r["accepted"]) == (attempt, accepted)
        if not accepted or script[c][0] == MUTE:
            assert "token_first" not in r and "token_last" not in r
            continue
        n = len(r["tokens"])
        assert len(r["token_first"]) == len(r["token_last"]) == n == 5
        assert r["token_first"] == [-1, -1, -1, c, attempt] and r["token_last"] == [-1, -1, -1, n_keys[c], 1000 + c]
        timed += 1
    assert timed == p.aligned and timed > N // 2
    # every aligned (clip, attempt) is an accepted one, once; and the row was touched by nothing between its collect and its align
    aligned = [(c, a) for x in e.log if x[0] == "align" for c, a in zip(x[2], x[3])]
    assert sorted(aligned) == sorted((c, want[c][0]) for c in range(N) if want[c][1] and script[c][0] != MUTE)
    for i, x in enumerate(e.log):
        if x[0] != "align":
            continue
        k = i - 1
        while e.log[k][0] == "retry":       # _settle of the other rows of the same collect
            assert e.log[k][2] not in x[1]
            k -= 1
        assert e.log[k][0] == "collect" and set(x[1]) <= set(e.log[k][1]), (e.log[k], x)


def test_without_fallback_every_clip_that_produced_tokens_is_timed_and_n_keys_may_be_left_out():
    N = 9
    script = [[GOOD] * 6, [BAD] * 6, [MUTE] * 6] * 3
    e, p, res = _run("plain", N, script, 3, 2, 2, None, align_heads=HEADS)
    for c, r in enumerate(res):
        if c % 3 == 2:
            assert "token_first" not in r
        else:
            assert r["token_first"][3:] == [c, 0] and r["token_last"][3] == -1
    assert all(x[4] is None for x in e.log if x[0] == "align")


def test_without_the_keyword_the_engine_is_never_asked():
    N = 12
    script, _ = make_script(N, np.random.default_rng(1))
    e, p, res = _run("plain", N, script, 3, 4, 2, None, fallback=True)
    assert not [x for x in e.log if x[0] in ("capture", "align")] and all("token_first" not in r for r in res)
    assert p.aligned == 0


def test_the_header_declares_both_functions():
    names = hip.declared_symbols()
    assert "nh_align_capture" in names and "nh_align_decoded" in names
