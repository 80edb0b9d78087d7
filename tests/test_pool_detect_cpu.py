"""CPU: language detection in the decode pool's refill policy (norma_amd/pool.py, detect_languages=...) against the stand-in
engine of tests/pool_standin.py.  The stand-in keeps the C ABI's rules (include/norma_hip.h): the table goes in once after
pool_begin and while no row is busy; NH_LANG_DETECT needs the table; pool_languages answers only for rows admitted with NH_LANG_DETECT that
have stepped since and have not been refilled.  A clip's "audio" decides its language here too: clip c detects TABLE[c % 7].
The GPU side is tests/test_gpu_pool_detect.py."""
import numpy as np
import pytest

from norma_amd import pool
from norma_amd.hip import NH_LANG_DETECT
from pool_standin import BAD, GOOD, TABLE, Encoder, Engine, detected, feeder, probs_of


def run_pool(kind, e, N, rows, feed, check, langs="omit", **kw):
    lk = {} if langs == "omit" else {"langs": langs}
    if kind == "plain":
        p = pool.DecodePool(e, rows=rows, staging=feed, check_every=check, **kw)
        return p, p.run(N, e.encode, **lk)
    encs = [Encoder(), Encoder()]
    p = pool.FedDecodePool(e, encs, rows=rows, batch=feed, check_every=check, **kw)
    return p, p.run(N, feeder(encs), **lk)


def lengths_for(N, seed=3):
    return [int(v) for v in np.random.default_rng(seed).integers(3, 40, N)]


@pytest.mark.parametrize("kind", ["plain", "fed"])
@pytest.mark.parametrize("rows,feed,check", [(3, 4, 1), (5, 4, 16), (8, 3, 5)])
def test_every_clip_detects_when_no_languages_are_given(kind, rows, feed, check):
    N = 23
    e = Engine(lengths_for(N), detect=True)
    p, got = run_pool(kind, e, N, rows, feed, check, detect_languages=TABLE)
    # the table goes in exactly once, straight after pool_begin, and per-clip languages are implied
    assert e.log[0] == ("begin", rows, True) and e.log[1] == ("table", tuple(TABLE))
    assert sum(1 for l in e.log if l[0] in ("begin", "table")) == 2
    admits = [l for l in e.log if l[0] == "admit"]
    assert [a[1] for a in admits] == list(range(N)) and all(a[3] == NH_LANG_DETECT for a in admits)
    # results in clip order, each with its own language, its probabilities, and the token in its prompt
    assert [g["clip"] for g in got] == list(range(N))
    for c, g in enumerate(got):
        assert g["language"] == detected(c) == g["tokens"][1]
        assert np.array_equal(g["language_probs"], probs_of(c))
    # every detected clip was asked for once
    asked = [r for l in e.log if l[0] == "languages" for r in l[1]]
    assert len(asked) == N


@pytest.mark.parametrize("kind", ["plain", "fed"])
def test_given_and_detected_clips_mix_in_one_pool(kind):
    N = 17
    langs = [None if c % 3 != 1 else 51000 + c for c in range(N)]
    e = Engine(lengths_for(N, 5), detect=True)
    p, got = run_pool(kind, e, N, 4, 3, 4, langs=langs, detect_languages=TABLE, per_clip_language=False)
    admits = {l[1]: l[3] for l in e.log if l[0] == "admit"}
    for c in range(N):
        if langs[c] is None:                                  # NH_LANG_DETECT exactly where langs has no entry
            assert admits[c] == NH_LANG_DETECT
            assert got[c]["language"] == detected(c) and np.array_equal(got[c]["language_probs"], probs_of(c))
        else:
            assert admits[c] == langs[c]
            assert got[c]["language"] == langs[c] and "language_probs" not in got[c]
        assert got[c]["tokens"][1] == got[c]["language"]
    # pool_languages was read for detected rows only (the engine refuses any other), each once
    asked = sum(len(l[1]) for l in e.log if l[0] == "languages")
    assert asked == sum(1 for l in langs if l is None)


@pytest.mark.parametrize("kind", ["plain", "fed"])
def test_a_retried_clip_keeps_the_language_of_its_greedy_attempt(kind):
    N = 12
    script = [[BAD] * (c % 4) + [GOOD] * (6 - c % 4) for c in range(N)]          # accepted at attempt c % 4
    script[5] = [BAD] * 6                                                        # never: dropped after five retries
    e = Engine(lengths_for(N, 9), script, clip0=70, detect=True)
    p, got = run_pool(kind, e, N, 3, 4, 3, detect_languages=TABLE, fallback=True, seed=1, clip0=70)
    for c, g in enumerate(got):
        assert g["attempt"] == (5 if c == 5 else c % 4) and g["accepted"] == (c != 5)
        assert g["language"] == detected(c) == g["tokens"][1]
        assert np.array_equal(g["language_probs"], probs_of(c))
    assert p.retries == sum(g["attempt"] for g in got) > 0
    # the language is read once per clip, with the t = 0 attempt, never again for a retry
    assert sum(len(l[1]) for l in e.log if l[0] == "languages") == N


@pytest.mark.parametrize("kind", ["plain", "fed"])
def test_without_the_keyword_no_new_engine_method_is_touched(kind):
    N = 9
    e = Engine(lengths_for(N))          # without detect=True the stand-in has neither method
    assert not hasattr(e, "pool_detect_languages") and not hasattr(e, "pool_languages")
    p, got = run_pool(kind, e, N, 3, 4, 2)
    assert e.log[0] == ("begin", 3, False)
    assert all(l[3] == -1 for l in e.log if l[0] == "admit")
    assert all("language" not in g and "language_probs" not in g for g in got)
    e = Engine(lengths_for(N))
    langs = [50259 + c for c in range(N)]
    p, got = run_pool(kind, e, N, 3, 4, 2, langs=langs, per_clip_language=True)
    assert [l[3] for l in e.log if l[0] == "admit"] == langs and all("language" not in g for g in got)


def test_the_constant_matches_the_header():
    import re
    from norma_amd import hip
    with open(hip.HEADER_PATH) as f:
        m = re.search(r"#define\s+NH_LANG_DETECT\s+\((-?\d+)\)", f.read())
    assert m and int(m.group(1)) == hip.NH_LANG_DETECT == NH_LANG_DETECT == -2
    assert {"nh_pool_detect_languages", "nh_pool_languages"} <= set(hip.declared_symbols())
