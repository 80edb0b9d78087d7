"""CPU: language detection in the decode pool's refill policy (norma_amd/pool.py, detect_languages=...) against a stand-in
engine of its own.  The stand-in keeps the C ABI's rules (include/norma_hip.h): the table goes in once after pool_begin and
while no row is busy; NH_LANG_DETECT needs the table; pool_languages answers only for rows admitted with NH_LANG_DETECT that
have stepped since and have not been refilled.  A clip's "audio" decides its language here too: clip c detects TABLE[c % 7].
The GPU side is tests/test_gpu_pool_detect.py."""
import numpy as np
import pytest

from norma_amd import pool
from norma_amd.hip import NH_LANG_DETECT

TABLE = list(range(50259, 50259 + 99))
GOOD, BAD = (-0.5, 0.1), (-2.0, 0.1)      # (avg_logprob, no_speech_prob): accepted / needs a fallback


def detected(c):
    return TABLE[c % 7]


def probs_of(c):
    p = np.full(len(TABLE), 0.25 / (len(TABLE) - 1), dtype=np.float32)
    p[c % 7] = 0.75
    return p


class DetectEngine:
    """A decode of clip c takes lengths[c] + attempt steps; pool_collect returns script[c][attempt] (default: accepted)."""

    def __init__(self, lengths, script=None, clip0=0):
        self.lengths, self.script, self.clip0 = lengths, script, clip0
        self.log = []
        self.table = None

    def pool_begin(self, rows, max_new, per_clip_language):
        self.rows, self.per_clip = rows, per_clip_language
        self.table = None                  # nh_pool_begin clears the table
        self.left = [None] * rows          # steps still to run per row (None: not busy)
        self.clip = [None] * rows
        self.attempt = [0] * rows
        self.lang = [None] * rows          # token in slot 1 of the row's prompt
        self.detect = [False] * rows       # admitted with NH_LANG_DETECT
        self.stepped = [False] * rows
        self.staged = {}
        self.log.append(("begin", rows, per_clip_language))

    def pool_detect_languages(self, lang_tokens):
        assert self.per_clip, "NH_ERR_INVALID: pool begun without per-clip languages"
        assert all(l is None for l in self.left), "NH_ERR_STATE: rows are busy"
        assert 1 <= len(lang_tokens) <= 256
        self.table = list(lang_tokens)
        self.log.append(("table", tuple(lang_tokens)))

    def encode(self, first, n, row0, must):
        assert row0 == self.rows
        self.staged = {row0 + i: first + i for i in range(n)}

    def _admit(self, c, dst, lang):
        assert self.left[dst] is None, "admit into a busy row"
        if lang == NH_LANG_DETECT:
            assert self.per_clip and self.table is not None, "NH_LANG_DETECT without a table"
        else:
            assert lang >= 0 or not self.per_clip
        self.clip[dst], self.left[dst], self.attempt[dst] = c, self.lengths[c], 0
        self.detect[dst], self.stepped[dst] = lang == NH_LANG_DETECT, False
        self.lang[dst] = None if lang == NH_LANG_DETECT else lang
        self.log.append(("admit", c, dst, lang))

    def pool_admit(self, src, dst, lang):
        assert src in self.staged
        self._admit(self.staged.pop(src), dst, lang)

    def pool_admit_from(self, enc, src, dst, lang):
        assert src in enc.rows
        self._admit(enc.rows.pop(src), dst, lang)

    def pool_retry(self, row, temperature, seed, clip, attempt):
        assert self.left[row] is None and self.clip[row] is not None, "retry of a busy or never admitted row"
        assert clip == self.clip0 + self.clip[row]
        assert self.lang[row] is not None, "the retried prompt must hold a language"
        self.left[row], self.attempt[row] = self.lengths[self.clip[row]] + attempt, attempt
        self.log.append(("retry", self.clip[row], row, attempt))

    def pool_step(self, n):
        flags = np.zeros(self.rows, dtype=np.int32)
        for r in range(self.rows):
            if self.left[r] is None:
                flags[r] = 3
                continue
            if n > 0:
                if self.detect[r] and not self.stepped[r] and self.attempt[r] == 0:
                    self.lang[r] = detected(self.clip[r])     # the row's first step writes its prompt's slot 1
                self.stepped[r] = True
            self.left[r] = max(0, self.left[r] - n)
            flags[r] = 1 if self.left[r] == 0 else 0
        self.log.append(("step", n))
        return flags

    def pool_languages(self, rows, want_probs=True):
        for r in rows:
            assert 0 <= r < self.rows, "NH_ERR_INVALID: row outside the pool"
            assert self.detect[r] and self.stepped[r], "NH_ERR_STATE: not a detected row that has stepped"
        self.log.append(("languages", tuple(rows)))
        toks = [self.lang[r] for r in rows]
        return toks, (np.stack([probs_of(self.clip[r]) for r in rows]) if want_probs else None)

    def pool_collect(self, rows):
        out = []
        for r in rows:
            assert self.left[r] == 0
            c, a = self.clip[r], self.attempt[r]
            lp, ns = self.script[c][a] if self.script else GOOD
            out.append(dict(clip=c, avg_logprob=lp, no_speech_prob=ns, tokens=[1, self.lang[r], 2, c, a]))
            self.left[r] = None
        self.log.append(("collect", tuple(rows)))
        return out


class FakeEncoder:
    def __init__(self):
        self.rows = {}


def run_pool(kind, e, N, rows, feed, check, langs="omit", **kw):
    lk = {} if langs == "omit" else {"langs": langs}
    if kind == "plain":
        p = pool.DecodePool(e, rows=rows, staging=feed, check_every=check, **kw)
        return p, p.run(N, e.encode, **lk)
    encs = [FakeEncoder(), FakeEncoder()]

    def encode(i, first, n):
        assert not encs[i].rows
        encs[i].rows = {k: first + k for k in range(n)}
    p = pool.FedDecodePool(e, encs, rows=rows, batch=feed, check_every=check, **kw)
    return p, p.run(N, encode, **lk)


def lengths_for(N, seed=3):
    return [int(v) for v in np.random.default_rng(seed).integers(3, 40, N)]


@pytest.mark.parametrize("kind", ["plain", "fed"])
@pytest.mark.parametrize("rows,feed,check", [(3, 4, 1), (5, 4, 16), (8, 3, 5)])
def test_every_clip_detects_when_no_languages_are_given(kind, rows, feed, check):
    N = 23
    e = DetectEngine(lengths_for(N))
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
    e = DetectEngine(lengths_for(N, 5))
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
    e = DetectEngine(lengths_for(N, 9), script, clip0=70)
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

    class Old(DetectEngine):
        def pool_detect_languages(self, *a):
            raise AssertionError("pool_detect_languages called")

        def pool_languages(self, *a, **k):
            raise AssertionError("pool_languages called")
    e = Old(lengths_for(N))
    p, got = run_pool(kind, e, N, 3, 4, 2)
    assert e.log[0] == ("begin", 3, False)
    assert all(l[3] == -1 for l in e.log if l[0] == "admit")
    assert all("language" not in g and "language_probs" not in g for g in got)
    e = Old(lengths_for(N))
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
