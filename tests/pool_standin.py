"""The stand-in engine of the CPU pool tests (test_pool_cpu, test_pool_fallback_cpu, test_pool_detect_cpu, test_pool_align_cpu,
test_guard_cpu, test_pool_trace_cpu): the engine methods norma_amd/pool.py calls, scripted and logged, with the rules of the C
ABI (include/norma_hip.h) as assertions -- no admit into a busy row, no retry of a running one, the language table once and on
an idle pool, pool_languages only for detected rows that have stepped.  Clip c decodes for lengths[c] + attempt steps and
collects as script[c][attempt] = (avg_logprob, no_speech_prob) (no script: GOOD); its "audio" decides its language: TABLE[c % 7].

e.log, one tuple per call: ("begin", rows, per_clip_language), ("encode", first, n), ("admit", clip, row, lang),
("retry", clip, row, temperature, seed, clip id, attempt), ("step", n), ("collect", rows), and of the optional methods
("table", tokens), ("languages", rows), ("capture", heads), ("align", rows, clips, attempts, n_keys), ("set_guard", keywords),
("guard_bias", row, bias), ("guard_report", rows)."""
import numpy as np

from norma_amd.hip import NH_LANG_DETECT

GOOD, BAD = (-0.5, 0.1), (-2.0, 0.1)      # (avg_logprob, no_speech_prob): accepted / needs a fallback
SILENT = (-2.0, 0.9)                      # needs a fallback by its log-prob, accepted all the same: no_speech_prob > 0.6
MUTE = (-2.0, 0.99)                       # the no-speech exit: accepted at attempt 0, nothing to align
TABLE = list(range(50259, 50259 + 99))
N_POS = 12


def detected(c):
    return TABLE[c % 7]


def probs_of(c):
    p = np.full(len(TABLE), 0.25 / (len(TABLE) - 1), dtype=np.float32)
    p[c % 7] = 0.75
    return p


class Engine:
    """detect, align, guard: the engine has pool_detect_languages / pool_languages, align_capture / align_decoded, set_guard /
    guard_bias / guard_report only when switched on -- a pool that touches one it was not asked to use fails on the attribute.
    loops, always: clips whose row takes the guard's loop exit at attempt 0 / at every attempt.
    busy_every = k: encode answers "busy" (False) unless it must, except at every k-th time it is asked.
    fail = (method, k): the k-th call of that method raises self.error."""

    def __init__(self, lengths, script=None, clip0=0, detect=False, align=False, guard=False, loops=(), always=(), fail=None):
        self.lengths, self.script, self.clip0 = lengths, script, clip0
        self.loops, self.always, self.fail = set(loops), set(always), fail
        self.with_detect, self.with_align = detect, align
        self.log, self.busy_every, self.asked, self.calls = [], 0, 0, 0
        self.error = RuntimeError("the stand-in engine failed")
        if detect:
            self.pool_detect_languages, self.pool_languages = self._table, self._languages
        if align:
            self.align_capture, self.align_decoded = self._capture, self._align
        if guard:
            self.set_guard, self.guard_bias, self.guard_report = self._set_guard, self._bias, self._report

    def _called(self, name):
        if self.fail and self.fail[0] == name:
            self.calls += 1
            if self.calls == self.fail[1]:
                raise self.error

    def pool_begin(self, rows, max_new, per_clip_language):
        self.rows, self.per_clip = rows, per_clip_language
        self.table = None                  # nh_pool_begin clears the table
        self.left = [None] * rows          # steps still to run per row (None: not busy)
        self.clip = [None] * rows          # the clip whose cross K/V the row holds
        self.attempt = [0] * rows
        self.lang = [None] * rows          # token in slot 1 of the row's prompt
        self.detect = [False] * rows       # admitted with NH_LANG_DETECT
        self.stepped = [False] * rows
        self.staged = {}
        self.max_concurrent = 0
        self.log.append(("begin", rows, per_clip_language))

    def encode(self, first, n, row0, must):
        assert row0 == self.rows
        self.asked += 1
        if self.busy_every and not must and self.asked % self.busy_every:
            return False                   # "the encoder is busy": the pool must go on decoding and ask again
        self.staged = {row0 + i: first + i for i in range(n)}
        self.log.append(("encode", first, n))

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
        self.log.append(("retry", self.clip[row], row, temperature, seed, clip, attempt))

    def pool_step(self, n):
        self._called("pool_step")
        self.max_concurrent = max(self.max_concurrent, sum(l is not None for l in self.left))
        flags = np.zeros(self.rows, dtype=np.int32)
        for r in range(self.rows):
            if self.left[r] is None:
                flags[r] = 3
                continue
            if self.detect[r] and not self.stepped[r] and self.attempt[r] == 0:
                self.lang[r] = detected(self.clip[r])     # the row's first step writes its prompt's slot 1
            self.stepped[r] = True
            self.left[r] = max(0, self.left[r] - n)
            flags[r] = 1 if self.left[r] == 0 else 0
        self.log.append(("step", n))
        return flags

    def pool_collect(self, rows):
        self._called("pool_collect")
        out = []
        for r in rows:
            assert self.left[r] == 0
            c, a = self.clip[r], self.attempt[r]
            lp, ns = self.script[c][a] if self.script else GOOD
            mute = ns > 0.95 and a == 0
            if self.with_align:
                tokens = [7, 8, 9] + ([] if mute else [100 + c, 200 + a])
            else:
                tokens = [1, self.lang[r], 2, c, a] if self.with_detect else [c, a]
            out.append(dict(clip=c, lang=self.lang[r], avg_logprob=lp, no_speech_prob=ns, no_speech_exit=mute, tokens=tokens))
            self.left[r] = None
        self.log.append(("collect", tuple(rows)))
        return out

    # ---- only with detect=True
    def _table(self, lang_tokens):
        assert self.per_clip, "NH_ERR_INVALID: pool begun without per-clip languages"
        assert all(l is None for l in self.left), "NH_ERR_STATE: rows are busy"
        assert 1 <= len(lang_tokens) <= 256
        self.table = list(lang_tokens)
        self.log.append(("table", tuple(lang_tokens)))

    def _languages(self, rows, want_probs=True):
        for r in rows:
            assert 0 <= r < self.rows, "NH_ERR_INVALID: row outside the pool"
            assert self.detect[r] and self.stepped[r], "NH_ERR_STATE: not a detected row that has stepped"
        self.log.append(("languages", tuple(rows)))
        toks = [self.lang[r] for r in rows]
        return toks, (np.stack([probs_of(self.clip[r]) for r in rows]) if want_probs else None)

    # ---- only with align=True: align_decoded answers with numbers made of (clip, attempt, n_keys), so a result shows which
    # decode it was aligned on
    def _capture(self, heads):
        assert all(l is None for l in self.left), "heads set while a row is busy"
        self.log.append(("capture", tuple(heads)))

    def _align(self, rows, n_keys=None):
        first = np.full((len(rows), N_POS), -1, dtype=np.int32)
        last = np.full((len(rows), N_POS), -1, dtype=np.int32)
        for i, r in enumerate(rows):
            assert self.left[r] is None and self.clip[r] is not None, "aligned a busy or an empty row"
            nk = -1 if n_keys is None else n_keys[i]
            first[i, 3:5] = [self.clip[r], self.attempt[r]]
            last[i, 3:5] = [nk, 1000 + self.clip[r]]
        self.log.append(("align", tuple(rows), tuple(self.clip[r] for r in rows), tuple(self.attempt[r] for r in rows),
                         None if n_keys is None else tuple(n_keys)))
        return first, last

    # ---- only with guard=True
    def _set_guard(self, **kw):
        assert all(l is None for l in self.left), "guard set while a row is busy"
        self.log.append(("set_guard", kw))

    def _bias(self, row, bias):
        assert self.left[row] is None
        self.log.append(("guard_bias", row, bias))

    def _report(self, rows):
        self.log.append(("guard_report", tuple(rows)))
        return [int(self.clip[r] in self.always or (self.clip[r] in self.loops and self.attempt[r] == 0)) for r in rows]


class Encoder:
    """an encoder context of the fed pool: the clips it holds, by row"""

    def __init__(self):
        self.rows = {}


def feeder(encs, submissions=None):
    """the fed pool's encode(i, first, n) over `encs`: a context is handed out again only when every clip of its last
    submission was admitted"""
    def encode(i, first, n):
        assert not encs[i].rows
        encs[i].rows = {k: first + k for k in range(n)}
        if submissions is not None:
            submissions.append((i, first, n))
    return encode
