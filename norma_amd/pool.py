"""Refill policy of the decode pool (include/norma_hip.h: nh_pool_*).

The reference's decode loop ends per sequence at eot (src/models/whisper/model.rs:317) and it decodes one stream at a time
(src/lib.rs:462-464); a batch decoded in lockstep makes the short sequences wait for the longest one.  The pool keeps a fixed
number of decode rows busy instead: the encoder is still fed `staging` clips at a time, every encoded clip is admitted to
whichever row is free, finished rows are collected every `check_every` steps.  The policy is engine-agnostic (it only calls
the methods below), so the CPU tests drive it with a counting stand-in and the GPU tests with HipWhisper.  Both pools are one
run loop (_Pool._run) over a source of encoded clips; run(.., on_result=f) calls f(clip, result) as soon as a result is final.

engine methods used: pool_begin(rows, max_new, per_clip_language), pool_admit(src_row, dst_row, lang),
pool_step(n) -> flags per row (0 running, 1 / 2 finished, 3 empty), pool_collect(rows) -> [result],
pool_retry(row, temperature, seed, clip, attempt) (only with fallback=True), pool_prefix(row, ids) (only with prefix=...),
pool_detect_languages(lang_tokens) and pool_languages(rows) -> (tokens, probs) (only with detect_languages=...),
and the caller's encode(first_clip, n_clips, row0, must) which must leave clips first .. first + n - 1 encoded in rows
row0 ... -- or, when `must` is false, may return False to say "the encoder is busy, ask again" (several pools share one GPU:
the pool then goes on decoding what it has instead of waiting for the encoder with its rows idle).

fallback=True adds decode_with_fallback (src/models/whisper/model.rs:164-191) per clip: an admitted clip is the t = 0 attempt;
a collected result that fails the test of model.rs:177-179 sends its row through pool_retry(row, temperature, seed, clip,
attempt) -- the same clip again, sampled at the next of `temperatures`, on the cross K/V the row still holds -- until a result
is accepted or the temperatures are used up (the reference returns None there: the clip is dropped, accepted=False).  The row
stays the clip's own meanwhile; the other rows go on being refilled.

detect_languages=<language tokens in Language::iter() order> adds the language step of decode_with_fallback (model.rs:170-173)
per clip: the table goes to pool_detect_languages(tokens) once after pool_begin (per-clip languages are implied), a clip
without an entry in `langs` is admitted with NH_LANG_DETECT and detects its language in its own first decode step, and
pool_languages(rows) -> (tokens, probs) is read when its t = 0 attempt is collected.  Every result then carries "language",
detected clips also "language_probs"; a retried clip keeps what its t = 0 attempt detected.  Without the keyword neither
engine method is called.

align_heads=[(decoder layer, head), ...] adds token-level timestamps ("Alignment from the decode"): the list goes
to align_capture(heads) once after pool_begin, so every row keeps those heads' cross-attention queries while it decodes, and
align_decoded(rows, n_keys) -> (first, last) is read right after the collect that yields a clip's accepted attempt -- under
fallback=True after _settle accepts, never for a rejected or dropped attempt -- and before the row is offered for admission.
The result gains "token_first" / "token_last": one encoder frame (20 ms) per entry of "tokens", -1 for the prompt.  A no-speech
exit gets none.  run(.., n_keys=[frames that hold audio per clip]) bounds each clip's alignment (None: all frames).  Without
the keyword neither engine method is called.

guard=<dict of set_guard's keywords> puts the repetition guard into the pool's steps: set_guard(**guard) once
after pool_begin.  bias=<callable clip -> {token: beta} | None> gives a clip its own logit bias (hotwords, per-clip
suppression): guard_bias(row, dict) right before the clip's admission, applied while guard has bias=True.  With a guard that
has a loop exit (loop_period > 0) every result carries "loop_exit", read with guard_report(rows) at the collect.
loop_fallback=True (with fallback=True) makes a result whose row took the exit fail the test of _settle whatever its
avg_logprob -- the counterpart of the reference's dead `compression_ratio > threshold` half -- still subject to the
no_speech_prob clause.  Without these keywords none of the three engine methods is called.  Like the alignment heads and the
language table, the guard and the rows' bias lists stay set on the engine after run(): a caller that goes on to use the
context otherwise switches them off itself (set_guard(None), guard_bias(row, None)).

prefix=<callable (clip, prev) -> token ids | None> gives a clip its own decoder prompt prefix ("Pool rows"; the
engine's nh_pool_prefix): asked right before the clip's admission, after its bias; a non-empty answer goes to
pool_prefix(row, ids), and the clip's result is the sequence from sot on, as under set_prompts.  Every row has its own
length; the engine consumes the prefixes of the rows admitted between two steps in one ragged pass.  A clip that has a prefix
cannot detect its language (the engine refuses NH_LANG_DETECT into such a row): give it one in `langs`.  prefix together with
align_heads is a ValueError: nh_align_decoded does not cover prompted decodes.
after=<callable clip -> earlier clip index | None> orders clips that depend on one another -- the chunks of one recording, each
decoded under the text of the chunk before it, among many recordings in flight: clip c is admitted only once that clip's
result is final (under fallback=True: once _settle accepted or dropped it), and `prev` of the prefix callable is that result
(None without `after`, or where it answers None).  Admission stays in clip order: the pool holds c and everything behind it
meanwhile, which cannot deadlock, since the predecessor was admitted earlier.  An index >= clip is a ValueError.
condition_on_previous(startofprev, eot) below is the prefix callable of host.Model's history rule.  Without the two keywords
neither callable exists and pool_prefix is never called.
"""
import queue
import threading
from typing import Callable, List, Optional, Sequence

from .hip import NH_LANG_DETECT

TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)   # m::TEMPERATURES of model.rs:175 (LOGPROB_THRESHOLD -1, NO_SPEECH_THRESHOLD 0.6)


def condition_on_previous(startofprev: int, eot: int, max_prefix: int = 223):
    """The `prefix` callable that conditions a clip on the text of the clip `after` names: [startofprev] + the text ids (< eot)
    of prev["tokens"] behind its prompt, cut to the last max_prefix - 1 (223 = max_target_positions / 2 - 1 of every Whisper).
    None -- no prefix -- without a prev, and when prev was a no-speech exit, was not accepted, was accepted above t = 0.5 (what
    it says is not to be trusted as context: host.Model's history rule, DESIGN.md 13 "Layers above"), or holds no text."""
    assert max_prefix >= 2

    def prefix(clip: int, prev: Optional[dict]):
        if prev is None or prev.get("no_speech_exit") or not prev.get("accepted", True) or prev.get("temperature", 0.0) > 0.5:
            return None
        toks = list(prev["tokens"])
        p = 0
        while p < len(toks) and toks[p] > eot:   # [sot, lang?, task]: the special ids above eot that open every result
            p += 1
        text = [int(t) for t in toks[p:] if t < eot]
        return [int(startofprev)] + text[-(max_prefix - 1):] if text else None
    return prefix


def _has_loop_exit(guard: Optional[dict]) -> bool:
    """a guard with a loop exit (loop_period > 0) has something for guard_report to say"""
    return guard is not None and int(guard.get("loop_period", 0)) > 0


class _Pool:
    """what both pools are: the per-row policy on a collected result, and the one run loop over a source of encoded clips"""

    def __init__(self, engine, rows, max_new_tokens, check_every, per_clip_language, fallback, seed, clip0, temperatures,
                 logprob_threshold, no_speech_threshold, detect_languages, align_heads, guard, bias, loop_fallback,
                 prefix=None, after=None):
        assert rows >= 1 and check_every >= 1
        if prefix is not None and align_heads is not None:
            raise ValueError("align_heads with prefix: nh_align_decoded does not cover prompted decodes")
        self.prefix_of, self.after_of = prefix, after
        self.e, self.rows, self.check_every = engine, rows, check_every
        self.max_new, self.per_clip_language = max_new_tokens, per_clip_language
        self.fallback, self.seed, self.clip0 = bool(fallback), int(seed), int(clip0)
        self.temperatures = tuple(float(t) for t in temperatures)
        assert len(self.temperatures) >= 1 and self.temperatures[0] == 0.0 and all(t > 0.0 for t in self.temperatures[1:]), \
            "temperatures: 0 first (an admitted row is greedy), then the sampled retries"
        self.logprob_threshold, self.no_speech_threshold = float(logprob_threshold), float(no_speech_threshold)
        self.detect_languages = None if detect_languages is None else [int(t) for t in detect_languages]
        if self.detect_languages is not None:
            self.per_clip_language = True
        self.align_heads = None if align_heads is None else [(int(l), int(h)) for l, h in align_heads]
        self.guard = None if guard is None else dict(guard)
        self.bias_of, self.loop_fallback = bias, bool(loop_fallback)
        self._report = _has_loop_exit(self.guard)
        self.steps = 0          # decode steps launched
        self.row_steps = 0      # sum over steps of the rows that were busy (what the step kernels' per-row work scales with)
        self.encodes = 0
        self.retries = 0        # pool_retry calls
        self.aligned = 0        # clips aligned

    def _begin(self):
        self.e.pool_begin(self.rows, self.max_new, self.per_clip_language)
        if self.guard is not None:
            self.e.set_guard(**self.guard)           # the fresh pool has no busy row
        if self.align_heads is not None:
            self.e.align_capture(self.align_heads)   # the fresh pool has no busy row: the steps are captured with the list
        if self.detect_languages is not None:
            self.e.pool_detect_languages(self.detect_languages)
        self._lang = [None] * self.rows     # per row: (language token, probabilities or None) of the clip it holds

    def _admit_lang(self, row: int, clip: int, langs) -> int:
        """the `lang` a clip is admitted with"""
        given = None if langs is None else langs[clip]
        if self.detect_languages is None:
            return -1 if given is None else int(given)
        self._lang[row] = None if given is None else (int(given), None)
        return NH_LANG_DETECT if given is None else int(given)

    def _collect(self, fin: List[int], attempt: List[int]) -> List[dict]:
        """pool_collect, plus the languages: detected ones are read once, with the t = 0 attempt (those rows have stepped)"""
        out = self.e.pool_collect(fin)
        if self._report:
            for res, flag in zip(out, self.e.guard_report(fin)):
                res["loop_exit"] = bool(flag)
        if self.detect_languages is not None:
            det = [r for r in fin if self._lang[r] is None]
            if det:
                assert all(attempt[r] == 0 for r in det)
                toks, probs = self.e.pool_languages(det)
                for i, r in enumerate(det):
                    self._lang[r] = (int(toks[i]), probs[i])
            for r, res in zip(fin, out):
                res["language"] = self._lang[r][0]
                if self._lang[r][1] is not None:
                    res["language_probs"] = self._lang[r][1]
        return out

    def _settle(self, row: int, clip: int, res: dict, attempt: int) -> bool:
        """True: `res` is the clip's result (accepted, or dropped after the last temperature) and the row is free.
        False: the row decodes the clip again at the next temperature."""
        res["attempt"], res["temperature"], res["accepted"] = attempt, self.temperatures[attempt], True
        if not self.fallback:
            return True
        # model.rs:177-179; compression_ratio is NaN there (:383), so `compression_ratio > threshold` never holds
        # ... and has this counterpart: a row that took the guard's loop exit (loop_fallback)
        needs = res["avg_logprob"] < self.logprob_threshold or (self.loop_fallback and bool(res.get("loop_exit")))
        if not needs or res["no_speech_prob"] > self.no_speech_threshold:
            return True
        if attempt + 1 >= len(self.temperatures):
            res["accepted"] = False     # model.rs:190: None -- the numbers are the last attempt's
            return True
        self.e.pool_retry(row, self.temperatures[attempt + 1], self.seed, self.clip0 + clip, attempt + 1)
        self.retries += 1
        return False

    def _align(self, settled, n_keys):
        """settled: [(row, clip, result)] of this collect whose rows are about to be freed; the accepted ones that produced
        tokens are aligned in one call, on the state their rows still hold"""
        if self.align_heads is None:
            return
        todo = [(r, c, res) for r, c, res in settled if res["accepted"] and not res["no_speech_exit"]]
        if not todo:
            return
        nk = None if n_keys is None else [int(n_keys[c]) for _, c, _ in todo]
        first, last = self.e.align_decoded([r for r, _, _ in todo], n_keys=nk)
        for i, (_, _, res) in enumerate(todo):
            n = len(res["tokens"])
            res["token_first"], res["token_last"] = [int(v) for v in first[i][:n]], [int(v) for v in last[i][:n]]
        self.aligned += len(todo)

    def _run(self, n_clips: int, src, langs, on_result, n_keys) -> List[dict]:
        """Decode clips 0 .. n_clips - 1 as `src` has them encoded; returns their results in clip order.  src.ready(clip, wait):
        is the next clip to admit encoded?  Asked once per pass; wait: no row is busy, there is nothing to decode meanwhile.
        src.admit(clip, row, lang): move it into the row; is the clip after it encoded as well?"""
        e, R = self.e, self.rows
        self._begin()
        results: List[Optional[dict]] = [None] * n_clips
        owner = [-1] * R                  # clip decoding in each row
        attempt = [0] * R                 # index into temperatures of the decode that row is on
        clip = busy = done = 0            # next clip to admit, rows decoding, clips with a result
        while done < n_clips:
            more = clip < n_clips and src.ready(clip, busy == 0)
            for r in range(R):            # admit in clip order into the lowest free rows
                if not more:
                    break
                if owner[r] < 0:
                    prev = None
                    if self.after_of is not None:
                        p = self.after_of(clip)
                        if p is not None:
                            if not 0 <= p < clip:
                                raise ValueError(f"after({clip}) = {p}: a clip can only follow an earlier clip")
                            prev = results[p]
                            if prev is None:       # its predecessor decodes still (or is on a retry): hold this clip and all behind it
                                break
                    if self.bias_of is not None:   # the clip's bias list goes to its row first (None or {}: the row's list is cleared)
                        e.guard_bias(r, self.bias_of(clip))
                    if self.prefix_of is not None:
                        ids = self.prefix_of(clip, prev)
                        if ids is not None and len(ids):
                            e.pool_prefix(r, [int(t) for t in ids])
                    more = src.admit(clip, r, self._admit_lang(r, clip, langs)) and clip + 1 < n_clips
                    owner[r], attempt[r] = clip, 0
                    clip += 1
                    busy += 1
            if busy == 0:
                continue
            flags = e.pool_step(self.check_every)
            self.steps += self.check_every
            self.row_steps += busy * self.check_every
            fin = [r for r in range(R) if owner[r] >= 0 and flags[r] in (1, 2)]
            if fin:
                settled = []
                for r, res in zip(fin, self._collect(fin, attempt)):
                    if not self._settle(r, owner[r], res, attempt[r]):
                        attempt[r] += 1   # the row is busy again with the same clip
                        continue
                    settled.append((r, owner[r], res))
                self._align(settled, n_keys)   # while the rows still hold their clips
                for r, c, res in settled:
                    results[c] = res
                    if on_result:
                        on_result(c, res)
                    owner[r] = -1
                    busy -= 1
                    done += 1
        return results  # type: ignore[return-value]


class _Staged:
    """DecodePool's clips: encoded `staging` at a time into the staging rows R .. of the pool's own context, whenever those are
    empty; clip c sits in staging row R + (c - first)"""

    def __init__(self, pool, n_clips: int, encode):
        self.p, self.n_clips, self.encode = pool, n_clips, encode
        self.first = self.end = 0         # clips first .. end - 1 are or were staged; those from the next to admit on still are

    def ready(self, clip: int, wait: bool) -> bool:
        if clip == self.end:
            n = min(self.p.staging, self.n_clips - clip)
            if self.encode(clip, n, self.p.rows, wait) is not False:   # False: the encoder is busy, ask again after a step
                self.p.encodes += 1
                self.first, self.end = clip, clip + n
        return clip < self.end

    def admit(self, clip: int, row: int, lang: int) -> bool:
        self.p.e.pool_admit(self.p.rows + (clip - self.first), row, lang)
        return clip + 1 < self.end


class DecodePool(_Pool):
    def __init__(self, engine, rows: int = 64, staging: int = 32, max_new_tokens: int = 0, check_every: int = 16,
                 per_clip_language: bool = False, fallback: bool = False, seed: int = 0, clip0: int = 0,
                 temperatures: Sequence[float] = TEMPERATURES, logprob_threshold: float = -1.0, no_speech_threshold: float = 0.6,
                 detect_languages: Optional[Sequence[int]] = None, align_heads: Optional[Sequence] = None,
                 guard: Optional[dict] = None, bias: Optional[Callable[[int], Optional[dict]]] = None, loop_fallback: bool = False,
                 prefix: Optional[Callable[[int, Optional[dict]], Optional[Sequence[int]]]] = None,
                 after: Optional[Callable[[int], Optional[int]]] = None):
        assert staging >= 1
        super().__init__(engine, rows, max_new_tokens, check_every, per_clip_language, fallback, seed, clip0, temperatures,
                         logprob_threshold, no_speech_threshold, detect_languages, align_heads, guard, bias, loop_fallback,
                         prefix=prefix, after=after)
        self.staging = staging

    def run(self, n_clips: int, encode: Callable[[int, int, int, bool], Optional[bool]], langs: Optional[Sequence[Optional[int]]] = None,
            on_result: Optional[Callable[[int, dict], None]] = None, n_keys: Optional[Sequence[int]] = None) -> List[dict]:
        """Decode clips 0 .. n_clips - 1; returns their results in clip order."""
        return self._run(n_clips, _Staged(self, n_clips, encode), langs, on_result, n_keys)


class _Fed:
    """FedDecodePool's clips: an encoder thread submits them `batch` at a time to the encoder contexts in turn and queues what
    it has encoded; a context is handed back to it only when every clip of its submission has been moved"""

    def __init__(self, pool, n_clips: int, encode):
        self.p = pool
        self.queue: "queue.Queue" = queue.Queue()      # (encoder index, first clip, n) in submission order; None: see errs
        self.free = [threading.Semaphore(1) for _ in pool.encoders]   # encoder context not holding un-admitted clips
        self.stop = threading.Event()                  # the calling thread is done, whether or not every clip was encoded
        self.errs: List[BaseException] = []
        self.cur = None                                # the submission being admitted
        self.thread = threading.Thread(target=self._feed, args=(n_clips, encode))
        self.thread.start()

    def _feed(self, n_clips: int, encode):
        try:
            for k, first in enumerate(range(0, n_clips, self.p.batch)):
                i = k % len(self.free)
                self.free[i].acquire()
                if self.stop.is_set():
                    break
                n = min(self.p.batch, n_clips - first)
                encode(i, first, n)
                self.p.encodes += 1
                self.queue.put((i, first, n))
        except BaseException as ex:   # noqa: BLE001 -- re-raised on the calling thread, which may be waiting for a submission
            self.errs.append(ex)
            self.queue.put(None)

    def ready(self, clip: int, wait: bool) -> bool:
        if self.cur is None:
            try:
                self.cur = self.queue.get(block=wait)
            except queue.Empty:
                return False
            if self.cur is None:
                raise self.errs[0]
        return True

    def admit(self, clip: int, row: int, lang: int) -> bool:
        i, first, n = self.cur
        self.p.e.pool_admit_from(self.p.encoders[i], clip - first, row, lang)
        if clip + 1 == first + n:
            self.free[i].release()        # every clip of that submission has been moved: the context may encode again
            self.cur = None
        return clip + 1 < first + n or self.ready(clip + 1, False)

    def close(self):
        self.stop.set()
        for s_ in self.free:              # a thread that waits for a context wakes up, sees the flag and ends
            s_.release()
        self.thread.join()


class FedDecodePool(_Pool):
    """One decoding context fed by encoder contexts of the same weight set (nh_pool_admit_from): the pool never stalls for an
    encoder submission -- its stream only ever runs decode steps and the device-to-device moves of admitted clips -- while an
    encoder thread keeps the encoder contexts busy one after the other.  `encode(e, first_clip, n)` must leave clips first ..
    first + n - 1 encoded in rows 0 .. n - 1 of encoder context e (called on the encoder thread; an encoder context is handed
    out again only when every clip of its previous submission has been admitted).  When run() raises, whether the error is the
    engine's or `encode`'s, the encoder thread has ended."""

    def __init__(self, engine, encoders: Sequence, rows: int = 64, batch: int = 32, max_new_tokens: int = 0, check_every: int = 16,
                 per_clip_language: bool = False, fallback: bool = False, seed: int = 0, clip0: int = 0,
                 temperatures: Sequence[float] = TEMPERATURES, logprob_threshold: float = -1.0, no_speech_threshold: float = 0.6,
                 detect_languages: Optional[Sequence[int]] = None, align_heads: Optional[Sequence] = None,
                 guard: Optional[dict] = None, bias: Optional[Callable[[int], Optional[dict]]] = None, loop_fallback: bool = False,
                 prefix: Optional[Callable[[int, Optional[dict]], Optional[Sequence[int]]]] = None,
                 after: Optional[Callable[[int], Optional[int]]] = None):
        assert batch >= 1 and len(encoders) >= 1
        super().__init__(engine, rows, max_new_tokens, check_every, per_clip_language, fallback, seed, clip0, temperatures,
                         logprob_threshold, no_speech_threshold, detect_languages, align_heads, guard, bias, loop_fallback,
                         prefix=prefix, after=after)
        self.encoders, self.batch = list(encoders), batch

    def run(self, n_clips: int, encode: Callable[[int, int, int], None], langs: Optional[Sequence[Optional[int]]] = None,
            n_keys: Optional[Sequence[int]] = None, on_result: Optional[Callable[[int, dict], None]] = None) -> List[dict]:
        src = _Fed(self, n_clips, encode)
        try:
            return self._run(n_clips, src, langs, on_result, n_keys)
        finally:
            src.close()
