"""One call for a whole recording: plan the cuts on the device (HipWhisper.cut_plan: the quietest frame near the end of every
clip of at most 30 s), run the chunks through log-mel, encoder and greedy decode in groups, and join the chunks' segments on
one time axis.  The contract of the cuts is in include/norma_hip.h and DESIGN.md 11.  transcribe_speech / stitch_speech are the
same call on the recording's speech alone (HipWhisper.vad_plan): a chunk is then a concatenation of pieces of the
recording, and to_recording maps a time inside a chunk back to the recording's own axis.

The reference walks a recording sequentially and re-seeks to its last timestamp (`model.rs:100-146`); here the chunks are
independent, which is what lets them be batched.  `stitch` delimits segments the way `model.rs:100-105` does.
"""
from typing import List, Sequence, Tuple

import numpy as np

from .pool import _has_loop_exit

SAMPLE_RATE = 16000
KEY_SAMPLES = 320      # samples per encoder frame (20 ms): one timestamp unit
MIN_MEL_SAMPLES = 160  # a shorter clip produces 1500 mel frames, not 3000, and cannot share a batch with longer ones


def _groups(lens: Sequence[int], max_batch: int) -> List[Tuple[int, int]]:
    """[first, last) of consecutive chunks submitted together: at most max_batch, and a chunk of fewer than 160 samples
    (only the final one can be) alone"""
    out, a, n = [], 0, len(lens)
    while a < n:
        b = a + 1
        if lens[a] >= MIN_MEL_SAMPLES:
            while b < n and b - a < max_batch and lens[b] >= MIN_MEL_SAMPLES:
                b += 1
        out.append((a, b))
        a = b
    return out


def _beam_rows(hm, beam_size: int, align: bool) -> int:
    """chunks per group: a beam of K spreads every chunk over K rows of the context (HipWhisper.decode_beam); 1: the greedy decode"""
    if beam_size < 1 or beam_size > hm.max_batch:
        raise ValueError(f"beam_size must lie in 1 .. max_batch ({hm.max_batch})")
    if beam_size > 1 and align:
        raise ValueError("align=True does not cover beam decodes (align_decoded refuses after one)")
    return hm.max_batch // beam_size


def _set_prompt(hm, prompt, n: int, align: bool):
    """one id list in front of every chunk of the group just encoded (HipWhisper.set_prompts; a new batch starts without one)"""
    if prompt is not None and len(prompt):
        if align:
            raise ValueError("align=True does not cover prompted decodes (align_decoded refuses after one)")
        hm.set_prompts([list(prompt)] * n)


class _Guard:
    """guard=<HipWhisper.set_guard's keywords> and bias=<{token: beta}, the same for every chunk> around the decodes of one call
    (DESIGN.md 16): set on entry, switched off and cleared on exit -- the call owns the context's guard and the bias lists of
    rows 0 .. rows-1 meanwhile, and what the caller had set there before is gone after it.  Neither given: no engine method is
    called and the context's own guard, if any, applies.  With a loop
    exit in the guard every result of a greedy decode carries "loop_exit" (after a beam decode guard_report refuses)."""

    def __init__(self, hm, guard, bias, rows: int, beam_size: int):
        self.hm, self.guard, self.bias, self.rows = hm, (None if guard is None else dict(guard)), bias, rows
        self.report = _has_loop_exit(self.guard) and beam_size == 1

    def __enter__(self):
        if self.guard is not None:
            self.hm.set_guard(**self.guard)
        if self.bias:
            for r in range(self.rows):
                self.hm.guard_bias(r, self.bias)
        return self

    def __exit__(self, *exc):
        if self.bias:
            for r in range(self.rows):
                self.hm.guard_bias(r, None)
        if self.guard is not None:
            self.hm.set_guard(None)
        return False

    def mark(self, res):
        if self.report:
            for r, flag in zip(res, self.hm.guard_report()):
                r["loop_exit"] = bool(flag)


def _score(hm, res, prompt) -> List[np.ndarray]:
    """hm.score on the sequences a group's decode returned: per clip f32 [len(tokens)], entry i = ln p(tokens[i]), 0.0 for the
    [sot, language?, task] prompt.  A prefix the decode ran under goes in front of them, as nh_score asks.  A clip that
    generated nothing (the no-speech exit returns the bare prompt) has nothing to score: it goes in with eot appended, which
    nh_score needs to accept the batch, and reports zeros."""
    pre = list(prompt) if prompt is not None and len(prompt) else []
    P = 2 if res[0]["tokens"][1] == hm._task else 3
    seqs = [pre + list(r["tokens"]) + ([hm._eot] if len(r["tokens"]) <= P else []) for r in res]
    lp = hm.score(seqs, prompt_len=len(pre) + P)
    out = []
    for i, r in enumerate(res):
        n = len(r["tokens"])
        out.append(lp[i, len(pre):len(pre) + n].copy() if n > P else np.zeros(n, dtype=np.float32))
    return out


def _pcm(pcm):
    """a host f32 array (16 kHz mono) or (device pointer, n_samples), as the plan and log-mel calls take it: (rec, n)"""
    if isinstance(pcm, np.ndarray):
        return np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1), None
    return int(pcm[0]), int(pcm[1])


def _transcribe(hm, totals, fill, annotate, max_new_tokens, align, prompt, beam_size, score, guard, bias) -> List[dict]:
    """A planned recording through log-mel, encoder and decode, a group of chunks at a time.  totals: samples per chunk;
    fill(a, b) puts the log-mel of chunks a .. b-1 into rows 0 ..; annotate(i, result) adds the plan's own fields of chunk i,
    which come after token_logprob and before n_samples, n_keys and token_first / token_last."""
    out = []
    rows = _beam_rows(hm, beam_size, align)
    with _Guard(hm, guard, bias, rows, beam_size) as gd:
        for a, b in _groups(totals, rows):
            fill(a, b)
            hm.encode()
            _set_prompt(hm, prompt, b - a, align)
            res = hm.decode_greedy(max_new_tokens) if beam_size == 1 else hm.decode_beam(beam_size, max_new_tokens)
            gd.mark(res)
            keys = [-(-int(v) // KEY_SAMPLES) for v in totals[a:b]]
            if align:
                first, last = hm.align_decoded(n_keys=keys)
            if score:
                lps = _score(hm, res, prompt)
            for i, r in enumerate(res):
                if score:
                    r.update(token_logprob=lps[i])
                annotate(a + i, r)
                r.update(n_samples=int(totals[a + i]), n_keys=keys[i])
                if align:
                    r.update(token_first=first[i].copy(), token_last=last[i].copy())
                out.append(r)
    return out


def transcribe_recording(hm, pcm, params=None, max_new_tokens: int = 0, align: bool = False, prompt=None,
                         beam_size: int = 1, score: bool = False, guard=None, bias=None) -> List[dict]:
    """hm: a HipWhisper with weights, filters and tokens set.  pcm: a host f32 array (16 kHz mono), or (device pointer,
    n_samples).  params: the cut parameters (HipWhisper.cut_plan).  Returns one dict per chunk: the fields of decode_greedy
    plus start_sample, n_samples and n_keys = ceil(n_samples / 320), the encoder frames that hold audio.  align=True (the
    caller has set hm.align_capture): token_first / token_last of align_decoded(n_keys=...) as well.
    prompt: token ids every chunk decodes under (taken verbatim: <|startofprev|> first is the caller's to add; at most
    max_target_positions / 2 - 1 of them); the results exclude them.  Not together with align=True.
    score=True: token_logprob as well, f32 [len(tokens)]: ln p of every returned token under the model (HipWhisper.score on the
    group's returned sequences, after its align_decoded; 0.0 for the prompt tokens).
    guard, bias: the repetition guard of the chunks' decodes and one {token: beta} list for all of them (see _Guard)."""
    rec, n = _pcm(pcm)
    starts, lens = hm.cut_plan(rec, n, params)
    return _transcribe(hm, lens, lambda a, b: hm.logmel_chunks_rows(rec, starts[a:b], lens[a:b], 0),
                       lambda i, r: r.update(start_sample=int(starts[i])), max_new_tokens, align, prompt, beam_size, score, guard, bias)


def _segments(tokens, v):
    """(s, e) index pairs of the boundary tokens that delimit a chunk's segments, the way model.rs:100-105 does: a boundary
    token is a timestamp or eot, a segment runs from one boundary token to the next, and eot opens none"""
    def boundary(t):
        return t > tokens.no_timestamps or t == tokens.eot

    i = 0
    while True:
        s = next((j for j in range(i, len(v)) if boundary(v[j])), None)
        if s is None or v[s] == tokens.eot:
            return
        e = next((j for j in range(s + 1, len(v)) if boundary(v[j])), None)
        if e is None:
            return
        yield s, e
        if v[e] == tokens.eot:
            return
        i = e + 1


def stitch(results: Sequence[dict], tokens) -> List[Tuple[float, float, List[int]]]:
    """results: what transcribe_recording returned; tokens: the vocabulary's special tokens (eot, no_timestamps).
    Returns (start_s, end_s, token_ids) per segment, in order, on the recording's own time axis: a chunk's tokens are split
    at its timestamp tokens the way model.rs:100-105 delimits segments (a boundary token is a timestamp or eot; a segment
    runs from one boundary token to the next, both excluded from token_ids), and a timestamp token `t` of a chunk stands for
    start_sample / 16000 + 0.02 * (t - no_timestamps - 1) seconds.  A segment the decode left open (closed by eot instead of
    a timestamp) ends with its chunk.  Segments without text and chunks ended by the no-speech exit contribute nothing."""
    out = []
    for r in results:
        if r.get("no_speech_exit"):
            continue
        t0 = r["start_sample"] / SAMPLE_RATE
        v = list(r["tokens"])
        for s, e in _segments(tokens, v):
            start = t0 + 0.02 * (v[s] - tokens.no_timestamps - 1)
            end = (r["start_sample"] + r["n_samples"]) / SAMPLE_RATE if v[e] == tokens.eot else t0 + 0.02 * (v[e] - tokens.no_timestamps - 1)
            if e > s + 1:
                out.append((start, end, v[s + 1:e]))
    return out


def transcribe_speech(hm, pcm, params=None, max_new_tokens: int = 0, align: bool = False, prompt=None,
                      beam_size: int = 1, score: bool = False, guard=None, bias=None) -> List[dict]:
    """transcribe_recording on the recording's speech alone.  params: the parameters of HipWhisper.vad_plan.  Returns one dict
    per chunk (none for a recording without speech): the fields of decode_greedy plus pieces = [(offset_in_chunk, start_sample,
    n_samples)], n_samples = the chunk's total, n_keys = ceil(n_samples / 320), and with align=True token_first / token_last.  prompt, score:
    as for transcribe_recording; so are guard and bias."""
    rec, n = _pcm(pcm)
    starts, lens, first = hm.vad_plan(rec, n, params)
    pieces = []
    for k in range(len(first) - 1):
        off, row = 0, []
        for j in range(int(first[k]), int(first[k + 1])):
            row.append((off, int(starts[j]), int(lens[j])))
            off += int(lens[j])
        pieces.append(row)
    totals = [row[-1][0] + row[-1][2] for row in pieces]
    return _transcribe(hm, totals, lambda a, b: hm.logmel_pieces_rows(rec, starts, lens, first[a:b + 1], 0),
                       lambda i, r: r.update(pieces=pieces[i]), max_new_tokens, align, prompt, beam_size, score, guard, bias)


def to_recording(pieces: Sequence[Tuple[int, int, int]], tau_samples: float, end: bool = False) -> float:
    """A time inside a chunk (samples from the chunk's start) on the recording's axis (samples).  pieces: (offset_in_chunk,
    start_sample, n_samples) in order.  A start maps through the piece with off <= tau < off + len, an end through the piece
    with off < tau <= off + len: a segment that ends exactly at a piece's end stays in front of the dropped silence, one that
    starts there begins behind it.  Past the last piece: that piece's end."""
    for off, start, n in pieces:
        if (off < tau_samples <= off + n) if end else (off <= tau_samples < off + n):
            return start + (tau_samples - off)
    off, start, n = pieces[-1] if tau_samples > 0 else pieces[0]
    return start + min(max(tau_samples - off, 0), n)


def stitch_speech(results: Sequence[dict], tokens) -> List[Tuple[float, float, List[int]]]:
    """stitch for what transcribe_speech returned: the same segment rules, every time mapped through to_recording -- a
    segment's first timestamp as a start, its closing one as an end.  A segment closed by eot ends at the end of its chunk's
    last piece."""
    out = []
    for r in results:
        if r.get("no_speech_exit"):
            continue
        v, pieces = list(r["tokens"]), r["pieces"]
        for s, e in _segments(tokens, v):
            start = to_recording(pieces, KEY_SAMPLES * (v[s] - tokens.no_timestamps - 1)) / SAMPLE_RATE
            if v[e] == tokens.eot:
                end = (pieces[-1][1] + pieces[-1][2]) / SAMPLE_RATE
            else:
                end = to_recording(pieces, KEY_SAMPLES * (v[e] - tokens.no_timestamps - 1), end=True) / SAMPLE_RATE
            if e > s + 1:
                out.append((start, end, v[s + 1:e]))
    return out
