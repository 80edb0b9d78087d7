"""CPU: the orchestration of norma_amd/longform.py (transcribe_recording, transcribe_speech) against a logging stand-in for
HipWhisper: which engine calls a recording's chunks turn into, in which order, and which fields every result carries, in which
order.  longform_trace_parent.json holds both as the two functions produced them when each still had a chunk loop of its own
(this file run as a script at that commit); the GPU side is tests/test_gpu_cut.py, test_gpu_vad.py, test_gpu_score.py,
test_gpu_prompt.py and test_gpu_guard.py."""
import json
import os

import numpy as np
import pytest

from norma_amd import longform

TRACE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "longform_trace_parent.json")
SOT, TASK, EOT = 90, 91, 80
CHUNKS = [48000, 30000, 480000, 161, 160, 9000, 100]      # 7 chunks, the last shorter than 160 samples: it goes alone
MUTE = 3                                                  # the chunk that takes the no-speech exit: the bare prompt comes back


class Hm:
    """decode_* answer with tokens made of (call, row), so a result shows which decode of which group it came from"""
    max_batch, _task, _eot = 3, TASK, EOT

    def __init__(self, fail_decode=0):
        self.log, self.decodes, self.fail_decode, self.batch, self.chunk0 = [], 0, fail_decode, 0, 0

    @staticmethod
    def _rec(rec, n):
        return (f"{rec.dtype}{list(rec.shape)} contiguous={rec.flags.c_contiguous}", n) if isinstance(rec, np.ndarray) else (rec, n)

    def cut_plan(self, rec, n, params):
        self.log.append(("cut_plan", self._rec(rec, n), params))
        lens = np.array(CHUNKS, dtype=np.int64)
        self.first_of = (np.cumsum(lens) - lens + 7).tolist()     # what a group's first argument names its first chunk by
        return np.array(self.first_of), lens

    def vad_plan(self, rec, n, params):
        """chunk k is made of 1 + k % 3 pieces that add up to CHUNKS[k], with 50 samples of silence dropped between pieces"""
        self.log.append(("vad_plan", self._rec(rec, n), params))
        starts, lens, first, at = [], [], [0], 11
        for k, total in enumerate(CHUNKS):
            m = 1 + k % 3
            for j in range(m):
                ln = total // m + (total % m if j == m - 1 else 0)
                starts.append(at)
                lens.append(ln)
                at += ln + 50
            first.append(len(starts))
        self.first_of = first[:-1]
        return np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int32), np.array(first, dtype=np.int32)

    def logmel_chunks_rows(self, rec, starts, lens, row0):
        self.log.append(("logmel_chunks_rows", self._rec(rec, None)[0], [int(v) for v in starts], [int(v) for v in lens], row0))
        self.chunk0, self.batch = self.first_of.index(int(starts[0])), len(lens)

    def logmel_pieces_rows(self, rec, starts, lens, first, row0):
        self.log.append(("logmel_pieces_rows", self._rec(rec, None)[0], len(starts), len(lens), [int(v) for v in first], row0))
        self.chunk0, self.batch = self.first_of.index(int(first[0])), len(first) - 1

    def encode(self):
        self.log.append(("encode", self.batch))

    def set_prompts(self, prompts):
        self.log.append(("set_prompts", prompts))

    def _decode(self, name, *args):
        self.log.append((name,) + args)
        self.decodes += 1
        if self.decodes == self.fail_decode:
            raise RuntimeError("decode failed")
        out = []
        for i in range(self.batch):
            mute = self.chunk0 + i == MUTE
            toks = [SOT, TASK] + ([] if mute else [10 + self.decodes, 20 + i, 30 + self.chunk0 + i, EOT])
            out.append(dict(tokens=toks, avg_logprob=-0.1 * (self.chunk0 + i), no_speech_prob=0.9 if mute else 0.1, no_speech_exit=mute))
        return out

    def decode_greedy(self, max_new_tokens):
        return self._decode("decode_greedy", max_new_tokens)

    def decode_beam(self, beam_size, max_new_tokens):
        assert self.batch * beam_size <= self.max_batch
        return self._decode("decode_beam", beam_size, max_new_tokens)

    def align_decoded(self, n_keys=None):
        self.log.append(("align_decoded", list(n_keys)))
        first = np.arange(self.batch * 8, dtype=np.int32).reshape(self.batch, 8) + 100 * self.decodes
        return first, first + 1000

    def score(self, seqs, prompt_len):
        self.log.append(("score", [list(s) for s in seqs], prompt_len))
        lp = np.zeros((len(seqs), max(len(s) for s in seqs)), dtype=np.float32)
        for i, s in enumerate(seqs):
            lp[i, prompt_len:len(s)] = [-0.25 * t for t in s[prompt_len:]]
        return lp

    def set_guard(self, *args, **kw):
        self.log.append(("set_guard", list(args), kw))

    def guard_bias(self, row, bias):
        self.log.append(("guard_bias", row, bias))

    def guard_report(self):
        self.log.append(("guard_report",))
        return [int((self.chunk0 + i) % 2) for i in range(self.batch)]


GUARD = dict(no_repeat_ngram=3, loop_period=4, loop_repeats=3, bias=True)
CASES = {
    "plain": dict(),
    "device_pointer": dict(),                 # pcm as (device pointer, n_samples)
    "params_max_new": dict(params={"max_s": 30.0}, max_new_tokens=40),
    "align": dict(align=True),
    "score": dict(score=True),
    "align_score": dict(align=True, score=True),
    "prompt": dict(prompt=[60, 61, 62]),
    "prompt_score": dict(prompt=[60, 61, 62], score=True),
    "beam": dict(beam_size=3),
    "beam_score_guard": dict(beam_size=3, score=True, guard=GUARD),
    "guard_bias": dict(guard=GUARD, bias={5: -1.5, 6: 2.0}),
    "guard_without_loop_exit": dict(guard=dict(no_repeat_ngram=3)),
    "bias_alone": dict(bias={5: -1.5}),
}
FUNCTIONS = {"recording": longform.transcribe_recording, "speech": longform.transcribe_speech}
PCM = np.zeros((2, sum(CHUNKS) + 1000), dtype=np.float64)[:, ::2]      # not f32, flat or contiguous: the call sees to it once


def plain(v):
    return v.tolist() if isinstance(v, np.ndarray) else v


def trace(fn, case):
    """the stand-in's call log and every result as its (field, value) pairs in order, as JSON holds them"""
    hm = Hm()
    res = FUNCTIONS[fn](hm, (0xABC000, PCM.size) if case == "device_pointer" else PCM, **CASES[case])
    return json.loads(json.dumps(dict(log=hm.log, results=[[[k, plain(v)] for k, v in r.items()] for r in res])))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("fn", list(FUNCTIONS))
def test_the_engine_calls_and_the_result_fields_are_what_they_were_with_a_chunk_loop_per_function(fn, case):
    with open(TRACE_PATH) as f:
        want = json.load(f)[f"{fn}-{case}"]
    got = trace(fn, case)
    assert got["log"] == want["log"]
    assert got["results"] == want["results"]


@pytest.mark.parametrize("fn", list(FUNCTIONS))
def test_the_calls_and_fields_spelled_out(fn):
    """what the recorded traces hold, by hand, for the head of a guarded, scored run: plan, guard and bias on rows 0 .. 2, then
    per group log-mel, encode, decode, report, score; 7 chunks in groups of 3, 3 and the short one alone"""
    hm = Hm()
    res = FUNCTIONS[fn](hm, PCM, score=True, guard=GUARD, bias={5: -1.5})
    names = [x[0] for x in hm.log]
    mel = "logmel_chunks_rows" if fn == "recording" else "logmel_pieces_rows"
    group = [mel, "encode", "decode_greedy", "guard_report", "score"]
    assert names == ["cut_plan" if fn == "recording" else "vad_plan", "set_guard"] + ["guard_bias"] * 3 + group * 3 + ["guard_bias"] * 3 + ["set_guard"]
    assert [x[1] for x in hm.log if x[0] == "encode"] == [3, 3, 1]
    assert hm.log[1] == ("set_guard", [], GUARD) and hm.log[-1] == ("set_guard", [None], {})
    assert [x[1:] for x in hm.log if x[0] == "guard_bias"] == [(r, {5: -1.5}) for r in range(3)] + [(r, None) for r in range(3)]
    own = ["start_sample"] if fn == "recording" else ["pieces"]
    for i, r in enumerate(res):
        assert list(r) == ["tokens", "avg_logprob", "no_speech_prob", "no_speech_exit", "loop_exit", "token_logprob"] + own + ["n_samples", "n_keys"]
        assert r["n_samples"] == CHUNKS[i] and r["n_keys"] == -(-CHUNKS[i] // 320) and r["loop_exit"] == bool(i % 2)
        assert r["token_logprob"].dtype == np.float32 and len(r["token_logprob"]) == len(r["tokens"])
    assert not res[MUTE]["token_logprob"].any() and res[0]["token_logprob"].tolist() == [0.0, 0.0, -2.75, -5.0, -7.5, -20.0]
    if fn == "speech":
        starts = hm.vad_plan(PCM, None, None)[0]
        assert res[4]["pieces"] == [(0, starts[7], 80), (80, starts[8], 80)]      # chunks 0 .. 3 are 1 + 2 + 3 + 1 pieces


@pytest.mark.parametrize("fn", list(FUNCTIONS))
def test_align_is_refused_with_a_prompt_and_with_a_beam(fn):
    hm = Hm()
    with pytest.raises(ValueError, match="prompted"):
        FUNCTIONS[fn](hm, PCM, align=True, prompt=[60])
    assert not [x for x in hm.log if x[0] in ("set_prompts", "decode_greedy", "align_decoded")]
    hm = Hm()
    with pytest.raises(ValueError, match="beam"):
        FUNCTIONS[fn](hm, PCM, align=True, beam_size=3)
    assert [x[0] for x in hm.log] == ["cut_plan" if fn == "recording" else "vad_plan"]
    for k in (0, 4):
        with pytest.raises(ValueError, match="beam_size"):
            FUNCTIONS[fn](Hm(), PCM, beam_size=k)


@pytest.mark.parametrize("fn", list(FUNCTIONS))
def test_the_guard_and_the_bias_lists_are_cleared_when_a_decode_raises(fn):
    hm = Hm(fail_decode=2)
    with pytest.raises(RuntimeError, match="decode failed"):
        FUNCTIONS[fn](hm, PCM, guard=GUARD, bias={5: -1.5})
    assert [x[0] for x in hm.log[-5:]] == ["decode_greedy", "guard_bias", "guard_bias", "guard_bias", "set_guard"]
    assert [x[1:] for x in hm.log[-4:-1]] == [(r, None) for r in range(3)] and hm.log[-1] == ("set_guard", [None], {})


if __name__ == "__main__":
    with open(TRACE_PATH, "w") as f:
        json.dump({f"{fn}-{case}": trace(fn, case) for fn in FUNCTIONS for case in CASES}, f, separators=(",", ":"))
        f.write("\n")
