"""CPU: tokens into words (norma_amd/words.py) -- the byte-level vocabulary against the recorded decodes of the tokenizers
crate, and the merge rules on hand-made tables -- and the declaration of nh_score."""
import json
import math
import os

import numpy as np

import common
from norma_amd import hip, words

ASSETS = os.path.join(common.ROOT, "tests", "golden", "assets")
SPECIAL = 600   # first special id of the hand-made tables below


def test_token_bytes_decode_to_the_recorded_text():
    """Concatenated pieces decode (lossily, as the crate does) to what tokenizers' decode(skip_special_tokens = true) gave.
    That decode keeps the text of added tokens that are not special (timestamps); token_bytes maps them to b"", so they are
    spelled out here from the file."""
    path = os.path.join(ASSETS, "tokenizer.json")
    tb = words.token_bytes(path)
    with open(path, encoding="utf-8") as f:
        added = {a["id"]: a for a in json.load(f)["added_tokens"]}
    with open(os.path.join(ASSETS, "tokenizer_cases.json"), encoding="utf-8") as f:
        cases = json.load(f)
    assert len(tb) == cases["vocab_size"]
    assert all(tb[i] == b"" for i in added) and all(isinstance(b, bytes) for b in tb)
    assert all(tb[i] for i in range(len(tb)) if i not in added), "every vocabulary entry has bytes"
    for name, i in cases["token_to_id"].items():
        if i is not None and i not in added:
            assert tb[i].decode("utf-8") == name.replace("Ġ", " "), name
    assert len(cases["cases"]) > 20
    for case in cases["cases"]:
        bs = b""
        for i in case["ids"]:
            if i >= len(tb):
                continue   # the crate ignores ids beyond the vocabulary
            bs += tb[i] if i not in added else (b"" if added[i]["special"] else added[i]["content"].encode())
        assert bs.decode("utf-8", errors="replace") == case["skip_special"], case["note"]


def table(*pieces):
    """ids 0 .. of the given pieces (str or bytes), then specials from SPECIAL on"""
    tb = [p.encode() if isinstance(p, str) else p for p in pieces]
    return tb + [b""] * (SPECIAL + 8 - len(tb))


def run(tb, ids, prompt_len=0, logprob=None, first=None, last=None):
    n = len(ids)
    first = list(range(10, 10 + n)) if first is None else first
    last = [f + 1 for f in first] if last is None else last
    logprob = [-0.1 * (i + 1) for i in range(n)] if logprob is None else logprob
    return words.merge(ids, tb, first, last, logprob, prompt_len, n, SPECIAL)


def test_a_leading_space_splits_and_a_bare_piece_continues():
    tb = table(" hello", " wor", "ld", " again")
    w = run(tb, [0, 1, 2, 3])
    assert [x["text"] for x in w] == [" hello", " world", " again"]
    assert [x["tokens"] for x in w] == [[0], [1, 2], [3]]
    # times: first frame of the first token, one past the last frame of the last; probability: exp(mean)
    assert w[1]["start"] == 0.02 * 11 and w[1]["end"] == 0.02 * (13 + 1)
    assert w[1]["probability"] == math.exp((-0.2 + -0.30000000000000004) / 2)
    assert w[0]["probability"] == math.exp(-0.1 / 1) and w[0]["start"] == 0.02 * 10 and w[0]["end"] == 0.02 * 12


def test_a_character_split_across_two_tokens_stays_one_word():
    e = "é".encode()
    tb = table(" caf", e[:1], e[1:], " au")
    w = run(tb, [0, 1, 2, 3])
    assert [x["text"] for x in w] == [" café", " au"] and w[0]["tokens"] == [0, 1, 2]
    # ... even when the piece after the incomplete one starts with a space
    w = run(tb, [0, 1, 3])
    assert [x["tokens"] for x in w] == [[0, 1, 2]] and w[0]["text"] == " caf� au"   # indices into the sequence


def test_punctuation_joins_its_neighbours():
    tb = table(" \"", " hello", ",", " world", ".", " (", " x", " )", " ,")
    w = run(tb, [0, 1, 2, 3, 4])
    assert [x["text"] for x in w] == [" \" hello,", " world."]
    assert [x["tokens"] for x in w] == [[0, 1, 2], [3, 4]]
    w = run(tb, [5, 6, 7, 8, 3])
    assert [x["text"] for x in w] == [" ( x ) ,", " world"]
    assert [x["tokens"] for x in w] == [[0, 1, 2, 3], [4]]


def test_special_tokens_end_a_word_and_belong_to_none():
    tb = table(" one", "s", " two")
    ts0, ts1, eot = SPECIAL + 3, SPECIAL + 5, SPECIAL
    ids = [SPECIAL + 1, SPECIAL + 2, ts0, 0, ts1, 1, 2, eot]
    w = run(tb, ids, prompt_len=2)
    assert [x["text"] for x in w] == [" one", "s", " two"]       # "s" does not continue a word a timestamp has ended
    assert [x["tokens"] for x in w] == [[3], [5], [6]]
    assert all(ids[i] < SPECIAL for x in w for i in x["tokens"])


def test_an_empty_sequence_and_a_sequence_of_specials_have_no_words():
    tb = table(" a")
    assert words.merge([], tb, [], [], [], 0, 0, SPECIAL) == []
    assert run(tb, [SPECIAL + 1, SPECIAL + 2, SPECIAL], prompt_len=2) == []
    assert run(tb, [0, 0], prompt_len=2) == []                   # everything is prompt


def test_times_and_probability_are_the_exact_expressions():
    tb = table(" a", "b", "c")
    lp = np.array([-0.5, -1.25, -0.125], dtype=np.float32)
    w = run(tb, [0, 1, 2], logprob=lp, first=[7, 9, 40], last=[8, 12, 41])
    assert len(w) == 1
    assert w[0]["start"] == 0.02 * 7 and w[0]["end"] == 0.02 * (41 + 1)
    assert w[0]["probability"] == math.exp((float(lp[0]) + float(lp[1]) + float(lp[2])) / 3)


def test_nh_score_is_declared():
    assert "nh_score" in hip.declared_symbols()
