"""Tokens into words: text, times and a probability per word, from what the library already returns per token -- the first and
last encoder frame (HipWhisper.align / align_decoded) and the log-probability (HipWhisper.score).  Pure Python / numpy, no GPU.

A word's probability is exp(mean of its tokens' log-probabilities); its times are the frames of its first and last token.
There are no duration heuristics."""
import json
import math
from typing import List, Sequence

FRAME_S = 0.02   # one encoder frame

# a word made of one of these alone is glued to the word after it / before it
PREPEND = "\"'“¿([{-"
APPEND = "\"'.。,，!！?？:：”)]}、"


def _byte_decoder():
    """The inverse of GPT-2's byte map: printable latin-1 code points stand for themselves, the other bytes for 256, 257, ..."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    chars, n = list(keep), 0
    for b in range(256):
        if b not in keep:
            keep.append(b)
            chars.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(keep, chars)}


def token_bytes(tokenizer_json_path: str) -> List[bytes]:
    """The bytes of every token id of a Hugging Face tokenizer.json with a byte-level BPE model: vocabulary entries through
    the GPT-2 byte map; added and special tokens (timestamps, <|endoftext|>, ...) map to b""."""
    with open(tokenizer_json_path, encoding="utf-8") as f:
        tj = json.load(f)
    vocab = tj["model"]["vocab"]
    added = tj.get("added_tokens", [])
    n = 1 + max(list(vocab.values()) + [a["id"] for a in added])
    dec = _byte_decoder()
    out = [b""] * n
    for text, i in vocab.items():
        out[i] = bytes(dec[ch] for ch in text)
    for a in added:
        out[a["id"]] = b""
    return out


def _complete(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def merge(tokens: Sequence[int], pieces: Sequence[bytes], first: Sequence[int], last: Sequence[int], logprob: Sequence[float],
          prompt_len: int, n_tokens: int, first_special: int) -> List[dict]:
    """Words of one clip.  tokens / first / last / logprob: per token index, as a decode, align and score returned them;
    pieces: token_bytes(...).  Tokens [prompt_len, n_tokens) are looked at.
      * an id >= first_special (eot, timestamps, ...) ends the current word and belongs to none;
      * a token opens a new word when its piece starts with a space, or when the word before is complete (a special token
        ended it, or there is none) -- and only if the bytes collected so far decode as UTF-8: a piece that leaves an
        incomplete sequence stays glued to the next token, whatever that one starts with;
      * a word that is one of PREPEND alone goes in front of the following word, then one of APPEND alone behind the
        preceding one (\" and ' are in both: in front where a word follows).
    Returns dicts: text, tokens (indices into `tokens`), start = 0.02 first[first token], end = 0.02 (last[last token] + 1),
    probability = exp(mean of the tokens' log-probabilities)."""
    words, cur = [], None   # [bytes, token indices]
    for i in range(prompt_len, n_tokens):
        t = int(tokens[i])
        if t >= first_special:
            if cur is not None:
                words.append(cur)
            cur = None
            continue
        piece = pieces[t]
        if cur is not None and piece.startswith(b" ") and _complete(cur[0]):
            words.append(cur)
            cur = None
        if cur is None:
            cur = [b"", []]
        cur[0] += piece
        cur[1].append(i)
    if cur is not None:
        words.append(cur)
    texts = [[w[0].decode("utf-8", errors="replace"), w[1]] for w in words]

    def alone(text, chars):
        s = text.strip()
        return len(s) == 1 and s in chars

    fronted = []
    for k, (text, idx) in enumerate(texts):
        if fronted and fronted[-1][2]:   # the word before waits to go in front of this one
            fronted[-1] = [fronted[-1][0] + text, fronted[-1][1] + idx, False]
        else:
            fronted.append([text, idx, False])
        fronted[-1][2] = alone(text, PREPEND) and k + 1 < len(texts)
    out = []
    for text, idx, _ in fronted:
        if out and alone(text, APPEND):
            out[-1] = [out[-1][0] + text, out[-1][1] + idx]
        else:
            out.append([text, idx])
    res = []
    for text, idx in out:
        lp = [float(logprob[i]) for i in idx]
        res.append(dict(text=text, tokens=list(idx), start=FRAME_S * int(first[idx[0]]), end=FRAME_S * (int(last[idx[-1]]) + 1),
                        probability=math.exp(sum(lp) / len(lp))))
    return res
