"""NGramLM — a back-off n-gram language model (order <= 3) over the CTC vocabulary's token ids, for shallow fusion
inside the CTC prefix beam search (ctc.beam_search_decode(..., lm=...), csrc/ctc_beam.hip).

The vocabulary is a word list (lib/standard/myvocab.py: ids are words), so a token n-gram is a word n-gram; no
lexicon is involved.  <s> and </s> take the pseudo-ids V and V + 1.  The reference only names LM fusion
(runner.py:78-101, a transformer LM whose weights never reach the model); this is the n-gram form every CTC decoder
carries.

  from_arpa(path_or_text, vocab)             standard ARPA text (log10 -> natural log in fp64)
  from_token_ids / from_sentences / from_dataset
                                             absolute discounting that normalises exactly (see from_token_ids)
  logp(context, w)                           the fp64 host query on the fp32 table values: the definition
  to_arpa(vocab)                             9 significant digits (round trip within 1 fp32 ulp)
  device_tables(device)                      the packed form the kernel reads, cached per device

Device form: `uni` (V + 2, 2) fp32 {logp, backoff}; `table` (capacity, 2) int64 = 16-byte slots {uint64 key, float
logp, float backoff} for bigrams and trigrams, open-addressed, capacity a power of two, every key within `probe`
<= 4 slots of its home (asserted when built).  key = order << 45 | a << 30 | b << 15 | c (15-bit ids; a bigram has
a = 0); an empty slot is all ones.
"""
from __future__ import annotations

import math
import os

import numpy as np

LN10 = math.log(10.0)
LOG_ZERO = -99.0 * LN10        # ARPA's "-99": probability zero
MAX_ORDER = 3
MAX_PROBE = 4
EMPTY_KEY = (1 << 64) - 1
_M64 = (1 << 64) - 1


def pack_key(ids):
    """(a, b[, c]) -> the table key of a bigram / trigram."""
    k = len(ids) << 45
    for x in ids:
        assert 0 <= x < (1 << 15)
    if len(ids) == 2:
        return k | ids[0] << 15 | ids[1]
    return k | ids[0] << 30 | ids[1] << 15 | ids[2]


def home_slot(key, seed, mask):
    z = ((key ^ seed) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 32)) * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 29
    return z & mask


class NGramLM:
    def __init__(self, ngrams, V, blank, pad, order):
        """ngrams: {ids tuple (length 1..order): (logp, backoff)} natural log, fp64; use the from_* constructors."""
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"n-gram order must be in [1, {MAX_ORDER}], got {order}")
        if not 2 <= V <= 16384:
            raise ValueError("2 <= V <= 16384")
        self.V, self.blank, self.pad, self.order = int(V), int(blank), int(pad) if pad is not None else -1, int(order)
        self.bos, self.eos = self.V, self.V + 1
        self.exact = {tuple(k): (float(v[0]), float(v[1])) for k, v in ngrams.items()}
        for k in self.exact:
            if not 1 <= len(k) <= order or any(not 0 <= x <= self.eos for x in k):
                raise ValueError(f"bad n-gram {k}")
        self.table32 = {k: (float(np.float32(lp)), float(np.float32(bo))) for k, (lp, bo) in self.exact.items()}
        self.has_eos = (self.eos,) in self.exact
        missing = [c for c in self.scorable() if (c,) not in self.exact]
        if missing:
            raise ValueError(f"tokens without a unigram (and no <unk> entry to stand in): {missing[:8]}")
        self._dev = {}

    # ------------------------------------------------------------------------------------------ construction
    def scorable(self):
        """Token ids the decoder may emit: all but blank and pad."""
        return [c for c in range(self.V) if c != self.blank and c != self.pad]

    @classmethod
    def from_arpa(cls, path_or_text, vocab, blank=None, pad=None):
        """Words map through vocab.stoi (<s>, </s> -> V, V + 1); n-grams with a word outside the vocabulary are
        dropped; a scorable token without a unigram takes the file's <unk> entry."""
        text = path_or_text
        if "\n" not in str(path_or_text) and os.path.exists(str(path_or_text)):
            with open(path_or_text, "r", encoding="utf-8") as f:
                text = f.read()
        V = len(vocab)
        blank = vocab.blank_idx if blank is None else blank
        pad = vocab.pad_idx if pad is None else pad
        stoi = dict(vocab.stoi)
        stoi["<s>"], stoi["</s>"] = V, V + 1
        ngrams, n, top, unk = {}, 0, 0, None
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\":
                continue
            if line == "\\end\\":
                break
            if line.startswith("ngram "):
                o, cnt = line[6:].split("=")
                if int(cnt) > 0:
                    top = max(top, int(o))
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-7])
                if n > MAX_ORDER:
                    raise ValueError(f"ARPA order {n} > {MAX_ORDER}")
                continue
            if n == 0:
                continue
            f = line.split()
            if len(f) not in (n + 1, n + 2):
                raise ValueError(f"malformed ARPA line: {line!r}")
            lp = float(f[0]) * LN10
            bo = float(f[n + 1]) * LN10 if len(f) == n + 2 else 0.0
            words = f[1:n + 1]
            if n == 1 and words[0] == "<unk>":
                unk = (lp, bo)
            if all(w in stoi for w in words):
                ngrams[tuple(stoi[w] for w in words)] = (lp, bo)
        if top > MAX_ORDER:
            raise ValueError(f"ARPA order {top} > {MAX_ORDER}")
        order = max((len(k) for k in ngrams), default=1)
        if unk is not None:
            for c in range(V):
                if c != blank and c != pad and (c,) not in ngrams:
                    ngrams[(c,)] = (unk[0], 0.0)
        return cls(ngrams, V, blank, pad, order)

    @classmethod
    def from_token_ids(cls, seqs, V, blank, pad, order=3, discount=0.75):
        """Back-off model with absolute discounting D, over S = scorable tokens plus </s>, counts taken over
        <s> w1..wn </s>:
          P(w) = (c(w) + 1) / (sum c + |S|);
          seen context h (h' = h less its oldest symbol): c(h) = sum_w c(hw), n+(h) distinct successors,
          P(w | h) = (c(hw) - D) / c(h) for c(hw) > 0, bo(h) = (D n+(h) / c(h)) / (1 - sum_{seen w} P(w | h'));
          a context that has seen all of S takes D = 0; an unseen context has back-off 0 (log).
        sum_{w in S} P(w | h) = 1 for every h."""
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"n-gram order must be in [1, {MAX_ORDER}], got {order}")
        pad = -1 if pad is None else int(pad)
        bos, eos = V, V + 1
        S = [c for c in range(V) if c != blank and c != pad] + [eos]
        counts = [dict() for _ in range(order + 1)]          # counts[n]: {ids: c}
        for s in seqs:
            s = [bos] + [int(c) for c in s if 0 <= int(c) < V and c != blank and c != pad] + [eos]
            for n in range(1, order + 1):
                for i in range(len(s) - n + 1):
                    g = tuple(s[i:i + n])
                    if n == 1 and g[0] == bos:
                        continue
                    counts[n][g] = counts[n].get(g, 0) + 1
        total = sum(counts[1].values())
        prob = {(w,): (counts[1].get((w,), 0) + 1) / (total + len(S)) for w in S}
        bo = {}
        for n in range(2, order + 1):
            by_ctx = {}
            for g, c in counts[n].items():
                by_ctx.setdefault(g[:-1], []).append((g[-1], c))
            for h, succ in by_ctx.items():
                ch = sum(c for _, c in succ)
                D = 0.0 if len(succ) == len(S) else float(discount)
                lower = 0.0
                for w, c in succ:
                    prob[h + (w,)] = (c - D) / ch
                    lower += prob[h[1:] + (w,)]
                bo[h] = (D * len(succ) / ch) / (1.0 - lower) if D > 0.0 else 0.0
        log = lambda p: math.log(p) if p > 0.0 else LOG_ZERO
        ngrams = {g: (log(p), log(bo[g]) if g in bo else 0.0) for g, p in prob.items()}
        for h, b in bo.items():
            if h not in ngrams:                             # (<s>): a context only
                ngrams[h] = (LOG_ZERO, log(b))
        return cls(ngrams, V, blank, pad, order)

    @classmethod
    def from_sentences(cls, sentences, vocab, order=3, discount=0.75):
        return cls.from_token_ids([vocab.parse(s) for s in sentences], len(vocab), vocab.blank_idx, vocab.pad_idx,
                                  order, discount)

    @classmethod
    def from_dataset(cls, dataset, split="train", order=3, discount=0.75):
        """The teacher's LM: estimated from the transcripts of a labelled split of a MelDataset."""
        seqs = [r["target"]["transcripts"][:r["target"]["lens"]] for r in dataset.data[split] if r["target"]["lens"]]
        v = dataset.vocab
        return cls.from_token_ids(seqs, len(v), v.blank_idx, v.pad_idx, order, discount)

    # ------------------------------------------------------------------------------------------ queries
    def context(self, prefix):
        """h(l): the last min(order - 1, |l| + 1) symbols of <s> + l."""
        if self.order == 1:
            return ()
        return ((self.bos,) + tuple(int(c) for c in prefix))[-(self.order - 1):]

    def logp(self, context, w, exact=False, trace=None):
        """Natural-log back-off probability of w after `context` (ids, oldest first; only the last order - 1 are
        used), in fp64 on the fp32 table values (exact=True: on the fp64 values they were rounded from).  trace: an
        optional dict counting the path taken ("tri", "bi", "uni": the level that hit; "backoff_seen" /
        "backoff_unseen": each context left, with / without a stored back-off)."""
        tab = self.exact if exact else self.table32
        ctx = tuple(int(c) for c in context)
        ctx = ctx[-(self.order - 1):] if self.order > 1 else ()
        w = int(w)
        acc = 0.0
        while True:
            hit = tab.get(ctx + (w,))
            if hit is not None:
                if trace is not None:
                    lvl = ("uni", "bi", "tri")[len(ctx)]
                    trace[lvl] = trace.get(lvl, 0) + 1
                return acc + hit[0]
            if not ctx:
                return -math.inf
            b = tab.get(ctx)
            if trace is not None:
                lab = "backoff_seen" if b is not None else "backoff_unseen"
                trace[lab] = trace.get(lab, 0) + 1
            acc += b[1] if b is not None else 0.0
            ctx = ctx[1:]

    def to_arpa(self, vocab):
        words = list(vocab.itos) + ["<s>", "</s>"]
        by_n = [[k for k in sorted(self.table32) if len(k) == n] for n in range(1, self.order + 1)]
        out = ["\\data\\"] + [f"ngram {n + 1}={len(g)}" for n, g in enumerate(by_n)] + [""]
        for n, grams in enumerate(by_n, 1):
            out.append(f"\\{n}-grams:")
            for k in grams:
                lp, bo = self.table32[k]
                line = f"{lp / LN10:.9g}\t{' '.join(words[i] for i in k)}"
                if n < self.order and bo != 0.0:
                    line += f"\t{bo / LN10:.9g}"
                out.append(line)
            out.append("")
        out.append("\\end\\")
        return "\n".join(out) + "\n"

    # ------------------------------------------------------------------------------------------ device form
    def _pack(self):
        uni = np.zeros((self.V + 2, 2), np.float32)
        uni[:, 0] = -np.inf
        keys = {}
        for k, (lp, bo) in self.table32.items():
            if len(k) == 1:
                uni[k[0]] = (lp, bo)
            else:
                keys[pack_key(k)] = (lp, bo)
        cap = 16
        while cap < 2 * len(keys):
            cap *= 2
        while True:
            for seed in range(1, 33):
                seed = (seed * 0xD6E8FEB86659FD93) & _M64
                slots = [EMPTY_KEY] * cap
                worst, ok = 0, True
                for key in keys:
                    h = home_slot(key, seed, cap - 1)
                    d = 0
                    while d < MAX_PROBE and slots[(h + d) & (cap - 1)] != EMPTY_KEY:
                        d += 1
                    if d == MAX_PROBE:
                        ok = False
                        break
                    slots[(h + d) & (cap - 1)] = key
                    worst = max(worst, d)
                if ok:
                    table = np.zeros((cap, 2), np.uint64)
                    table[:, 0] = np.array(slots, dtype=np.uint64)
                    vals = np.zeros((cap, 2), np.float32)
                    for i, key in enumerate(slots):
                        if key != EMPTY_KEY:
                            vals[i] = keys[key]
                    table[:, 1] = vals.view(np.uint64)[:, 0]
                    probe = worst + 1
                    for key in keys:                        # every key lies within `probe` slots of its home
                        h = home_slot(key, seed, cap - 1)
                        assert any(slots[(h + d) & (cap - 1)] == key for d in range(probe))
                    assert probe <= MAX_PROBE
                    return dict(uni=uni, table=table.view(np.int64), mask=cap - 1, probe=probe, seed=seed,
                                order=self.order, V=self.V)
            cap *= 2

    def device_tables(self, device):
        """{"uni": (V + 2, 2) fp32, "table": (capacity, 2) int64, "mask", "probe", "seed", "order", "V"} with the two
        tensors on `device`; packed once, cached per device."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if "host" not in self._dev:
            self._dev["host"] = self._pack()
        if device not in self._dev:
            h = self._dev["host"]
            d = dict(h)
            d["uni"] = torch.from_numpy(h["uni"]).to(device)
            d["table"] = torch.from_numpy(h["table"]).to(device)
            self._dev[device] = d
        return self._dev[device]
