"""lm.NGramLM on the CPU: ARPA reading against hand-computed values, exact normalisation of the estimated model, the
ARPA round trip, and the packed device table read back with a numpy restatement of the kernel's probe."""
import math

import numpy as np
import pytest

from nn_conformer_for_speech_recognition_amd.lib.standard.myvocab import Vocab
from nn_conformer_for_speech_recognition_amd.lm import NGramLM

LN10 = math.log(10.0)
VOCAB = Vocab(["<blank>", "<pad>", "a", "b", "c"])
A, B, C, BOS, EOS = 2, 3, 4, 5, 6

ARPA = """\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-0.7 a -0.3
-0.8 b -0.2
-0.9 c

\\2-grams:
-0.4 <s> a -0.25
-0.6 a b -0.15
-0.5 b c
-0.3 b </s>

\\3-grams:
-0.2 <s> a b
-0.1 a b c

\\end\\
"""


def test_arpa_hand_computed_values_on_every_path():
    lm = NGramLM.from_arpa(ARPA, VOCAB)
    assert (lm.V, lm.order, lm.blank, lm.pad, lm.has_eos) == (5, 3, 0, 1, True)
    want = [
        ((A, B), C, -0.1, {"tri": 1}),                                       # trigram hit
        ((BOS, A), B, -0.2, {"tri": 1}),
        ((A, B), EOS, -0.15 - 0.3, {"backoff_seen": 1, "bi": 1}),            # back-off to a bigram hit
        ((A, B), A, -0.15 - 0.2 - 0.7, {"backoff_seen": 2, "uni": 1}),       # through both to the unigram
        ((C, A), C, 0.0 - 0.3 - 0.9, {"backoff_unseen": 1, "backoff_seen": 1, "uni": 1}),   # unseen context: 0
        ((B, C), A, 0.0 + 0.0 - 0.7, {"backoff_seen": 2, "uni": 1}),         # stored without a back-off: 0
        ((BOS,), A, -0.4, {"bi": 1}),                                        # first token: context (<s>)
        ((BOS,), C, -0.5 - 0.9, {"backoff_seen": 1, "uni": 1}),
        ((C, C, A, B), C, -0.1, {"tri": 1}),                                 # only the last two symbols count
    ]
    for ctx, w, log10, path in want:
        trace = {}
        got = lm.logp(ctx, w, trace=trace)
        assert abs(got - log10 * LN10) < 1e-6, (ctx, w, got, log10 * LN10)
        assert trace == path, (ctx, w, trace)
    assert lm.context(()) == (BOS,) and lm.context((A,)) == (BOS, A) and lm.context((A, B, C)) == (B, C)
    # a file on disk reads the same
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "lm.arpa")
        with open(path, "w") as f:
            f.write(ARPA)
        assert NGramLM.from_arpa(path, VOCAB).table32 == lm.table32


def test_arpa_order_four_and_missing_unigram_raise():
    four = ARPA.replace("ngram 3=2", "ngram 3=2\nngram 4=1").replace("\\end\\", "\\4-grams:\n-0.1 a b c a\n\n\\end\\")
    with pytest.raises(ValueError):
        NGramLM.from_arpa(four, VOCAB)
    with pytest.raises(ValueError):                          # c has no unigram and the file no <unk>
        NGramLM.from_arpa(ARPA.replace("-0.9 c\n", ""), VOCAB)
    lm = NGramLM.from_arpa(ARPA.replace("-0.9 c\n", "-2.5 <unk>\n"), VOCAB)
    assert abs(lm.logp((), C) + 2.5 * LN10) < 1e-6
    # an n-gram with a word outside the vocabulary is dropped
    lm2 = NGramLM.from_arpa(ARPA.replace("-0.5 b c\n", "-0.5 b c\n-0.1 b zebra\n"), VOCAB)
    assert lm2.table32 == NGramLM.from_arpa(ARPA, VOCAB).table32


def _model(seed=0, V=12, n=60, order=3, blank=0, pad=1):
    rng = np.random.default_rng(seed)
    toks = [c for c in range(V) if c != blank and c != pad]
    seqs = [list(rng.choice(toks[:5 + (i % 5)], rng.integers(1, 7))) for i in range(n)]
    return NGramLM.from_token_ids(seqs, V, blank, pad, order=order), seqs


@pytest.mark.parametrize("order", [1, 2, 3])
def test_estimated_model_normalises_exactly(order):
    lm, _ = _model(order=order)
    S = lm.scorable() + [lm.eos]
    ctxs = {k[:-1] for k in lm.exact if len(k) > 1} | {()}
    ctxs |= {(11, 11), (lm.bos, 11), (10, 11)}               # three unseen contexts
    assert not {(11, 11), (lm.bos, 11), (10, 11)} & {k for k in lm.exact}
    for h in sorted(ctxs):
        exact = sum(math.exp(lm.logp(h, w, exact=True)) for w in S)
        assert abs(exact - 1.0) < 1e-9, (h, exact)
        table = sum(math.exp(lm.logp(h, w)) for w in S)      # the fp32 table values
        assert abs(table - 1.0) < len(S) * 2.0 ** -24, (h, table)


def test_context_that_saw_everything_takes_no_discount():
    V, blank, pad = 4, 0, 1                                  # S = {2, 3, </s>}
    seqs = [[2, 2], [2, 3], [2], [3]]                        # context (2) is followed by 2, 3 and </s>
    lm = NGramLM.from_token_ids(seqs, V, blank, pad, order=2)
    c = {2: 1, 3: 1, lm.eos: 2}                              # successors of 2: (2,2) (2,3) (2,</s>) x2 (from [2,2], [2])
    for w, n in c.items():
        assert abs(lm.logp((2,), w, exact=True) - math.log(n / 4.0)) < 1e-12          # (c - 0) / c(h): D = 0
    assert lm.exact[(2,)][1] < -200.0                        # its back-off mass is zero
    assert abs(sum(math.exp(lm.logp((2,), w, exact=True)) for w in c) - 1.0) < 1e-12
    # context (3) saw only </s> twice... and 3 never: discounted, the rest backs off
    assert abs(lm.logp((3,), lm.eos, exact=True) - math.log((2 - 0.75) / 2.0)) < 1e-12


def _ulp_apart(a, b):
    ia, ib = (np.array([v], np.float32).view(np.int32)[0] for v in (a, b))
    return abs(int(ia) - int(ib))


def test_arpa_round_trip_within_one_ulp():
    words = ["<blank>", "<pad>"] + [f"w{i}" for i in range(10)]
    vocab = Vocab(words)
    lm, _ = _model()
    back = NGramLM.from_arpa(lm.to_arpa(vocab), vocab)
    assert back.order == lm.order and set(back.table32) == set(lm.table32)
    for k, (lp, bo) in lm.table32.items():
        assert _ulp_apart(lp, back.table32[k][0]) <= 1 and _ulp_apart(bo, back.table32[k][1]) <= 1, k


# ---------------------------------------------------------------------------------------------- the packed table
def _home(key, seed, mask):
    """The kernel's hash, restated on numpy uint64 (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = (np.uint64(key) ^ np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(32))) * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(29))
    return int(z) & mask


def _probe(t, ids):
    """The kernel's lookup of a bigram / trigram -> (logp, backoff) or None; its distance from home as third."""
    keys = t["table"].numpy().view(np.uint64)[:, 0]
    vals = t["table"].numpy().view(np.float32)[:, 2:]
    key = len(ids) << 45
    for sh, x in zip((30, 15, 0)[3 - len(ids):], ids):
        key |= min(max(int(x), 0), t["V"] + 1) << sh
    h = _home(key, t["seed"], t["mask"])
    for d in range(t["probe"]):
        s = (h + d) & t["mask"]
        if int(keys[s]) == key:
            return float(vals[s, 0]), float(vals[s, 1]), d
    return None


def _table_logp(t, order, ctx, w):
    """The kernel's lm_score on the packed tables, in fp64."""
    uni = t["uni"].numpy()
    ctx = tuple(ctx)[-(order - 1):] if order > 1 else ()
    u, v = (ctx[0], ctx[1]) if len(ctx) == 2 else (-1, ctx[0] if ctx else -1)
    bo2 = bo1 = 0.0
    if order >= 2 and v >= 0:
        bo1 = float(uni[v, 1])
    if order >= 3 and u >= 0:
        d = _probe(t, (u, v))
        bo2 = d[1] if d else 0.0
        tri = _probe(t, (u, v, w))
        if tri:
            return tri[0]
    if order >= 2 and v >= 0:
        bi = _probe(t, (v, w))
        if bi:
            return bo2 + bi[0]
    return bo2 + bo1 + float(uni[w, 0])


def test_packed_table_equals_logp_for_every_query():
    lm, _ = _model(seed=3)
    t = lm.device_tables("cpu")
    assert t is lm.device_tables("cpu")                      # cached
    cap = t["mask"] + 1
    assert cap & t["mask"] == 0 and 1 <= t["probe"] <= 4 and t["table"].shape == (cap, 2) and t["uni"].shape == (14, 2)
    S = lm.scorable() + [lm.eos]
    ids = lm.scorable() + [lm.bos]
    ctxs = [(lm.bos,)] + [(u, v) for u in ids for v in lm.scorable()]
    for h in ctxs:
        for w in S:
            assert _table_logp(t, lm.order, h, w) == lm.logp(h, w), (h, w)
    for order in (1, 2):
        lo, _ = _model(seed=3, order=order)
        tl = lo.device_tables("cpu")
        for h in ctxs[:40]:
            for w in S:
                assert _table_logp(tl, order, h, w) == lo.logp(h, w), (order, h, w)


def test_packed_table_every_key_within_probe_of_home():
    from tests.ctc_beam_lm_ref import SPARSE, random_lm
    lm = random_lm(**SPARSE["lm"])
    grams = [k for k in lm.table32 if len(k) > 1]
    assert len(grams) >= 2000
    t = lm.device_tables("cpu")
    dist = []
    for k in grams:
        hit = _probe(t, k)
        assert hit is not None and hit[:2] == lm.table32[k], k
        dist.append(hit[2])
    assert max(dist) == t["probe"] - 1 and t["probe"] <= 4   # the probe length is the one the table needs
    assert t["probe"] >= 2                                   # collisions are exercised


def test_from_sentences_parses_through_the_vocabulary():
    vocab = Vocab(["<blank>", "<pad>", "<unk>", "yes", "no", "up"])
    sents = ["yes no", "no up up", "yes", "zebra no"]            # zebra -> <unk>
    lm = NGramLM.from_sentences(sents, vocab, order=2)
    want = NGramLM.from_token_ids([vocab.parse(s) for s in sents], len(vocab), vocab.blank_idx, vocab.pad_idx, order=2)
    assert lm.exact == want.exact and lm.order == 2 and lm.has_eos
    assert (vocab.stoi["<unk>"], vocab.stoi["no"]) in lm.exact
    # yes is followed by no once and by </s> once: (1 - D) / 2
    assert abs(lm.logp((vocab.stoi["yes"],), vocab.stoi["no"], exact=True) - math.log(0.25 / 2.0)) < 1e-12


def test_hparams_decoder_lm_defaults_and_setter():
    from nn_conformer_for_speech_recognition_amd.lib.hparams import HParams
    hp = HParams(None)
    assert hp.decoder_lm is None and hp.lm_weight == 0.0 and hp.word_bonus == 0.0 and hp.token_beam == 0
    assert hp.lm is False                                      # the reference's flag ("train the transformer LM") is untouched
    lm, _ = _model()
    hp.set_decoder_lm(lm, 0.5, word_bonus=0.1, token_beam=8)
    assert hp.decoder_lm is lm and (hp.lm_weight, hp.word_bonus, hp.token_beam) == (0.5, 0.1, 8)
    hp.set_decoder_lm(None)
    assert hp.decoder_lm is None and hp.lm_weight == 0.0
