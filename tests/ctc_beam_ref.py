"""fp64 restatement of CTC prefix beam search without a language model (test infrastructure; csrc/ctc_beam.hip,
ctc.beam_search_decode), never calling the library.

A beam entry is a label prefix l with p_b(l), p_nb(l): the log-probabilities of its kept alignments ending in blank
and in non-blank.  Start: the empty prefix, p_b = 0, p_nb = -inf.  Per frame with log-probabilities r:
  stay     p_b'(l) (+)= (p_b (+) p_nb)(l) + r[blank];  p_nb'(l) (+)= p_nb(l) + r[last(l)]  (l non-empty)
  extend   p_nb'(l+c) (+)= r[c] + (c == last(l) ? p_b(l) : (p_b (+) p_nb)(l))   for every c not in {blank, pad}
((+) = log-sum-exp; candidates are identified by prefix content, so an extension that is itself in the beam lands on
that entry); the W candidates of highest p_b (+) p_nb survive, in descending order.

* full_search     every candidate enumerated; also reports the smallest score gap at any beam cut and between the
                  returned hypotheses (a free-running comparison is only meaningful where that gap is large);
* pruned_search   the kernel's candidate set: the W + 1 best tokens of the frame and, with 0-based beam rank a and
                  token rank b, the pairs (a + 1) * b <= W (tight=True: the insufficient (a + 1)(b + 1) <= W on W
                  tokens), merges taken over all tokens;
* ctc_loglik      log p(labels | x) by the alpha recursion;
* replay          follows a device back-pointer table frame by frame in fp64 and checks every choice it made."""
import numpy as np

NEG = -np.inf

# the free-running end-to-end case (tests/test_gpu_ctc_beam.py; pinned decidable by tests/test_ctc_beam_ref_cpu.py)
E2E = dict(seed=1, B=32, T=32, V=5, W=4, nbest=2, scale=2.0, min_gap=1e-3)


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def make_logits(seed, B, T, V, scale, blank=0):
    """The tests' inputs: scale * randn with the blank column raised by scale (fp32 values, seeded)."""
    x = np.random.default_rng(seed).standard_normal((B, T, V)) * scale
    x[..., blank] += scale
    return x.astype(np.float32)


def _frame(beam, r, blank, pad):
    """Candidates of one frame.  beam: [(prefix, p_b, p_nb)] -> (spb, spnb) of the n stays and ext (n, V): p_nb of
    prefix + c (-inf: not a candidate -- blank, pad, or merged into the stay of a live entry)."""
    n = len(beam)
    where = {p: i for i, (p, _, _) in enumerate(beam)}
    assert len(where) == n, "a prefix is held twice"
    pb = np.array([e[1] for e in beam], np.float64)
    pnb = np.array([e[2] for e in beam], np.float64)
    tot = np.logaddexp(pb, pnb)
    spb = tot + r[blank]
    spnb = np.full(n, NEG)
    ext = tot[:, None] + r[None, :]
    for i, (p, _, _) in enumerate(beam):
        if p:
            spnb[i] = pnb[i] + r[p[-1]]
            ext[i, p[-1]] = pb[i] + r[p[-1]]
    ext[:, blank] = NEG
    if pad >= 0:
        ext[:, pad] = NEG
    for k, (p, _, _) in enumerate(beam):
        if p and p[:-1] in where:
            i = where[p[:-1]]
            spnb[k] = np.logaddexp(spnb[k], ext[i, p[-1]])
            ext[i, p[-1]] = NEG
    return spb, spnb, ext


def _select(beam, spb, spnb, ext, W, keep=None):
    """The W best candidates (stable order: stays first, then extensions by (beam, token)) -> (new beam, gap at the
    cut: score of the last kept minus the best excluded, inf if nothing finite is excluded).  keep: optional (n, V)
    mask of the extensions that may be chosen (the pruned rule)."""
    n, V = ext.shape
    e = ext if keep is None else np.where(keep, ext, NEG)
    allc = np.concatenate([np.logaddexp(spb, spnb), e.ravel()])
    order = np.argsort(-allc, kind="stable")
    order = order[np.isfinite(allc[order])]
    new = []
    for c in order[:W]:
        if c < n:
            new.append((beam[c][0], spb[c], spnb[c]))
        else:
            i, tok = divmod(int(c) - n, V)
            new.append((beam[i][0] + (tok,), NEG, e[i, tok]))
    gap = allc[order[W - 1]] - allc[order[W]] if len(order) > W else np.inf
    return new, gap


def _hyps(beam, nbest):
    return [(p, float(np.logaddexp(a, c))) for p, a, c in beam[:nbest]]


def full_search(lp, W, blank=0, pad=-1, nbest=1):
    """lp (T, V) fp64 log-probabilities -> ([(prefix, score)] best first, smallest gap)."""
    beam = [((), 0.0, NEG)]
    gap = np.inf
    for r in np.asarray(lp, np.float64):
        spb, spnb, ext = _frame(beam, r, blank, pad)
        beam, g = _select(beam, spb, spnb, ext, W)
        gap = min(gap, g)
    out = _hyps(beam, nbest)
    for a, c in zip(out, out[1:]):
        gap = min(gap, a[1] - c[1])
    return out, float(gap)


def pruned_search(lp, W, blank=0, pad=-1, nbest=1, tight=False):
    """The kernel's pruned candidate set in fp64 -> [(prefix, score)] best first."""
    beam = [((), 0.0, NEG)]
    for r in np.asarray(lp, np.float64):
        V = len(r)
        spb, spnb, ext = _frame(beam, r, blank, pad)
        ok = [c for c in range(V) if c != blank and c != pad]
        ranked = sorted(ok, key=lambda c: (-r[c], c))[:W if tight else W + 1]
        keep = np.zeros(ext.shape, bool)
        for a in range(len(beam)):
            for b, c in enumerate(ranked):
                if ((a + 1) * (b + 1) <= W) if tight else ((a + 1) * b <= W):
                    keep[a, c] = True
        beam, _ = _select(beam, spb, spnb, ext, W, keep)
    return _hyps(beam, nbest)


def ctc_loglik(lp, labels, blank=0):
    """log p(labels | lp) over all alignments (alpha recursion, fp64); lp (T, V)."""
    lp = np.asarray(lp, np.float64)
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    S = len(ext)
    alpha = np.full(S, NEG)
    alpha[0] = lp[0, blank]
    if S > 1:
        alpha[1] = lp[0, ext[1]]
    for t in range(1, len(lp)):
        new = np.full(S, NEG)
        for s in range(S):
            a = alpha[s]
            if s >= 1:
                a = np.logaddexp(a, alpha[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                a = np.logaddexp(a, alpha[s - 2])
            new[s] = a + lp[t, ext[s]]
        alpha = new
    return float(np.logaddexp(alpha[-1], alpha[-2]) if S > 1 else alpha[-1])


def roundoff_eps(T, max_abs_score):
    """Four fp32 roundings per frame on a score path: 4 T 2^-24 max(1, max |score|)."""
    return 4.0 * T * 2.0 ** -24 * max(1.0, max_abs_score)


def replay(lp, bp_parent, bp_token, W, blank=0, pad=-1, T_eps=None):
    """Follow the device's choices frame by frame.  lp (Tb, V) fp64 log-probabilities of the utterance's valid frames;
    bp_parent / bp_token (>= Tb, W) int.  From the fp64 state of the device's previous beam every candidate is
    enumerated; the device's slots must name distinct prefixes that are all candidates, in descending order, with the
    smallest kept score >= the largest excluded score - eps; the device's set is then adopted with fp64 scores.
    Returns ([(prefix, score)] per non-empty slot of the last frame, eps, {"order", "cut"}: the largest violations
    seen, both <= eps).  T_eps: the T of eps (default: the utterance's frames)."""
    lp = np.asarray(lp, np.float64)
    Tb, V = lp.shape
    beam = [((), 0.0, NEG)]
    worst_cut = worst_order = 0.0
    max_abs = 0.0
    for t in range(Tb):
        spb, spnb, ext = _frame(beam, lp[t], blank, pad)
        n = len(beam)
        stay_tot = np.logaddexp(spb, spnb)
        new, seen, scores = [], set(), []
        took_stay = np.zeros(n, bool)
        took_ext = np.zeros(ext.shape, bool)
        ended = False
        for s in range(W):
            par, tok = int(bp_parent[t, s]), int(bp_token[t, s])
            if par == -1:
                ended = True
                assert tok == -1, f"frame {t} slot {s}: an empty slot carries a token"
                continue
            assert not ended, f"frame {t} slot {s}: a filled slot after an empty one"
            assert 0 <= par < n, f"frame {t} slot {s}: parent {par} is not a slot of frame {t - 1}"
            if tok == -1:
                assert not took_stay[par], f"frame {t} slot {s}: prefix held twice"
                took_stay[par] = True
                entry, sc = (beam[par][0], spb[par], spnb[par]), stay_tot[par]
            else:
                assert 0 <= tok < V and tok != blank and tok != pad, f"frame {t} slot {s}: token {tok} not allowed"
                assert np.isfinite(ext[par, tok]) or not np.isfinite(lp[t, tok]), \
                    f"frame {t} slot {s}: extension ({par}, {tok}) is no candidate (it merges into a live entry)"
                assert not took_ext[par, tok], f"frame {t} slot {s}: prefix held twice"
                took_ext[par, tok] = True
                entry, sc = (beam[par][0] + (tok,), NEG, ext[par, tok]), ext[par, tok]
            assert entry[0] not in seen, f"frame {t} slot {s}: prefix held twice"
            seen.add(entry[0])
            if scores:
                worst_order = max(worst_order, sc - scores[-1])
            new.append(entry)
            scores.append(sc)
        assert new, f"frame {t}: the beam is empty"
        rest = np.concatenate([np.where(took_stay, NEG, stay_tot), np.where(took_ext, NEG, ext).ravel()])
        excluded = rest.max()
        if len(new) < W:
            assert not np.isfinite(excluded), f"frame {t}: {W - len(new)} empty slots while candidates were left out"
        elif np.isfinite(excluded):
            worst_cut = max(worst_cut, excluded - min(scores))
        max_abs = max(max_abs, float(np.max(np.abs(scores))))
        beam = new
    eps = roundoff_eps(Tb if T_eps is None else T_eps, max_abs)
    assert worst_order <= eps, f"slots out of order by {worst_order:.3e} > eps {eps:.3e}"
    assert worst_cut <= eps, f"a left-out candidate beats a kept one by {worst_cut:.3e} > eps {eps:.3e}"
    return _hyps(beam, len(beam)), eps, {"order": worst_order, "cut": worst_cut}
