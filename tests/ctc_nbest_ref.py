"""fp64 restatement of the n-best CTC likelihood and the expected risk over it (csrc/ctc_nbest.hip,
ctc.nbest_log_likelihood / expected_risk_loss / mwer_loss), in torch on the CPU, and the cases the GPU tests run.

Per utterance b with frames x_b (T_b, V), hypotheses y_1..N (None: missing) and risks r:
  ll[n]  = log P_ctc(y_n | x_b)  (torch.nn.functional.ctc_loss, reduction='none', negated); -inf where infeasible
           (T_b < L + adjacent equal labels), missing, or longer than max_labels; T_b == 0 with L == 0: 0
  live   = ll finite;  post = softmax of ll over the live n (0 elsewhere);  rbar = mean of r over the live n
  loss   = sum_n post (r - rbar), 0 with fewer than two live hypotheses
  c      = post ((r - rbar) - loss)
  d loss / d x = sum_n c_n occ_n   (no softmax term: it is multiplied by sum_n c = 0)
expected_risk computes the gradient by autograd THROUGH the log-softmax and the CTC loss; occupancy / grad_from_occ
restate the closed form from explicit alpha / beta tables; brute_force_ll enumerates all V^T labellings.
tests/test_ctc_nbest_ref_cpu.py pins the three against each other."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

NEG_INF = float("-inf")


def repeats(h):
    return sum(1 for a, b in zip(h, h[1:]) if a == b)


def feasible(T, h):
    return T >= len(h) + repeats(h)


def ext_labels(h, blank):
    e = [blank] * (2 * len(h) + 1)
    e[1::2] = h
    return e


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _ll(lp, h, blank):
    """log P_ctc(h | lp) as a torch scalar on lp's graph (lp (T, V) log-probabilities); None where infeasible."""
    T = lp.shape[0]
    if not feasible(T, h):
        return None
    if T == 0:
        return lp.new_zeros(())
    tg = torch.tensor([h], dtype=torch.long).reshape(1, len(h))
    return -F.ctc_loss(lp[:, None, :], tg, torch.tensor([T]), torch.tensor([len(h)]), blank=blank,
                       reduction="none")[0]


def expected_risk(x, hyps, risk, blank=0, max_labels=None, dtype=torch.float64):
    """One utterance: x (T_b, V) array of logits, hyps a list of label lists (None: missing), risk a list of numbers.
    -> dict(ll (N,), post (N,), loss, c (N,), grad (T_b, V)) as float64 numpy, computed in `dtype`."""
    xt = torch.tensor(np.asarray(x), dtype=dtype).requires_grad_()
    lp = F.log_softmax(xt, -1)
    N = len(hyps)
    lls = [None if (h is None or (max_labels is not None and len(h) > max_labels)) else _ll(lp, list(h), blank)
           for h in hyps]
    lls = [None if (l is None or not math.isfinite(float(l.detach()))) else l for l in lls]
    live = [n for n in range(N) if lls[n] is not None]
    ll = np.full(N, NEG_INF)
    post = np.zeros(N)
    c = np.zeros(N)
    grad = np.zeros(tuple(xt.shape))
    loss = 0.0
    for n in live:
        ll[n] = float(lls[n].detach())
    if live:
        p = torch.softmax(torch.stack([lls[n] for n in live]), 0)
        r = torch.tensor([float(risk[n]) for n in live], dtype=dtype)
        d = r - r.mean()
        post[live] = p.detach().double().numpy()
        if len(live) >= 2:
            lt = (p * d).sum()
            loss = float(lt.detach())
            c[live] = (p * (d - lt)).detach().double().numpy()
            if xt.numel():
                lt.backward()
                grad = xt.grad.double().numpy()
    return dict(ll=ll, post=post, loss=loss, c=c, grad=grad)


def reference(x, ils, hyps, risks, blank=0, max_labels=None, dtype=torch.float64):
    """A batch: x (B, T, V), ils (B,), hyps[b][n], risks[b][n] -> ll, post (B, N), loss (B,), c (B, N), grad (B, T, V)
    (zero at t >= ils[b]); the gradient is of sum_b loss[b]."""
    B, T, V = x.shape
    N = len(hyps[0])
    out = dict(ll=np.zeros((B, N)), post=np.zeros((B, N)), loss=np.zeros(B), c=np.zeros((B, N)),
               grad=np.zeros((B, T, V)))
    for b in range(B):
        r = expected_risk(x[b, :ils[b]], hyps[b], risks[b], blank, max_labels, dtype)
        out["ll"][b], out["post"][b], out["loss"][b], out["c"][b] = r["ll"], r["post"], r["loss"], r["c"]
        out["grad"][b, :ils[b]] = r["grad"]
    return out


def alpha_beta(lp, h, blank):
    """Explicit log-space tables (T, S) in fp64 and ll; lp (T, V) log-probabilities, T >= 1, h feasible."""
    e = ext_labels(h, blank)
    T, S = lp.shape[0], len(e)
    em = lp[:, e]
    skip = np.array([s >= 2 and s % 2 == 1 and e[s] != e[s - 2] for s in range(S)])
    a = np.full((T, S), NEG_INF)
    a[0, :min(S, 2)] = em[0, :min(S, 2)]
    pad = np.full(2, NEG_INF)
    for t in range(1, T):
        p = np.concatenate([pad, a[t - 1]])
        a[t] = np.logaddexp(np.logaddexp(p[2:], p[1:-1]), np.where(skip, p[:-2], NEG_INF)) + em[t]
    bt = np.full((T, S), NEG_INF)
    bt[T - 1, max(S - 2, 0):] = em[T - 1, max(S - 2, 0):]
    skipf = np.array([s % 2 == 1 and s + 2 < S and e[s] != e[s + 2] for s in range(S)])
    for t in range(T - 2, -1, -1):
        p = np.concatenate([bt[t + 1], pad])
        bt[t] = np.logaddexp(np.logaddexp(p[:-2], p[1:-1]), np.where(skipf, p[2:], NEG_INF)) + em[t]
    ll = np.logaddexp(a[T - 1, S - 1], a[T - 1, S - 2]) if S >= 2 else a[T - 1, 0]
    return a, bt, em, ll


def occupancy(lp, h, blank):
    """occ[t, v]: the posterior probability that h's alignment emits class v at frame t (rows sum to 1)."""
    a, bt, em, ll = alpha_beta(lp, h, blank)
    e = ext_labels(h, blank)
    with np.errstate(invalid="ignore"):
        g = np.where(np.isfinite(a) & np.isfinite(bt), np.exp(a + bt - em - ll), 0.0)
    occ = np.zeros(lp.shape)
    for s, v in enumerate(e):
        occ[:, v] += g[:, s]
    return occ


def grad_from_occ(x, hyps, c, blank=0):
    """sum_n c[n] occ_n of one utterance (x (T_b, V) logits): the closed form without the softmax term."""
    lp = log_softmax(x)
    g = np.zeros(lp.shape)
    for h, cn in zip(hyps, c):
        if cn != 0.0:
            g += cn * occupancy(lp, list(h), blank)
    return g


def brute_force_ll(lp, h, blank):
    """log of the summed probability of all V^T labellings that collapse (merge repeats, drop blanks) to h."""
    T, V = lp.shape
    total = 0.0
    for path in itertools.product(range(V), repeat=T):
        out, prev = [], None
        for k in path:
            if k != prev and k != blank:
                out.append(k)
            prev = k
        if out == list(h):
            total += math.exp(sum(lp[t, k] for t, k in enumerate(path)))
    return math.log(total) if total > 0 else NEG_INF


# ----------------------------------------------------------------------------- the GPU cases
def _rand_hyp(rng, L, V, blank=0, rep=0.0):
    """L labels among the first 64 non-blank classes; adjacent labels are equal with probability `rep` and never by
    accident (V == 2 has one label: every neighbour repeats)."""
    pool = [v for v in range(V) if v != blank][:64]
    h = []
    for _ in range(L):
        if h and (rng.random() < rep or len(pool) == 1):
            h.append(h[-1])
        else:
            h.append(int(rng.choice([v for v in pool if not h or v != h[-1]])))
    return h


def _nbest(rng, L, V, N, rep=0.0):
    """An n-best list as a beam gives it: a hypothesis of L labels and N - 1 variants with one or two labels
    substituted, so that the likelihoods are close enough for every hypothesis to carry weight."""
    base = _rand_hyp(rng, L, V, rep=rep)
    pool = [v for v in range(V) if v != 0][:64]
    out = [base]
    while len(out) < N:
        h = list(base)
        for u in rng.choice(L, size=min(L, 1 + len(out) % 2), replace=False):
            near = {h[u - 1] if u > 0 else -1, h[u + 1] if u + 1 < L else -1, h[u]}
            free = [v for v in pool if v not in near]
            if free:
                h[u] = int(rng.choice(free))
        out.append(h)
    return out


def _case(seed, B, T, V, ils, hyps, risks=None, blank=0, max_labels=None, scale=1.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    if risks is None:
        risks = [[float(rng.integers(0, 6)) for _ in hb] for hb in hyps]
        for rb in risks:                      # never all equal by accident
            rb[0], rb[-1] = 0.0, 3.0
    return dict(x=x, ils=list(ils), hyps=hyps, risks=risks, blank=blank, max_labels=max_labels)


def _build_cases():
    r = np.random.default_rng(5)
    C = {}
    C["ragged_T_0_and_1"] = _case(1, 4, 12, 6, [12, 7, 1, 0], [
        [_rand_hyp(r, 4, 6), _rand_hyp(r, 2, 6), []],
        [_rand_hyp(r, 3, 6), _rand_hyp(r, 7, 6), _rand_hyp(r, 1, 6)],
        [[], [2], [3]],
        [[], [], [1]]])
    C["V2"] = _case(2, 2, 10, 2, [10, 9], [[[1], [1, 1]], [[], [1, 1, 1]]])
    C["V1024_N5"] = _case(3, 2, 20, 1024, [20, 13], [_nbest(r, 8, 1024, 4, rep=0.2) + [[]],
                                                     _nbest(r, 5, 1024, 4, rep=0.2) + [[7]]])
    nb = _nbest(r, 9, 12, 15, rep=0.2)
    C["N16_missing_identical"] = _case(4, 2, 24, 12, [24, 20], [
        [nb[0], list(nb[0])] + [None if n % 5 == 4 else nb[n + 1] for n in range(14)],
        [None] * 13 + [nb[3][:4], None, nb[4][:4]]])
    C["S63_one_wave"] = _case(5, 1, 40, 8, [40], [_nbest(r, 31, 8, 2) + [[]]], max_labels=31)
    C["S65_lds"] = _case(6, 1, 40, 8, [40], [_nbest(r, 32, 8, 2) + [[]]], max_labels=32)
    C["wave_boundaries"] = _case(7, 4, 140, 16, [140] * 4, [_nbest(r, L, 16, 2) for L in (63, 64, 100, 129)],
                                 max_labels=129)
    h511 = _rand_hyp(r, 511, 8)
    C["L511_T520"] = _case(8, 1, 520, 8, [520], [[h511, h511[:510]]], max_labels=511)
    C["prefetch_block"] = _case(9, 4, 33, 7, [15, 16, 17, 33], [_nbest(r, 5, 7, 2, rep=0.3) for _ in range(4)])
    rep = [1, 1, 2, 2, 2]                      # 5 labels, 3 repeats: exactly one alignment at T_b = 8
    C["repeats_exact_and_infeasible"] = _case(10, 2, 8, 5, [8, 7], [[rep, [1, 2, 1], [3]], [rep, [1, 2, 1], [3]]])
    C["over_max_labels"] = _case(11, 2, 14, 9, [14, 11], [[[1, 2, 3], [4, 5, 6, 7, 8], [2, 2], None],
                                                          [[1, 2, 3, 4, 5], [3, 1], [3, 1], [6]]], max_labels=3)
    return C


CASES = _build_cases()


def pad_hyps(hyps, width=None, fill=-1):
    """(ids (B, N, L) int64 padded with `fill`, lengths (B, N) int64 with -1 for a missing hypothesis)."""
    L = max([len(h) for hb in hyps for h in hb if h is not None] + [1])
    L = max(L, width or 0)
    ids = [[(list(h) if h is not None else []) + [fill] * (L - (len(h) if h is not None else 0)) for h in hb]
           for hb in hyps]
    lens = [[-1 if h is None else len(h) for h in hb] for hb in hyps]
    return torch.tensor(ids, dtype=torch.int64), torch.tensor(lens, dtype=torch.int64)
