"""CPU restatements of the RNN-T loss (csrc/rnnt.hip, transducer.rnnt_loss), the yardsticks of tests/test_gpu_rnnt.py:

  ll_autograd       fp64 torch: ll by an explicit alpha recursion, the gradient of -ll by autograd
  brute_force_ll    the log-sum over EVERY monotone path of the lattice (tiny lattices)
  tables            explicit alpha / beta tables in a chosen dtype (numpy)
  closed_form_grad  the gradient from those tables: softmax gamma - the two path weights
  reference         ll and the closed-form gradient of a batch in fp64, or -- the same formula -- in fp32

With T_b, U_b the lengths, lp = log_softmax(x), b(t,u) = lp[t,u,blank], y(t,u) = lp[t,u,label_{u+1}]:
  alpha(0,0) = 0; alpha(t,u) = lse(alpha(t-1,u) + b(t-1,u), alpha(t,u-1) + y(t,u-1))
  beta(T-1,U) = b(T-1,U); beta(t,u) = lse(beta(t+1,u) + b(t,u), beta(t,u+1) + y(t,u));  ll = beta(0,0)
tests/test_rnnt_ref_cpu.py pins them against each other."""
import itertools

import numpy as np
import torch


def log_softmax_np(x, dtype):
    x = x.astype(dtype)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=dtype))


def emissions(lp, labels, blank):
    """(b (T, U+1), y (T, U)) of one utterance's log-probabilities lp (T, U+1, V)."""
    U = len(labels)
    b = lp[:, :, blank]
    y = np.stack([lp[:, u, labels[u]] for u in range(U)], 1) if U else np.zeros((lp.shape[0], 0), lp.dtype)
    return b, y


def tables(b, y):
    """alpha, beta (T, U+1) and ll of one utterance in b's dtype."""
    T, U1 = b.shape
    ninf = b.dtype.type(-np.inf)
    alpha = np.full((T, U1), ninf, b.dtype)
    beta = np.full((T, U1), ninf, b.dtype)
    alpha[0, 0] = 0
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            up = alpha[t - 1, u] + b[t - 1, u] if t > 0 else ninf
            left = alpha[t, u - 1] + y[t, u - 1] if u > 0 else ninf
            alpha[t, u] = np.logaddexp(up, left)
    beta[T - 1, U1 - 1] = b[T - 1, U1 - 1]
    for t in range(T - 1, -1, -1):
        for u in range(U1 - 1, -1, -1):
            if t == T - 1 and u == U1 - 1:
                continue
            down = beta[t + 1, u] + b[t, u] if t + 1 < T else ninf
            right = beta[t, u + 1] + y[t, u] if u + 1 < U1 else ninf
            beta[t, u] = np.logaddexp(down, right)
    return alpha, beta, alpha[T - 1, U1 - 1] + b[T - 1, U1 - 1]


def closed_form_grad(x, labels, blank, dtype=np.float64):
    """(ll, d(-ll)/dx (T, U+1, V)) of one utterance x (T, U+1, V) from explicit alpha / beta tables, all in dtype."""
    lp = log_softmax_np(x, dtype)
    T, U1, V = lp.shape
    b, y = emissions(lp, labels, blank)
    alpha, beta, ll = tables(b, y)
    gamma = np.exp(alpha + beta - ll)
    grad = np.exp(lp) * gamma[:, :, None]
    for t in range(T):
        for u in range(U1):
            if t + 1 < T:
                grad[t, u, blank] -= np.exp(alpha[t, u] + b[t, u] + beta[t + 1, u] - ll)
            elif u == U1 - 1:
                grad[t, u, blank] -= np.exp(alpha[t, u] + b[t, u] - ll)
            if u + 1 < U1:
                grad[t, u, labels[u]] -= np.exp(alpha[t, u] + y[t, u] + beta[t, u + 1] - ll)
    return ll, grad


def ll_autograd(x, labels, blank):
    """(ll, d(-ll)/dx) of one utterance in fp64 torch: explicit alpha recursion, gradient by autograd."""
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(xt, -1)
    T, U1, _ = lp.shape
    alpha = [[None] * U1 for _ in range(T)]
    alpha[0][0] = torch.zeros((), dtype=torch.float64)
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(alpha[t][u - 1] + lp[t, u - 1, labels[u - 1]])
            alpha[t][u] = torch.logsumexp(torch.stack(terms), 0)
    ll = alpha[T - 1][U1 - 1] + lp[T - 1, U1 - 1, blank]
    (-ll).backward()
    return float(ll.detach()), xt.grad.numpy()


def brute_force_ll(x, labels, blank):
    """log of the sum over every monotone path from (0, 0) to the final blank at (T-1, U): a path is an order of T-1
    blanks (t -> t + 1) and U labels (u -> u + 1), then the last blank."""
    lp = log_softmax_np(np.asarray(x), np.float64)
    T, U1, _ = lp.shape
    U = U1 - 1
    total = []
    for label_steps in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        s = 0.0
        for k in range(T - 1 + U):
            if k in label_steps:
                s += lp[t, u, labels[u]]
                u += 1
            else:
                s += lp[t, u, blank]
                t += 1
        total.append(s + lp[T - 1, U, blank])
    return float(np.logaddexp.reduce(total))


def reference(x, targets, ils, tls, blank, dtype=np.float64):
    """{"ll" (B,), "grad" (B, T, U1, V)} of a batch in dtype: an utterance without frames has ll -inf and no
    gradient; the gradient is 0 outside the valid cells t < T_b, u <= U_b."""
    B, T, U1, V = x.shape
    ll = np.full(B, -np.inf, dtype)
    grad = np.zeros(x.shape, dtype)
    for i in range(B):
        Tb, Ub = ils[i], tls[i]
        if Tb == 0:
            continue
        ll[i], grad[i, :Tb, :Ub + 1] = closed_form_grad(x[i, :Tb, :Ub + 1], list(targets[i][:Ub]), blank, dtype)
    return {"ll": ll.astype(np.float64), "grad": grad.astype(np.float64)}


def _case(seed, B, T, U1, V, ils=None, tls=None, blank=0, labels=None, scale=2.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, U1, V)) * scale).astype(np.float32)
    allowed = np.array([v for v in range(V) if v != blank])
    tg = allowed[rng.integers(0, len(allowed), (B, U1 - 1))] if labels is None else np.asarray(labels)
    return dict(x=x, targets=tg.astype(np.int64).reshape(B, U1 - 1), blank=blank,
                ils=list(ils) if ils is not None else [T] * B, tls=list(tls) if tls is not None else [U1 - 1] * B)


def _ragged(n, hi, lo=0):
    """n lengths ending with hi: lo first, the rest spread between."""
    return [lo + (hi - lo) * i // max(n - 1, 1) for i in range(n)]


# name -> case.  The shape cases are named by what they exercise: U1 (1, 2: the smallest lattices; 63 / 64 / 65: the
# one-wave kernel's last lanes and the first LDS size; 256 / 257: the step to the 1024-thread block; 1024: the limit),
# T (1, 2, 3, 17: more diagonals than the prefetch chunk of 16 with any U1) and V (2: the least; 5, 37: scalar rows;
# 1024: float4 rows, four loads per lane).  Each has three utterances, the last one of full length.
CASES = {
    "U1_1_T1_V2": _case(1, 3, 1, 1, 2),
    "U1_1_T17_V5": _case(2, 3, 17, 1, 5, ils=[3, 16, 17]),
    "U1_2_T2_V37": _case(3, 3, 2, 2, 37, ils=[1, 2, 2], tls=[1, 0, 1]),
    "U1_2_T3_V1024": _case(4, 3, 3, 2, 1024, ils=[2, 3, 3], tls=[0, 1, 1]),
    "U1_9_T17_V1024": _case(5, 3, 17, 9, 1024, ils=[16, 9, 17], tls=[8, 3, 8]),
    "U1_63_T3_V5": _case(6, 3, 3, 63, 5, ils=[1, 3, 3], tls=[62, 31, 62]),
    "U1_64_T17_V5": _case(7, 3, 17, 64, 5, ils=[17, 5, 17], tls=[40, 63, 63]),
    "U1_65_T2_V37": _case(8, 3, 2, 65, 37, ils=[2, 1, 2], tls=[64, 64, 64]),
    "U1_256_T3_V5": _case(9, 3, 3, 256, 5, ils=[2, 3, 3], tls=[255, 100, 255]),
    "U1_257_T17_V2": _case(10, 3, 17, 257, 2, ils=[17, 3, 17], tls=[256, 256, 200]),
    "U1_1024_T3_V2": _case(11, 3, 3, 1024, 2, ils=[3, 1, 3], tls=[1023, 1023, 700]),
    "ragged_T_0_and_1": _case(12, 4, 6, 4, 7, ils=[0, 1, 4, 6], tls=[2, 3, 3, 1]),
    "ragged_U_0_and_Umax": _case(13, 4, 5, 6, 7, ils=[5, 3, 5, 4], tls=[0, 5, 2, 5]),
    "repeated_labels": _case(14, 3, 7, 5, 6, labels=[[2, 2, 2, 2], [1, 1, 3, 3], [4, 1, 1, 4]]),
    "blank_not_0": _case(15, 3, 5, 4, 6, blank=3, ils=[5, 4, 5], tls=[3, 2, 3]),
    "blank_last": _case(16, 3, 4, 3, 5, blank=4),
}
