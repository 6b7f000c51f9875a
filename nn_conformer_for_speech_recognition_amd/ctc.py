"""CTC head on libcfm — drop-ins for the reference's loss and decode calls.

  CTCLoss / ctc_loss   torch.nn.CTCLoss(blank=hp.blank_idx, zero_infinity=True) as built at
                       runner.py:35 and applied at runner.py:142-143 to the log-probabilities of
                       ASRNN.forward (asrnn.py:256).  Same arguments, layouts ((T, B, V) by default),
                       reductions and zero_infinity behaviour; log_softmax is fused (idempotent on
                       log-probabilities), so raw logits may be passed too.
  ctc_head_loss        the fused head of the training step: Linear(d -> V) + log_softmax + CTC as ONE
                       autograd node (no fp32 logits gradient round trip: the CTC kernel writes the
                       logits gradient in the compute dtype straight into the head's two GEMMs).
  greedy_decode        ASRNN.predict (asrnn.py:48-58, argmax) + the id filter of Vocab.decode
                       (myvocab.py:211-231: <pad>/<blank> dropped, no repeat collapse by default).
  beam_search_decode   CTC prefix beam search: the alternative to that argmax (modelled on torchaudio's CUDA
                       CTC decoder), alone or with a back-off n-gram language model (lm.NGramLM) fused in.
  forced_align         the best single alignment (Viterbi path) of a GIVEN transcript: per-frame labels and scores,
                       per-token frame spans and the path's score (modelled on torchaudio.functional.forced_align,
                       batched).  No reference counterpart; the Runner uses it for word spans (Runner.align) and for
                       the confidence filter of the pseudo-label pass (hp.nst_min_confidence).
  edit_distance        batched Levenshtein distance over token ids, optionally with the aligned pairs: the word error
                       rate of runner.py:160,230 (jiwer's wer; the vocabulary's tokens are words) without the trip
                       through strings on the host, and the pairs of the confusion matrix of evals.py:64.

Everything is stream-ordered with no host synchronisation when targets are padded (B, S) and the
lengths are device tensors, so a whole training step can be captured into one HIP graph.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

from . import ops

_RED = ("none", "mean", "sum")


def _lengths(v, B, device, limit=None, what="lengths"):
    """(B,) int32 device lengths.  Host-side lengths (lists, CPU tensors) are validated against
    `limit` as torch.nn.functional.ctc_loss does (it raises); device lengths are not read back (no
    sync) -- the kernels clamp them to the buffers' extents instead."""
    if isinstance(v, (list, tuple)):
        v = torch.tensor(v)
    if not torch.is_tensor(v):
        raise TypeError("lengths must be tensors or sequences of ints")
    if v.numel() != B:
        raise ValueError(f"expected {B} lengths, got {v.numel()}")
    if not v.is_cuda and v.numel() > 0:
        lo, hi = int(v.min()), int(v.max())
        if lo < 0:
            raise ValueError(f"{what} must be non-negative, got {lo}")
        if limit is not None and hi > limit:
            raise ValueError(f"expected {what} to have value at most {limit}, but got value {hi}")
    return v.to(device=device, dtype=torch.int32).contiguous()


def _check_blank(blank, V):
    if not 0 <= blank < V:
        raise ValueError(f"blank must be in label range [0, {V}), got {blank}")


def _prep_targets(targets, tgt_len, B, device):
    """(targets int32, ldt, offsets or None, Smax) for padded (B, S) or concatenated 1-D targets."""
    if targets.dim() == 2:
        t = targets.to(device=device, dtype=torch.int32).contiguous()
        return t, t.shape[1], None, t.shape[1]
    if targets.dim() == 1:
        t = targets.to(device=device, dtype=torch.int32).contiguous()
        off = (torch.cumsum(tgt_len, 0, dtype=torch.int32) - tgt_len).contiguous()
        smax = int(tgt_len.max().item()) if B > 0 else 0     # host sync (1-D form only)
        return t, 0, off, smax
    raise ValueError("targets must be (B, S) padded or 1-D concatenated")


def _logits(x, batch_first, who, what="logits", need_3d=False):
    """(x, B, T) of `who`'s logits argument: fp32 CUDA (RuntimeError naming `who`), optionally 3-D (ValueError), the
    class dimension made contiguous."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError(f"{who} runs on libcfm: fp32 CUDA {what} required")
    if need_3d and x.dim() != 3:
        raise ValueError("logits must be (B, T, V), or (T, B, V) with batch_first=False")
    x = x if x.stride(-1) == 1 else x.contiguous()
    B, T = (x.shape[0], x.shape[1]) if batch_first else (x.shape[1], x.shape[0])
    return x, B, T


def _problem(targets, in_len, tgt_len, B, T, device):
    """(il, tl, tg, ldt, off, smax): the lengths as _lengths gives them (host-side ones validated against T and the
    padded targets' width) and the targets as _prep_targets gives them."""
    il = _lengths(in_len, B, device, T, "input_lengths")
    tl = _lengths(tgt_len, B, device, targets.shape[1] if targets.dim() == 2 else None, "target_lengths")
    return (il, tl) + _prep_targets(targets, tl, B, device)


_NONFINITE = None


def set_nonfinite_counter(counter):
    """Bind a (1,) int32 device counter that every reduction='mean' CTC loss increments when its value is not
    finite (no host sync; e.g. a training loop's bad-step count, read once after the run).  None unbinds."""
    global _NONFINITE
    if counter is not None and (counter.dtype != torch.int32 or counter.numel() != 1 or not counter.is_cuda):
        raise ValueError("nonfinite counter: a (1,) int32 CUDA tensor")
    _NONFINITE = counter


def _reduce(nll, tl, reduction):
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    # mean_b(nll_b / max(L_b, 1)) as one launch (cfm_ctc_mean; was clamp + cast + divide + mean)
    return ops.ctc_mean(nll, tl, _NONFINITE)


class _CTCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, targets, in_len, tgt_len, blank, reduction, zero_infinity, batch_first):
        x, B, T = _logits(x, batch_first, "ctc_loss", "log-probs/logits")
        _check_blank(blank, x.shape[-1])
        il, tl, tg, ldt, off, smax = _problem(targets, in_len, tgt_len, B, T, x.device)
        nll, ws = ops.ctc_loss_fwd(x, tg, ldt, off, il, tl, smax, blank, zero_infinity, batch_first)
        ctx.save_for_backward(x, tg, off if off is not None else tg, il, tl, ws)
        ctx.cfg = (ldt, off is not None, smax, blank, zero_infinity, batch_first, reduction)
        return _reduce(nll, tl, reduction)

    @staticmethod
    def backward(ctx, g):
        x, tg, off, il, tl, ws = ctx.saved_tensors
        ldt, has_off, smax, blank, zi, bf, red = ctx.cfg
        dx = ops.ctc_loss_bwd(x, tg, ldt, off if has_off else None, il, tl, smax, blank, zi, bf, ws, g, red)
        return dx, None, None, None, None, None, None, None


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction="mean", zero_infinity=False,
             batch_first=False):
    """torch.nn.functional.ctc_loss on libcfm (log_probs (T, B, V), or (B, T, V) if batch_first)."""
    if reduction not in _RED:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    return _CTCFn.apply(log_probs, targets, input_lengths, target_lengths, int(blank), reduction,
                        bool(zero_infinity), bool(batch_first))


class CTCLoss(nn.Module):
    """torch.nn.CTCLoss(blank=0, reduction='mean', zero_infinity=False) on libcfm."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in _RED:
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ctc_loss(log_probs, targets, input_lengths, target_lengths, self.blank, self.reduction,
                        self.zero_infinity)


class _CTCHeadFn(torch.autograd.Function):
    """y (B*T, d) -> logits = y·Wᵀ + b (fp32, batch-major) -> CTC loss; backward writes the logits
    gradient in the compute dtype and runs the head's dgrad / wgrad GEMMs on it directly."""

    @staticmethod
    def forward(ctx, y, w, b, targets, in_len, tgt_len, B, T, blank, reduction, zero_infinity, cd):
        yc = y if y.dtype == cd else ops.cast(y, cd)
        wc = w if w.dtype == cd else ops.cast(w, cd)
        logits = ops.linear(yc, wc, b, out_dtype=torch.float32).view(B, T, -1)
        _check_blank(blank, w.shape[0])
        il, tl, tg, ldt, off, smax = _problem(targets, in_len, tgt_len, B, T, y.device)
        nll, ws = ops.ctc_loss_fwd(logits, tg, ldt, off, il, tl, smax, blank, zero_infinity, True)
        ctx.save_for_backward(logits, yc, wc, tg, off if off is not None else tg, il, tl, ws)
        ctx.cfg = (ldt, off is not None, smax, blank, zero_infinity, reduction, cd, y.dtype, b is not None)
        ctx.mark_non_differentiable(logits)
        ctx.set_materialize_grads(False)     # no (B, T, V) zero gradient for the logits output
        return _reduce(nll, tl, reduction), logits

    @staticmethod
    def backward(ctx, g, _glogits):
        logits, yc, wc, tg, off, il, tl, ws = ctx.saved_tensors
        ldt, has_off, smax, blank, zi, red, cd, ydt, has_b = ctx.cfg
        dl = ops.ctc_loss_bwd(logits, tg, ldt, off if has_off else None, il, tl, smax, blank, zi, True, ws, g, red,
                              grad_dtype=cd)
        dl2 = dl.view(-1, dl.shape[-1])
        dw = ops.linear_wgrad(dl2, yc)
        db = ops.colsum(dl2) if has_b else None
        dy = ops.linear_dgrad(dl2, wc, out_dtype=ydt)
        return dy, dw, db, None, None, None, None, None, None, None, None, None


def ctc_head_loss(y, weight, bias, targets, input_lengths, target_lengths, B, T, blank=0, reduction="mean",
                  zero_infinity=True, compute_dtype=torch.bfloat16):
    """Fused Linear(d -> V) + log_softmax + CTC over token-major encoder rows y (B*T, d).
    Returns (loss, logits (B, T, V) fp32 — e.g. for greedy_decode; not differentiable)."""
    if reduction not in _RED:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    return _CTCHeadFn.apply(y, weight, bias, targets, input_lengths, target_lengths, int(B), int(T), int(blank),
                            reduction, bool(zero_infinity), compute_dtype)


def greedy_decode(logits, lengths=None, blank=0, pad=-1, collapse=False, batch_first=True, compact=True):
    """ASRNN.predict + Vocab.decode's id filter on the device.
    Returns (ids (B, T) int64 = torch.argmax(logits, -1), tokens (B, T) int32 padded with -1, n (B,));
    compact=False: ids only (tokens, n are None)."""
    x, B, _ = _logits(logits, batch_first, "greedy_decode")
    ln = None if lengths is None else _lengths(lengths, B, x.device)
    return ops.ctc_greedy_decode(x, ln, blank, pad, collapse, batch_first, compact)


BEAM_MAX = 128
LM_CANDIDATES = 1024      # stays + extensions per frame of the LM search


def default_token_beam(beam_size, n_tokens):
    """min(W + 1, #tokens, 1024 // W - 1): the tokens each live entry is extended by when an LM is fused."""
    return max(1, min(beam_size + 1, n_tokens, LM_CANDIDATES // beam_size - 1))


def beam_search_decode(logits, lengths=None, beam_size=16, blank=0, pad=-1, nbest=1, batch_first=True,
                       return_trace=False, lm=None, lm_weight=0.0, word_bonus=0.0, token_beam=None, lm_eos=True):
    """CTC prefix beam search on the device (cfm_ctc_beam_decode; with `lm` cfm_ctc_beam_decode_lm).
    Returns (tokens (B, nbest, T) int32 padded with -1, lens (B, nbest) int32, scores (B, nbest) fp32 = log of
    the summed alignment probability the beam kept for each hypothesis), best first; with return_trace also
    (bp_parent, bp_token) (B, T, beam_size) int32, the back-pointer table.  `pad` (< 0: none) is never emitted.

    lm: an lm.NGramLM over the same ids (lm.V == V, the same blank and pad), fused at every extension:
    score(l + c) gains lm_weight * lm(c | context) + word_bonus; each live entry is extended by the `token_beam`
    acoustically best tokens of the frame (None: default_token_beam; beam_size * (1 + token_beam) <= 1024); the
    beam ranks on, and `scores` are, the fused scores.  lm_eos (only where the LM has </s>): the final scores add
    lm_weight * lm(</s> | context) and order the hypotheses; the back-pointer slots keep the last frame's order.
    With lm=None the other LM arguments must be at their defaults and the call is the plain search."""
    if not isinstance(beam_size, int) or isinstance(beam_size, bool) or not 1 <= beam_size <= BEAM_MAX:
        raise ValueError(f"beam_size must be an integer in [1, {BEAM_MAX}], got {beam_size!r}")
    if not isinstance(nbest, int) or isinstance(nbest, bool) or not 1 <= nbest <= beam_size:
        raise ValueError(f"nbest must be an integer in [1, beam_size], got {nbest!r}")
    x, B, _ = _logits(logits, batch_first, "beam_search_decode", need_3d=True)
    V = x.shape[-1]
    _check_blank(blank, V)
    if pad >= V:
        raise ValueError(f"pad must be in label range [0, {V}) or negative, got {pad}")
    ln = None if lengths is None else _lengths(lengths, B, x.device)
    if lm is None:
        if lm_weight != 0.0 or word_bonus != 0.0 or token_beam is not None or lm_eos is not True:
            raise ValueError("lm_weight, word_bonus, token_beam and lm_eos need an lm")
        tokens, lens, scores, bp_parent, bp_token = ops.ctc_beam_decode(x, ln, beam_size, blank, pad, nbest,
                                                                        batch_first)
    else:
        if lm.V != V:
            raise ValueError(f"the language model is over {lm.V} ids, the logits over {V}")
        if lm.blank != blank or max(lm.pad, -1) != max(pad, -1):
            raise ValueError(f"the language model's blank / pad ({lm.blank}, {lm.pad}) differ from the call's "
                             f"({blank}, {pad})")
        n_tokens = V - 1 - (1 if 0 <= pad != blank else 0)
        if token_beam is None:
            token_beam = default_token_beam(beam_size, n_tokens)
        if not isinstance(token_beam, int) or isinstance(token_beam, bool) or token_beam < 1:
            raise ValueError(f"token_beam must be a positive integer, got {token_beam!r}")
        K = min(token_beam, n_tokens)
        if K < 1 or beam_size * (1 + K) > LM_CANDIDATES or K > 768:
            raise ValueError(f"beam_size * (1 + token_beam) must be <= {LM_CANDIDATES} and token_beam <= 768, got "
                             f"beam_size {beam_size}, token_beam {K}")
        tokens, lens, scores, bp_parent, bp_token = ops.ctc_beam_decode_lm(
            x, lm.device_tables(x.device), ln, beam_size, K, lm_weight, word_bonus, bool(lm_eos) and lm.has_eos,
            blank, pad, nbest, batch_first)
    if return_trace:
        return tokens, lens, scores, (bp_parent, bp_token)
    return tokens, lens, scores


ForcedAlignment = namedtuple("ForcedAlignment", "alignments scores score starts ends token_scores")
ALIGN_MAX_LABELS = 511


def forced_align(logits, targets, input_lengths=None, target_lengths=None, blank=0, batch_first=True):
    """CTC forced alignment on the device (cfm_ctc_forced_align): the best single alignment of each utterance's
    transcript.  logits (B, T, V) fp32 CUDA (or (T, B, V) with batch_first=False), raw or log-probabilities (the
    log-softmax is fused and idempotent); targets padded (B, Smax) or 1-D concatenated, as for ctc_loss;
    input_lengths None: every utterance is T long; target_lengths None (padded targets only): Smax.  At most 511
    labels per utterance.  Host-side lengths are validated as for the loss, and host-side targets that contain
    `blank` within their (host-side) lengths raise ValueError; device lengths and targets are not read back -- the
    kernels clamp them.  Returns the named tuple
      alignments (B, T) int32     the label of each frame (blank included); -1 at and beyond the utterance's length
      scores (B, T) fp32          the frame's log-probability of that label; 0 beyond
      score (B,) fp32             the alignment's log-probability, the sum of its scores
      starts, ends (B, Smax) int32, token_scores (B, Smax) fp32   per target position: the first frame of its label,
                                  one past the last, the sum of `scores` over the span; -1 / -1 / 0 past the length
    Frames are rows of `logits` (encoder output frames).
    Tie rule: among equally good predecessors the path prefers to stay in its state, then to come from the state
    before, then to skip the blank; at the last frame the final blank wins a tie against the last label.
    Infeasible utterances (fewer frames than labels plus adjacent equal label pairs, so also no frames but labels;
    or a best path whose score is not finite): score -inf, alignments -1, scores 0, spans -1 / -1 / 0.  No frames
    and no labels: score 0.  No labels: every frame blank."""
    x, B, T = _logits(logits, batch_first, "forced_align", need_3d=True)
    blank = int(blank)
    _check_blank(blank, x.shape[-1])
    if not torch.is_tensor(targets):
        targets = torch.tensor(targets, dtype=torch.int64)
    if targets.dim() == 2 and targets.shape[0] != B:
        raise ValueError(f"expected targets for {B} utterances, got {targets.shape[0]}")
    if input_lengths is None:
        input_lengths = torch.full((B,), T, dtype=torch.int32, device=x.device)
    if target_lengths is None:
        if targets.dim() != 2:
            raise ValueError("target_lengths may be omitted only with padded (B, Smax) targets")
        target_lengths = torch.full((B,), targets.shape[1], dtype=torch.int32, device=x.device)
        host_tl = [targets.shape[1]] * B
    elif torch.is_tensor(target_lengths):
        host_tl = None if target_lengths.is_cuda else target_lengths.tolist()
    else:
        host_tl = list(target_lengths)
    il, tl, tg, ldt, off, smax = _problem(targets, input_lengths, target_lengths, B, T, x.device)
    if not targets.is_cuda and host_tl is not None:
        rows = targets.tolist()
        if targets.dim() == 2:
            bad = any(blank in r[:n] for r, n in zip(rows, host_tl))
        else:
            bad = blank in rows[:sum(host_tl)]
        if bad:
            raise ValueError(f"targets must not contain the blank index {blank}")
    if smax > ALIGN_MAX_LABELS:
        raise ValueError(f"forced_align takes at most {ALIGN_MAX_LABELS} labels per utterance, got {smax}")
    return ForcedAlignment(*ops.ctc_forced_align(x, tg, ldt, off, il, tl, smax, blank, batch_first))


EditDistance = namedtuple("EditDistance", "distance ref_lengths counts pair_ref pair_hyp n_pairs")
EDIT_MAX_LEN = 1024


def _id_rows(t, what):
    """(rows, ld): a 2-D id tensor as int32 with contiguous ids and a row stride ld >= its width (a view of `t` where
    its dtype and strides allow, so strided batches are read in place)."""
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what} must be int32 or int64 ids, got {t.dtype}")
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    n, w = t.shape
    if n <= 1 or w == 0:
        return t.contiguous(), w
    if t.stride(1) != 1 or t.stride(0) < w:
        t = t.contiguous()
    return t, t.stride(0)


def edit_distance(hyp, ref, hyp_lengths=None, ref_lengths=None, ops=False):
    """Batched edit distance (Levenshtein) over token ids on the device (cfm_edit_distance).  The vocabulary's tokens
    are words, so this is the word-level distance of jiwer's wer (runner.py:160,230).

    hyp (B, Lh), or (B, N, Lh) for an n-best list per reference (group = N from the shape: results are (B, N));
    ref (B, Lr); int32 or int64 CUDA tensors, rows may be strided (CPU tensors raise).  Lengths: device tensors, host
    lists or None (the full row), hyp_lengths shaped like hyp without its last dimension; they are clamped to
    [0, Lh] / [0, Lr] on the device and device lengths are never read back (no .item() / .tolist(): no host
    synchronisation).  Lh, Lr <= 1024.  Ids past a row's length are never read into a result.

    With r one reference (R ids) and h one hypothesis (H ids):
      D[i][0] = i, D[0][j] = j,
      D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)   for i, j >= 1,
      distance = D[R][H].
    ops=True adds ONE alignment, under this tie rule: a cell's direction is the first of diagonal (hit or
    substitution), up (deletion: a reference token without a partner), left (insertion) that attains the minimum; on
    the border i == 0 walks left and j == 0 walks up; the backtrace starts at (R, H).

    Returns the named tuple (all int32)
      distance (B,) / (B, N)
      ref_lengths (B,)               the clamped reference lengths (the denominator of a WER)
      counts (..., 4)                hits, substitutions, deletions, insertions of that path:
                                     hits + subs + dels = R, hits + subs + ins = H, subs + dels + ins = distance
      pair_ref, pair_hyp (..., Lr + Lh), n_pairs (...)   the path's pairs in forward order, -1 on the gap side,
                                     n_pairs <= R + H of them; entries past n_pairs are -1 on both sides
    counts, pair_ref, pair_hyp and n_pairs are None with ops=False (one launch, no direction matrix is stored)."""
    want_ops = bool(ops)
    from . import ops as _ops     # (the `ops` argument shadows the module here)
    if not torch.is_tensor(hyp) or not torch.is_tensor(ref) or not hyp.is_cuda or not ref.is_cuda:
        raise RuntimeError("edit_distance runs on libcfm: CUDA id tensors required")
    if ref.dim() != 2 or hyp.dim() not in (2, 3):
        raise ValueError("ref must be (B, Lr) and hyp (B, Lh) or (B, N, Lh)")
    B, Lr = ref.shape
    if hyp.shape[0] != B:
        raise ValueError(f"expected hypotheses for {B} references, got {hyp.shape[0]}")
    lead = tuple(hyp.shape[:-1])
    group = hyp.shape[1] if hyp.dim() == 3 else 1
    Lh = hyp.shape[-1]
    if Lr > EDIT_MAX_LEN or Lh > EDIT_MAX_LEN:
        raise ValueError(f"edit_distance takes at most {EDIT_MAX_LEN} ids per row, got Lr {Lr}, Lh {Lh}")
    if hyp.dim() == 3 and group == 0:
        raise ValueError("hyp (B, N, Lh) needs N >= 1")
    P = B * group
    dev = ref.device
    r2, ldr = _id_rows(ref, "ref")
    h2, ldh = _id_rows(hyp.reshape(P, Lh), "hyp")     # a view where the (B, N) strides allow
    if ref_lengths is None:
        rl = torch.full((B,), Lr, dtype=torch.int32, device=dev)
    else:
        rl = _lengths(ref_lengths, B, dev, None, "ref_lengths").reshape(-1).clamp(0, Lr)
    if hyp_lengths is None:
        hl = torch.full((P,), Lh, dtype=torch.int32, device=dev)
    else:
        hl = _lengths(hyp_lengths, P, dev, None, "hyp_lengths").reshape(-1)
    dist, counts, pair_ref, pair_hyp, n_pairs = _ops.edit_distance(r2, ldr, rl, h2, ldh, hl, P, group, Lr, Lh,
                                                                   want_ops)
    if not want_ops:
        return EditDistance(dist.view(lead), rl, None, None, None, None)
    return EditDistance(dist.view(lead), rl, counts.view(lead + (4,)), pair_ref.view(lead + (Lr + Lh,)),
                        pair_hyp.view(lead + (Lr + Lh,)), n_pairs.view(lead))


ExpectedRisk = namedtuple("ExpectedRisk", "loss ll post")
NBEST_MAX = 128
NBEST_MAX_LABELS = 511


def _nbest_problem(logits, hyps, hyp_lengths, input_lengths, blank, batch_first, max_labels, who):
    """(x, il, hyp rows int32, ldh, hl (B*N,) int32, N, max_labels) of an n-best call."""
    x, B, T = _logits(logits, batch_first, who, need_3d=True)
    _check_blank(blank, x.shape[-1])
    if not torch.is_tensor(hyps) or not hyps.is_cuda:
        raise RuntimeError(f"{who} runs on libcfm: CUDA id tensors required")
    if hyps.dim() != 3 or hyps.shape[0] != B:
        raise ValueError(f"hyps must be (B, N, L) with B = {B}, got {tuple(hyps.shape)}")
    N, Lh = hyps.shape[1], hyps.shape[2]
    if not 1 <= N <= NBEST_MAX:
        raise ValueError(f"N must be in [1, {NBEST_MAX}], got {N}")
    if max_labels is None:
        max_labels = min(Lh, NBEST_MAX_LABELS)
    max_labels = int(max_labels)
    if not 0 <= max_labels <= min(Lh, NBEST_MAX_LABELS):
        raise ValueError(f"max_labels must be in [0, min(L, {NBEST_MAX_LABELS})] = [0, {min(Lh, NBEST_MAX_LABELS)}], "
                         f"got {max_labels}")
    h2, ldh = _id_rows(hyps.reshape(B * N, Lh), "hyps")
    if hyp_lengths is None:
        hl = torch.full((B * N,), Lh, dtype=torch.int32, device=x.device)
    else:
        if isinstance(hyp_lengths, (list, tuple)):
            hyp_lengths = torch.tensor(hyp_lengths)
        if not torch.is_tensor(hyp_lengths) or hyp_lengths.numel() != B * N:
            raise ValueError(f"hyp_lengths must hold (B, N) = ({B}, {N}) lengths (negative: a missing hypothesis)")
        if not hyp_lengths.is_cuda and hyp_lengths.numel() > 0 and int(hyp_lengths.max()) > Lh:
            raise ValueError(f"expected hyp_lengths to have value at most {Lh}, but got value {int(hyp_lengths.max())}")
        hl = hyp_lengths.to(device=x.device, dtype=torch.int32).reshape(-1).contiguous()
    if input_lengths is None:
        il = torch.full((B,), T, dtype=torch.int32, device=x.device)
    else:
        il = _lengths(input_lengths, B, x.device, T, "input_lengths")
    return x, il, h2, ldh, hl, N, max_labels


def nbest_log_likelihood(logits, hyps, hyp_lengths=None, input_lengths=None, blank=0, batch_first=True,
                         max_labels=None):
    """Full CTC log-likelihood of each hypothesis of an n-best list (cfm_ctc_nbest_fwd): rescoring the beam's n-best,
    whose own scores sum only the alignments the beam kept.  logits (B, T, V) fp32 CUDA (or (T, B, V) with
    batch_first=False), raw or log-probabilities; hyps (B, N, L) int32 / int64 CUDA ids, e.g. beam_search_decode's
    tokens; hyp_lengths (B, N) device tensor, host list or None (L), a negative length marks a missing hypothesis;
    input_lengths as for forced_align.  Device lengths and ids are clamped, never read back.  1 <= N <= 128; at most
    max_labels (None: min(L, 511)) labels per hypothesis, longer ones are left out like missing ones.
    Returns (ll (B, N), post (B, N)) fp32, no gradient: ll = log P_ctc(hypothesis | logits) over all alignments (-inf
    where infeasible, not finite, missing or too long), post = softmax of ll over the utterance's finite entries."""
    blank = int(blank)
    x, il, h2, ldh, hl, N, ml = _nbest_problem(logits, hyps, hyp_lengths, input_lengths, blank, batch_first, max_labels,
                                               "nbest_log_likelihood")
    with torch.no_grad():
        ll, post, _, _ = ops.ctc_nbest_fwd(x.detach(), il, h2, ldh, hl, N, ml, blank, None, batch_first)
    return ll, post


class _ExpectedRiskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, il, h2, ldh, hl, N, ml, blank, risk, batch_first):
        ll, post, loss, ws = ops.ctc_nbest_fwd(x, il, h2, ldh, hl, N, ml, blank, risk, batch_first)
        ctx.save_for_backward(x, il, h2, hl, ws)
        ctx.cfg = (ldh, N, ml, blank, batch_first)
        ctx.mark_non_differentiable(ll, post)
        return loss, ll, post

    @staticmethod
    def backward(ctx, g, _gll, _gpost):
        x, il, h2, hl, ws = ctx.saved_tensors
        ldh, N, ml, blank, bf = ctx.cfg
        dx = ops.ctc_nbest_bwd(x, il, h2, ldh, hl, N, ml, blank, ws, g, bf)
        return dx, None, None, None, None, None, None, None, None, None


def expected_risk_loss(logits, hyps, hyp_lengths, risk, input_lengths=None, blank=0, batch_first=True,
                       max_labels=None):
    """Expected risk over an n-best list (cfm_ctc_nbest_fwd / _bwd): the MWER criterion of Prabhavalkar et al. 2018
    with the CTC likelihood as the hypothesis posterior.  Arguments as nbest_log_likelihood, plus risk (B, N): any
    numbers (fp32 is used), word errors being the use.  With the live hypotheses those with a finite ll:
      post = softmax of ll over the live n, rbar = mean of risk over the live n,
      loss[b] = sum_n post[b, n] * (risk[b, n] - rbar[b])      (0 with fewer than two live hypotheses)
    Returns the named tuple (loss (B,), ll (B, N), post (B, N)); the gradient flows to logits only:
      d loss[b] / d logits[b, t, v] = sum_n c[b, n] * occ_n[t, v],  c = post * ((risk - rbar) - loss),
    occ_n[t, v] the posterior probability that hypothesis n's alignment emits v at frame t.  The softmax term of the
    CTC gradient cancels (sum_n c = 0) and is never formed: the gradient is exactly zero outside the blank and the
    hypotheses' labels, beyond each utterance's length, and where the risks are all equal."""
    blank = int(blank)
    x, il, h2, ldh, hl, N, ml = _nbest_problem(logits, hyps, hyp_lengths, input_lengths, blank, batch_first, max_labels,
                                               "expected_risk_loss")
    if not torch.is_tensor(risk) or not risk.is_cuda:
        raise RuntimeError("expected_risk_loss runs on libcfm: a CUDA risk tensor required")
    if risk.numel() != hl.numel():
        raise ValueError(f"risk must be (B, N) = {(hl.numel() // N, N)}, got {tuple(risk.shape)}")
    r = risk.detach().to(torch.float32).reshape(-1).contiguous()
    return ExpectedRisk(*_ExpectedRiskFn.apply(x, il, h2, ldh, hl, N, ml, blank, r, bool(batch_first)))


def mwer_loss(logits, targets, input_lengths, target_lengths, nbest=4, beam_size=None, blank=0, pad=-1,
              batch_first=True, max_labels=None, lm=None, **lm_kw):
    """Minimum word error rate loss: the expected number of word errors over the beam's own n-best list.  Without
    gradient, on the detached logits: beam_search_decode(nbest=nbest, beam_size=beam_size or nbest, lm=lm, **lm_kw)
    and edit_distance of its hypotheses against targets (B, Lr) CUDA ids / target_lengths; hypotheses the beam did not
    fill (score -inf) are marked missing; then expected_risk_loss on the attached logits with the distances as the
    risk.  Hypotheses are cut to 511 labels (max_labels None: min(T, 511)); longer ones are not live.
    Returns (loss (B,), the EditDistance of the n-best list, post (B, N)).  No host synchronisation."""
    if not isinstance(nbest, int) or isinstance(nbest, bool) or not 1 <= nbest <= NBEST_MAX:
        raise ValueError(f"nbest must be an integer in [1, {NBEST_MAX}], got {nbest!r}")
    W = max(int(beam_size) if beam_size else nbest, nbest)
    with torch.no_grad():
        tokens, lens, scores = beam_search_decode(logits.detach(), input_lengths, beam_size=W, blank=blank, pad=pad,
                                                  nbest=nbest, batch_first=batch_first, lm=lm, **lm_kw)
        width = min(tokens.shape[-1], NBEST_MAX_LABELS)
        lens = torch.where(scores == float("-inf"), torch.full_like(lens, -1), lens)
        hyps = tokens[..., :width]
        ed = edit_distance(hyps, targets, lens, target_lengths)
        risk = ed.distance.to(torch.float32)
    out = expected_risk_loss(logits, hyps, lens, risk, input_lengths, blank, batch_first,
                             width if max_labels is None else max_labels)
    return out.loss, ed, out.post
