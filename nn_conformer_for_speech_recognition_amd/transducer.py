"""RNN-T (transducer) objective on libcfm — the Conformer's other published head (Graves 2012; Gulati et al. 2020).

  rnnt_loss        the transducer loss of dense joint logits (B, T, U + 1, V), the interface of
                   torchaudio.functional.rnnt_loss: csrc/rnnt.hip (cfm_rnnt_loss_fwd / _bwd) behind an autograd function.
  TransducerHead   prediction network (Embedding -> lstm.LSTM per utterance) + joint network + rnnt_loss on an encoder
                   output, with a time-synchronous greedy decode: decode (one kernel launch) and greedy_decode (the
                   same search restated as a loop of torch ops).
  rnnt_greedy_decode   that search on the head's weights as arrays: csrc/rnnt_greedy.hip (cfm_rnnt_greedy).

The loss and the decode are the hot paths and run on HIP kernels; the joint network is plain torch ops (see
TransducerHead).  Nothing
here reads a device value back: lengths given as device tensors are clamped by the kernels.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

from . import ops
from .ctc import _RED, _check_blank, _id_rows, _lengths
from .lstm import LSTM

RNNT_MAX_LABELS = 1023


class _RNNTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tg, ldt, il, tl, blank, zero_infinity):
        x = x.contiguous()
        ll, ws = ops.rnnt_loss_fwd(x, tg, ldt, il, tl, blank)
        ctx.save_for_backward(x, tg, il, tl, ws)
        ctx.cfg = (ldt, blank)
        nll = -ll
        return torch.where(torch.isinf(ll), torch.zeros_like(nll), nll) if zero_infinity else nll

    @staticmethod
    def backward(ctx, g):
        x, tg, il, tl, ws = ctx.saved_tensors
        ldt, blank = ctx.cfg
        # (an utterance whose ll is -inf gets a zero gradient from the kernel whatever g holds)
        dx = ops.rnnt_loss_bwd(x, tg, ldt, il, tl, blank, ws, g)
        return dx, None, None, None, None, None, None


def rnnt_loss(logits, targets, logit_lengths=None, target_lengths=None, blank=0, reduction="mean",
              zero_infinity=False):
    """RNN-T loss on the device (cfm_rnnt_loss_fwd / _bwd).

    logits (B, T, U1, V) CUDA, U1 = Umax + 1: the joint network's output, raw (log-softmax over V is applied).  Other
    dtypes than fp32 are cast to fp32, a non-contiguous tensor is made contiguous.  targets (B, >= Umax) int32 / int64
    ids holding no blanks; logit_lengths / target_lengths: device tensors, host lists or None (T / Umax).  Host-side
    lengths are validated (ValueError); device lengths and the labels are clamped on the device to [0, T],
    [0, Umax] and [0, V - 1] and never read back.  At most RNNT_MAX_LABELS = 1023 labels per utterance.

    With T_b, U_b the lengths, lp = log_softmax(logits), b(t,u) = lp[t,u,blank], y(t,u) = lp[t,u,label_{u+1}]:
      alpha(0,0) = 0;  alpha(t,u) = lse(alpha(t-1,u) + b(t-1,u), alpha(t,u-1) + y(t,u-1))
      loss_b = -(alpha(T_b-1,U_b) + b(T_b-1,U_b))
    reduction: 'none' (B,), 'sum', or 'mean' = the mean over the batch of the per-utterance loss (torchaudio's rule).
    An utterance without frames (T_b = 0) takes no part: its loss is +inf, or 0 with zero_infinity, as is a loss that
    is not finite; its gradient is zero either way.

    The gradient is exactly zero outside the valid cells t < T_b, u <= U_b (whose logits are never read), and every
    valid row of it sums to 0 over v.  alpha, beta and the loss are kept in double on the device; two runs on the same
    inputs are bit-identical."""
    if reduction not in _RED:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    if not torch.is_tensor(logits) or not logits.is_cuda or not logits.is_floating_point():
        raise RuntimeError("rnnt_loss runs on libcfm: floating-point CUDA logits required")
    if logits.dim() != 4:
        raise ValueError("logits must be (B, T, U + 1, V)")
    B, T, U1, V = logits.shape
    if min(B, T, U1) < 1 or V < 2:
        raise ValueError(f"logits (B, T, U + 1, V) need B, T, U + 1 >= 1 and V >= 2, got {tuple(logits.shape)}")
    blank = int(blank)
    _check_blank(blank, V)
    if U1 - 1 > RNNT_MAX_LABELS:
        raise ValueError(f"rnnt_loss takes at most {RNNT_MAX_LABELS} labels per utterance, got {U1 - 1}")
    if not torch.is_tensor(targets):
        targets = torch.tensor(targets, dtype=torch.int64)
    if targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] < U1 - 1:
        raise ValueError(f"targets must be (B, >= U) = ({B}, >= {U1 - 1}), got {tuple(targets.shape)}")
    dev = logits.device
    tg, ldt = _id_rows(targets.to(dev), "targets")
    il = (torch.full((B,), T, dtype=torch.int32, device=dev) if logit_lengths is None
          else _lengths(logit_lengths, B, dev, T, "logit_lengths"))
    tl = (torch.full((B,), U1 - 1, dtype=torch.int32, device=dev) if target_lengths is None
          else _lengths(target_lengths, B, dev, U1 - 1, "target_lengths"))
    x = logits if logits.dtype == torch.float32 else logits.float()
    nll = _RNNTFn.apply(x, tg, ldt, il, tl, blank, bool(zero_infinity))
    if reduction == "none":
        return nll
    return nll.sum() if reduction == "sum" else nll.mean()


class RNNTLoss(nn.Module):
    """rnnt_loss as a module (torchaudio.transforms.RNNTLoss's arguments, plus zero_infinity)."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in _RED:
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity

    def forward(self, logits, targets, logit_lengths=None, target_lengths=None):
        return rnnt_loss(logits, targets, logit_lengths, target_lengths, self.blank, self.reduction,
                         self.zero_infinity)


RNNTGreedy = namedtuple("RNNTGreedy", "tokens counts frames scores")


def rnnt_greedy_decode(ep, gtab, w_hh, w_pp, b_pp, w_out, b_out, lengths=None, blank=0, max_symbols=2,
                       max_tokens=None):
    """Time-synchronous greedy search of a transducer head on the device, one launch (cfm_rnnt_greedy).

    ep (B, T, J) = enc_proj(enc) with bias; gtab (V, 4H) = embedding.weight @ W_ih^T + b_ih + b_hh; w_hh (4H, H);
    w_pp (J, H), b_pp (J): pred_proj; w_out (V, J), b_out (V): out.  CUDA floating-point tensors (cast to fp32, made
    contiguous).  lengths: device tensor (clamped on the device to [0, T], never read back), host list (validated,
    ValueError) or None (T).  H a multiple of 8, H and J at most 1024.
    -> RNNTGreedy(tokens (B, W) int32 padded with -1, counts (B,) int32, frames (B, W) int32 padded with -1: the frame
    each token was emitted at, scores (B,) fp32: the sum of log_softmax(logits)[chosen] over every decision taken --
    labels and the blanks that close a frame; a frame closed by the max_symbols cap adds no blank term).
    W = max_tokens or T * max_symbols; an utterance that has emitted W tokens stops there.  Ties of the argmax go to
    the lowest index (torch's rule).  No host synchronisation; two runs are bit-identical."""
    ts = (ep, gtab, w_hh, w_pp, b_pp, w_out, b_out)
    if not all(torch.is_tensor(t) and t.is_cuda and t.is_floating_point() for t in ts):
        raise RuntimeError("rnnt_greedy_decode runs on libcfm: floating-point CUDA tensors required")
    if ep.dim() != 3 or w_out.dim() != 2 or w_hh.dim() != 2 or w_pp.dim() != 2 or gtab.dim() != 2:
        raise ValueError("ep must be (B, T, J), gtab (V, 4H), w_hh (4H, H), w_pp (J, H), w_out (V, J)")
    B, T, J = ep.shape
    V, H = w_out.shape[0], w_hh.shape[1]
    if min(B, T, J, H) < 1 or V < 2:
        raise ValueError(f"need B, T, J, H >= 1 and V >= 2, got B {B}, T {T}, J {J}, H {H}, V {V}")
    shapes = {"gtab": (gtab, (V, 4 * H)), "w_hh": (w_hh, (4 * H, H)), "w_pp": (w_pp, (J, H)), "b_pp": (b_pp, (J,)),
              "w_out": (w_out, (V, J)), "b_out": (b_out, (V,))}
    for name, (t, shape) in shapes.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    blank, max_symbols = int(blank), int(max_symbols)
    _check_blank(blank, V)
    if max_symbols < 1:
        raise ValueError("max_symbols must be >= 1")
    W = T * max_symbols if max_tokens is None else int(max_tokens)
    if W < 1:
        raise ValueError("max_tokens must be >= 1")
    dev = ep.device
    lens = None if lengths is None else _lengths(lengths, B, dev, T, "lengths")
    ep, gtab, w_hh, w_pp, b_pp, w_out, b_out = (t.to(device=dev, dtype=torch.float32).contiguous() for t in ts)
    tokens, frames, counts, scores = ops.rnnt_greedy(ep, gtab, w_hh, w_pp, b_pp, w_out, b_out, lens, blank,
                                                     max_symbols, W)
    return RNNTGreedy(tokens, counts, frames, scores)


class TransducerHead(nn.Module):
    """A transducer head on an encoder output enc (B, T, enc_dim).

    Prediction network: Embedding(n_tokens, embed) over [blank, l_1 .. l_U] (the blank id is the start symbol) ->
    lstm.LSTM(embed, hidden), one sequence per utterance with lengths target_lengths + 1.
    Joint network: Linear(enc_dim, joint)(enc)[:, :, None] + Linear(hidden, joint)(pred)[:, None] -> tanh ->
    Linear(joint, n_tokens).
    Loss: rnnt_loss on the joint logits.

    The joint network is plain torch ops and is NOT a tuned path: it materialises the (B, T, U + 1, joint) hidden
    tensor and the (B, T, U + 1, n_tokens) fp32 logits -- B * T * (U + 1) * n_tokens * 4 bytes, 391 MB at B 32, T 373,
    U 8, V 1024 -- and autograd keeps both for the backward.  A joint fused with the loss is future work."""

    def __init__(self, enc_dim, n_tokens, blank, embed=128, hidden=256, joint=256):
        super().__init__()
        if not 0 <= int(blank) < n_tokens:
            raise ValueError(f"blank must be in [0, {n_tokens}), got {blank}")
        self.n_tokens, self.blank = int(n_tokens), int(blank)
        self.embedding = nn.Embedding(n_tokens, embed)
        self.prediction = LSTM(embed, hidden, batch_first=True)
        self.enc_proj = nn.Linear(enc_dim, joint)
        self.pred_proj = nn.Linear(hidden, joint)
        self.out = nn.Linear(joint, n_tokens)

    def _labels(self, targets, target_lengths, B, device):
        """(ids (B, U1) int64 = [blank, targets] clamped to the vocabulary, targets on the device, U, the prediction
        network's lengths = target_lengths + 1)."""
        if not torch.is_tensor(targets):
            targets = torch.tensor(targets, dtype=torch.int64)
        if targets.dim() != 2 or targets.shape[0] != B:
            raise ValueError(f"targets must be (B, U) with B = {B}, got {tuple(targets.shape)}")
        targets = targets.to(device)
        U = targets.shape[1]
        if U > RNNT_MAX_LABELS:
            raise ValueError(f"TransducerHead takes at most {RNNT_MAX_LABELS} labels per utterance, got {U}")
        start = torch.full((B, 1), self.blank, dtype=torch.int64, device=device)
        ids = torch.cat([start, targets.long().clamp(0, self.n_tokens - 1)], 1)
        if target_lengths is None:
            plens = None
        elif torch.is_tensor(target_lengths):
            plens = target_lengths.to(device).clamp(0, U) + 1
        else:
            plens = [int(v) + 1 for v in target_lengths]
        return ids, targets, U, plens

    def joint(self, enc, pred):
        """Joint logits (B, T, U1, n_tokens) fp32 of enc (B, T, enc_dim) and pred (B, U1, hidden)."""
        h = self.enc_proj(enc.float()).unsqueeze(2) + self.pred_proj(pred.float()).unsqueeze(1)
        return self.out(torch.tanh(h))

    def joint_logits(self, enc, targets, target_lengths=None):
        """The logits the loss sees: (B, T, U + 1, n_tokens) fp32 for targets (B, U)."""
        ids, _, _, plens = self._labels(targets, target_lengths, enc.shape[0], enc.device)
        pred = self.prediction(self.embedding(ids), lengths=plens)[0]
        return self.joint(enc, pred)

    def forward(self, enc, enc_lengths, targets, target_lengths=None, zero_infinity=False):
        """Per-utterance loss (B,) of enc (B, T, enc_dim) with enc_lengths valid frames against targets (B, U) with
        target_lengths labels, attached to the graph (reduce it as the training loop needs)."""
        logits = self.joint_logits(enc, targets, target_lengths)
        tg = targets if torch.is_tensor(targets) else torch.tensor(targets, dtype=torch.int64)
        return rnnt_loss(logits, tg, enc_lengths, target_lengths, blank=self.blank, reduction="none",
                         zero_infinity=zero_infinity)

    def _cell(self, x, h, c):
        """One step of the prediction network's LSTM cell with the module's own weights (lstm.LSTM takes no initial
        state): gate order i, f, g, o."""
        p = self.prediction
        gates = x @ p.weight_ih_l0.t() + h @ p.weight_hh_l0.t()
        if p.bias:
            gates = gates + p.bias_ih_l0 + p.bias_hh_l0
        i, f, g, o = gates.chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c

    @torch.no_grad()
    def greedy_decode(self, enc, enc_lengths=None, max_symbols=2):
        """Time-synchronous greedy search: at each frame emit the joint's argmax and advance the prediction network
        until it is the blank, at most max_symbols times, then move to the next frame.
        -> (tokens (B, T * max_symbols) int32 padded with -1, counts (B,) int32).

        A FUNCTIONAL decode, not a tuned one: a Python loop over T * max_symbols steps of small torch ops.  Every
        frame runs its max_symbols inner iterations and masks stand in for data-dependent control flow, so nothing is
        read back from the device (no host synchronisation).  enc_lengths: device tensor, host list or None (T)."""
        if max_symbols < 1:
            raise ValueError("max_symbols must be >= 1")
        B, T, _ = enc.shape
        dev = enc.device
        W = T * max_symbols
        lens = (torch.full((B,), T, dtype=torch.int64, device=dev) if enc_lengths is None
                else _lengths(enc_lengths, B, dev, T, "enc_lengths").long())
        H = self.prediction.hidden_size
        tokens = torch.full((B, W), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros(B, dtype=torch.int64, device=dev)
        zero = torch.zeros(B, H, device=dev)
        start = torch.full((B,), self.blank, dtype=torch.int64, device=dev)
        h, c = self._cell(self.embedding(start), zero, zero)
        ep = self.enc_proj(enc.float())                                   # (B, T, joint)
        for t in range(T):
            open_ = lens > t                                              # still emitting at this frame
            for _ in range(max_symbols):
                logits = self.out(torch.tanh(ep[:, t] + self.pred_proj(h)))
                tok = logits.argmax(-1)
                emit = open_ & (tok != self.blank)
                at = counts.clamp(max=W - 1).unsqueeze(1)
                cur = tokens.gather(1, at)
                tokens.scatter_(1, at, torch.where(emit.unsqueeze(1), tok.to(torch.int32).unsqueeze(1), cur))
                counts += emit
                h2, c2 = self._cell(self.embedding(tok), h, c)
                h = torch.where(emit.unsqueeze(1), h2, h)
                c = torch.where(emit.unsqueeze(1), c2, c)
                open_ = emit                                              # a blank closes the frame
        return tokens, counts.to(torch.int32)

    @torch.no_grad()
    def decode(self, enc, enc_lengths=None, max_symbols=2, max_tokens=None):
        """greedy_decode's search as one kernel launch (rnnt_greedy_decode: real data-dependent control flow on the
        device, a blank ends the frame's work) -> RNNTGreedy(tokens (B, W) int32 padded with -1, counts, frames,
        scores), W = max_tokens or T * max_symbols.  enc_proj(enc) and the cell's input table embedding.weight @
        W_ih^T + biases are one GEMM each per call; nothing is read back.  enc_lengths: device tensor, host list or
        None (T)."""
        p = self.prediction
        gtab = self.embedding.weight.float() @ p.weight_ih_l0.float().t()
        if p.bias:
            gtab = gtab + (p.bias_ih_l0 + p.bias_hh_l0).float()
        ep = self.enc_proj(enc.float())
        return rnnt_greedy_decode(ep, gtab, p.weight_hh_l0, self.pred_proj.weight, self.pred_proj.bias,
                                  self.out.weight, self.out.bias, enc_lengths, blank=self.blank,
                                  max_symbols=max_symbols, max_tokens=max_tokens)
