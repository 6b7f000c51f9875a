"""Adafactor on libcfm — the reference's optimizer (lib/standard/runner.py:36,
``transformers.Adafactor(model.parameters(), lr=hp.lr, beta1=hp.beta1, scale_parameter=False,
relative_step=False)``) as ONE multi-tensor HIP step over all parameters (csrc/optim.hip) instead
of ~10 small PyTorch kernels per tensor.

Same constructor signature, defaults and state keys as transformers' Adafactor (exp_avg,
exp_avg_sq_row, exp_avg_sq_col / exp_avg_sq, step, RMS), every option on the device path:
relative_step and warmup_init (the learning-rate schedule), scale_parameter (the step is scaled by
max(eps[1], RMS(p)) per tensor; RMS(p) is summed in the pass that already sums the update's
squares) and weight_decay.  ``state[p]["RMS"]`` is a 0-d device tensor with scale_parameter=True
(a view of one buffer per group, refreshed by every step without a host sync) and stays 0 without
it: nothing reads it then, and the scale_parameter=False step loads nothing for it.

``capturable=True`` (torch.optim's name) makes ``step()`` free of host-dependent scalars: the
group's step count is one device int32 (``state[p]["step"]`` is a view of it), incremented by the
step itself, and beta2t and the relative step size are computed from it on the device.  One eager
warm-up step builds and uploads the task table and the buffers; after it ``step()`` makes no
host-to-device copy and may be captured into a HIP graph and replayed, with the gradients written
into the same ``.grad`` buffers.  Without it the scalars come from the Python step count, as
before.  All parameters of a group share one step count (either way).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L

_NEEDS_WARMUP = ("libcfm Adafactor: one eager warm-up step builds and uploads the table and buffers; "
                 "then step() may be captured and replayed")


class Adafactor(torch.optim.Optimizer):
    def __init__(self, params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None,
                 weight_decay=0.0, scale_parameter=True, relative_step=True, warmup_init=False, capturable=False):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        defaults = dict(lr=lr, eps=eps, clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1,
                        weight_decay=weight_decay, scale_parameter=scale_parameter, relative_step=relative_step,
                        warmup_init=warmup_init, capturable=capturable)
        super().__init__(params, defaults)
        self._step = 0
        self._dev = {}
        self._tables = {}
        self._fast = {}
        self._gbuf = {}     # per (group, device): RMS(p) per parameter; step counter and scalars if capturable
        self._stepped = set()   # ids of the device step counters that have counted a step

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:     # a state dict saved before the keyword existed (or by transformers)
            group.setdefault("capturable", False)

    @staticmethod
    def _geom(p):
        if p.dim() >= 2:
            R, C = p.shape[-2], p.shape[-1]
            return True, p.numel() // (R * C), R, C
        return False, 1, 1, p.numel()

    def _group_buffers(self, group, dev):
        """(rms, step, scalars) of a group: rms one float per parameter of the group (state["RMS"] views
        it); step (int32) and the two device scalars only when capturable."""
        key = (id(group), dev)
        gb = self._gbuf.get(key)
        if gb is None:
            rms = torch.zeros(len(group["params"]), device=dev)
            cap = group["capturable"]
            gb = (rms, torch.zeros((), dtype=torch.int32, device=dev) if cap else None,
                  torch.zeros(2, device=dev) if cap else None)
            self._gbuf[key] = gb
        return gb

    def _ensure_state(self, p, group):
        st = self.state[p]
        if len(st) == 0:
            factored, nb, R, C = self._geom(p)
            st["step"] = 0
            if group["beta1"] is not None:
                st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
            if factored:
                st["exp_avg_sq_row"] = torch.zeros(p.shape[:-1], device=p.device, dtype=torch.float32)
                st["exp_avg_sq_col"] = torch.zeros(p.shape[:-2] + p.shape[-1:], device=p.device, dtype=torch.float32)
            else:
                st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
            st["RMS"] = 0
        return st

    def _ptrkey(self, ps):
        """Every buffer the cached task table points at: parameter, gradient AND optimizer state
        (exp_avg, exp_avg_sq_row/col or exp_avg_sq).  A state swap (load_state_dict, a reset of
        self.state) changes the key, so the kernel never writes through a stale table."""
        key = []
        for p in ps:
            st = self.state.get(p, {})
            key.append((p.data_ptr(), p.grad.data_ptr(),
                        *(st[k].data_ptr() if torch.is_tensor(st.get(k)) else 0
                          for k in ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"))))
        return tuple(key)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():     # the device step reads fp32 contiguous state on the param's device
            for k in ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
                if torch.is_tensor(st.get(k)):
                    st[k] = st[k].float().contiguous()
        self._fast.clear()
        self._tables.clear()
        self._dev.clear()       # (keyed on the group dicts, which super().load_state_dict has replaced)
        self._gbuf.clear()
        self._stepped.clear()
        for group in self.param_groups:
            with_state = [p for p in group["params"] if len(self.state.get(p, {}))]
            if not with_state:
                continue
            dev = with_state[0].device
            if group["capturable"]:
                # the loaded step count goes into the group's device counter; the states view it again
                steps = {int(self.state[p]["step"]) for p in with_state}
                if len(steps) != 1:
                    raise L.CfmError("libcfm Adafactor: all parameters of a group must share the step count")
                counter = self._group_buffers(group, dev)[1]
                counter.fill_(steps.pop())
                self._stepped.add(id(counter))
                for p in with_state:
                    self.state[p]["step"] = counter
            else:
                for p in with_state:
                    self.state[p]["step"] = int(self.state[p]["step"])
            if group["scale_parameter"]:
                # re-point RMS at the group buffer (the loaded value is overwritten by the next step anyway)
                rms = self._group_buffers(group, dev)[0]
                for i, p in enumerate(group["params"]):
                    if len(self.state.get(p, {})):
                        self.state[p]["RMS"] = rms[i]

    def _lr(self, group, step):
        lr = group["lr"]
        if group["relative_step"]:
            min_step = 1e-6 * step if group["warmup_init"] else 1e-2
            lr = min(min_step, 1.0 / math.sqrt(step))
        return lr

    def _build_table(self, group, ps, dev):
        """Host-side task table of one group (one planned fill) -> (device copy, the plan's totals)."""
        n = len(ps)
        host = (ctypes.c_char * L.size_call("cfm_adafactor_table_bytes", n))()
        params = (L.AdafactorParam * n)()
        rms, counter, _ = self._group_buffers(group, dev)
        for i, p in enumerate(ps):
            st = self._ensure_state(p, group)
            if counter is not None:
                if st["step"] is not counter:
                    # a state that joins late (or was put there by hand) cannot share the group's device counter
                    if torch.is_tensor(st["step"]) or st["step"] != 0 or id(counter) in self._stepped:
                        raise L.CfmError("libcfm Adafactor: all parameters of a group must share the step count")
                    st["step"] = counter
            if group["scale_parameter"]:
                st["RMS"] = rms[i]          # the kernel writes RMS(p) of table entry i here
            factored, nb, R, C = self._geom(p)
            m = st.get("exp_avg")
            row = st["exp_avg_sq_row"] if factored else st["exp_avg_sq"]
            col = st["exp_avg_sq_col"] if factored else None
            params[i] = L.AdafactorParam(L.ptr(p), L.ptr(p.grad), L.ptr(m), L.ptr(row), L.ptr(col), p.numel(),
                                         nb, R, C, factored)
        totals = L.AdafactorTotals()
        L.call("cfm_adafactor_fill_table", ctypes.cast(host, ctypes.c_void_p), params, n, ctypes.byref(totals))
        raw = bytes(host)
        tkey = (id(group), dev)
        cached = self._tables.get(tkey)
        if cached is not None and cached[0] == raw:
            table = cached[1]
        else:
            table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev, non_blocking=False)
            self._tables[tkey] = (raw, table)
        return table, totals

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._step += 1
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise L.CfmError("libcfm Adafactor expects fp32 parameters and gradients")
                if not p.grad.is_contiguous():
                    p.grad = p.grad.contiguous()
            n = len(ps)
            dev = ps[0].device
            capturable = group["capturable"]
            # fast path: same parameter / gradient buffers as the cached table (every step of a
            # training loop whose gradients live in a captured graph's pool, or are re-used in
            # place): no per-parameter ctypes table build on the host, only the step counters
            ptrkey = self._ptrkey(ps)
            fast = self._fast.get((id(group), dev))
            if fast is not None and fast[0] == ptrkey:
                table, tot = fast[1], fast[2]
            else:
                if torch.cuda.is_current_stream_capturing():    # no table upload inside a capture
                    raise L.CfmError(_NEEDS_WARMUP)
                table, tot = self._build_table(group, ps, dev)
                self._fast[(id(group), dev)] = (self._ptrkey(ps), table, tot)   # state now exists
            step = None
            if not capturable:      # (capturable: the one device counter, incremented by the step itself)
                steps = set()
                for p in ps:
                    st = self.state[p]
                    st["step"] += 1
                    steps.add(st["step"])
                if len(steps) != 1:
                    raise L.CfmError("libcfm Adafactor: all parameters of a group must share the step count")
                step = steps.pop()
            key = (id(group), dev)
            buf = self._dev.get(key)
            scale = group["scale_parameter"]
            if (buf is None or buf[0].numel() < tot.rowmean_floats or buf[1].numel() < tot.part_floats
                    or buf[2].numel() < tot.blocks or (scale and buf[3] is None)):
                buf = (torch.empty(max(tot.rowmean_floats, 1), device=dev),
                       torch.empty(max(tot.part_floats, 1), device=dev), torch.empty(max(tot.blocks, 1), device=dev),
                       torch.empty(max(tot.blocks, 1), device=dev) if scale else None)     # block sums of p^2
                self._dev[key] = buf
            beta1 = group["beta1"] if group["beta1"] is not None else 0.0
            # (scale_parameter=False, weight_decay=0, not capturable: the six launches of the reference's step)
            rms, counter, scalars = self._group_buffers(group, dev)
            h = L.AdafactorHyper(decay_rate=group["decay_rate"], beta1=beta1, eps1=group["eps"][0],
                                 eps2=group["eps"][1], clip=group["clip_threshold"],
                                 weight_decay=group["weight_decay"], flags=L.ADA_SCALE_PARAMETER if scale else 0)
            if capturable:
                h.flags |= (L.ADA_DEVICE_STEP | (L.ADA_RELATIVE_STEP if group["relative_step"] else 0)
                            | (L.ADA_WARMUP_INIT if group["warmup_init"] else 0))
                h.lr = group["lr"] if group["lr"] is not None else 0.0
                h.step_dev, h.scalars_dev = L.ptr(counter), L.ptr(scalars)
                self._stepped.add(id(counter))
            else:
                h.lr = self._lr(group, step)
                h.beta2t = 1.0 - math.pow(step, group["decay_rate"])
            bufs = L.AdafactorBuffers(*map(L.ptr, buf), L.ptr(rms))
            L.call("cfm_adafactor_step", L.ptr(table), n, ctypes.byref(tot), ctypes.byref(bufs), ctypes.byref(h),
                   L.stream())
            self._keep = table      # keep the table alive until the stream has consumed it
        return loss
