"""cfm_ctc_loss_fwd, cfm_ctc_loss_bwd and cfm_ctc_forced_align share one argument check (check_ctc_problem,
csrc/ctc_common.h): each rejects the same bad problems with the same code, under its own name, and takes a good one.

The calls go through the C ABI directly.  Every rejected call is given real device buffers sized so that it would
stay in bounds even if a regression accepted it (the assertion must fail then, not the card): the logits are the
middle third of a three times wider allocation (a class index of -1 or V is inside it), the workspaces are sized
for Smax = 512 and are themselves the middle third of an allocation three times that size (Smax = -1 makes the
state stride -1, so a work array's rows would run downwards from its base), the per-label outputs are sized for
Smax = 512, and the target lengths are 0 (no label is read, no state but the first is touched)."""
import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, V, SMAX, BIG = 2, 8, 8, 4, 512
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -5

# (B, Smax, ldt, blank) -> code; the good problem is (B, SMAX, SMAX, 0)
BAD = {
    "B = 0": ((0, SMAX, SMAX, 0), ERR_SHAPE),
    "Smax = -1": ((B, -1, SMAX, 0), ERR_SHAPE),
    "ldt < Smax without offsets": ((B, SMAX, SMAX - 1, 0), ERR_SHAPE),
    "blank = V": ((B, SMAX, SMAX, V), ERR_ARG),
    "blank = -1": ((B, SMAX, SMAX, -1), ERR_ARG),
    "Smax = 512": ((B, BIG, BIG, 0), ERR_UNSUPPORTED),
}


class _Buffers:
    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.wide = torch.randn(B, T, 3 * V, generator=g).to(DEV)
        self.x = self.wide[:, :, V:2 * V]                                  # sb = 3 V T, st = 3 V
        self.targets = torch.ones(B, BIG, dtype=torch.int32, device=DEV)
        self.in_len = torch.full((B,), T, dtype=torch.int32, device=DEV)
        self.tgt_len = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.nll = torch.zeros(B, device=DEV)
        self.grad_out = torch.ones(B, device=DEV)
        self.grad = torch.zeros(B, T, V, device=DEV)
        self.ws = self._middle(L.size_call("cfm_ctc_ws_bytes", B, T, BIG))
        self.align_ws = self._middle(L.size_call("cfm_ctc_align_ws_bytes", B, T, BIG))
        self.alignments = torch.zeros(B, T, dtype=torch.int32, device=DEV)
        self.scores = torch.zeros(B, T, device=DEV)
        self.score = torch.zeros(B, device=DEV)
        self.starts = torch.zeros(B, BIG, dtype=torch.int32, device=DEV)
        self.ends = torch.zeros(B, BIG, dtype=torch.int32, device=DEV)
        self.token_scores = torch.zeros(B, BIG, device=DEV)

    def _middle(self, nbytes):
        """nbytes (rounded up to 256) in the middle of an allocation three times as large."""
        n = (nbytes + 255) & ~255
        self.keep = getattr(self, "keep", []) + [torch.zeros(3 * n, dtype=torch.uint8, device=DEV)]
        return self.keep[-1][n:2 * n]

    def call(self, name, b, smax, ldt, blank):
        """The entry point's return code for the problem (b utterances, smax, ldt, blank); everything else is good."""
        p = L.ptr
        head = (p(self.x), self.x.stride(0), self.x.stride(1), p(self.targets), ldt, None, p(self.in_len),
                p(self.tgt_len), b, T, V, smax, blank)
        lib = L.load()
        if name == "cfm_ctc_loss_fwd":
            return lib.cfm_ctc_loss_fwd(*head, 1, p(self.nll), p(self.ws), L.stream())
        if name == "cfm_ctc_loss_bwd":
            return lib.cfm_ctc_loss_bwd(*head, 1, p(self.ws), p(self.grad_out), 1, 0, p(self.grad), L.F32,
                                        self.grad.stride(0), self.grad.stride(1), L.stream())
        return lib.cfm_ctc_forced_align(*head, p(self.alignments), p(self.scores), p(self.score), p(self.starts),
                                        p(self.ends), p(self.token_scores), p(self.align_ws), L.stream())


ENTRY_POINTS = ("cfm_ctc_loss_fwd", "cfm_ctc_loss_bwd", "cfm_ctc_forced_align")   # (the backward after its forward)


def test_shared_argument_check():
    buf = _Buffers()
    lib = L.load()
    for name in ENTRY_POINTS:
        assert buf.call(name, B, SMAX, SMAX, 0) == 0, (name, lib.cfm_get_last_error())
    torch.cuda.synchronize()
    # empty targets: the loss is -sum_t log p(blank), the alignment is all blank with that score
    lp = torch.log_softmax(buf.x.double(), -1)[:, :, 0].sum(1)
    assert torch.allclose(buf.nll.double(), -lp, rtol=1e-5, atol=1e-5)
    assert torch.allclose(buf.score.double(), lp, rtol=1e-5, atol=1e-5)
    assert int(buf.alignments.abs().max()) == 0 and torch.isfinite(buf.grad).all()

    for what, (problem, code) in BAD.items():
        for name in ENTRY_POINTS:
            rc = buf.call(name, *problem)
            msg = lib.cfm_get_last_error().decode()
            print(f"  {what:28s} {name:22s} -> {rc}  {msg}")
            assert rc == code, (what, name, rc, msg)
            assert msg.startswith(name + ": "), (what, name, msg)
    torch.cuda.synchronize()
