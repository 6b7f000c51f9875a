"""transducer.TransducerHead, ASRNN's transducer option and Runner.train with hp.transducer_weight
(HParams.set_transducer): ctc + weight * sum_b(rnnt_b) / batch_size.

The head's loss is held to tests/rnnt_ref.py on the head's own joint logits (the bound of tests/test_gpu_rnnt.py); its
parameter gradients to fp64 autograd of a torch restatement of the head (torch.nn.LSTM per utterance, the loss gradient
from the pinned closed form) within tests/test_gpu_lstm_batched.py's bound, relative L2 <= 2e-4; the greedy decode to a
plain per-utterance loop in fp64.  With the weight None the Runner's step is the one it took before the switch existed;
with 0.0 the shared parameters end up the same; with 0.5 the gradient that reaches the joint logits is 0.5 / batch_size
times the fp64 reference's."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from nn_conformer_for_speech_recognition_amd import transducer
from nn_conformer_for_speech_recognition_amd.transducer import TransducerHead
from tests import rnnt_ref as rr
from tests.lstm_batched_ref import ref as lstm_ref
from tests.test_gpu_runner_mwer import _dataset, _hp, _same_parameters, _seed, _train_as_before, _vocab

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLANK = 2
ENC, NTOK, EMBED, HIDDEN, JOINT = 24, 12, 16, 32, 20


class _Head64(nn.Module):
    """The head restated in fp64 torch on the CPU, the prediction network a torch.nn.LSTM run per utterance."""

    def __init__(self, head):
        super().__init__()
        self.blank = head.blank
        self.embedding = nn.Embedding(NTOK, EMBED)
        self.prediction = nn.LSTM(EMBED, HIDDEN)
        self.enc_proj, self.pred_proj, self.out = nn.Linear(ENC, JOINT), nn.Linear(HIDDEN, JOINT), nn.Linear(JOINT, NTOK)
        self.double()
        self.load_state_dict({k: v.detach().double().cpu() for k, v in head.state_dict().items()})

    def joint_logits(self, enc, targets, tls):
        ids = torch.cat([torch.full((targets.shape[0], 1), self.blank), targets], 1)
        pred = lstm_ref(self.prediction, self.embedding(ids), [t + 1 for t in tls])[0]
        return self.out(torch.tanh(self.enc_proj(enc).unsqueeze(2) + self.pred_proj(pred).unsqueeze(1)))


def _head(seed=0, out_scale=1.0, blank_bias=0.0):
    torch.manual_seed(seed)
    head = TransducerHead(ENC, NTOK, BLANK, embed=EMBED, hidden=HIDDEN, joint=JOINT)
    with torch.no_grad():
        head.out.weight.mul_(out_scale)
        head.out.bias[BLANK] += blank_bias
    return head.to(DEV)


def _problem(B=3, T=11, U=5, seed=1):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, T, ENC, generator=g)
    allowed = torch.tensor([v for v in range(NTOK) if v != BLANK])
    targets = allowed[torch.randint(0, NTOK - 1, (B, U), generator=g)]
    return enc, targets, [T, 7, 1][:B], [U, 0, 3][:B]


def test_head_loss_equals_the_reference_on_its_own_logits():
    head = _head()
    enc, targets, ils, tls = _problem()
    il, tl = torch.tensor(ils, device=DEV), torch.tensor(tls, device=DEV)
    with torch.no_grad():
        logits = head.joint_logits(enc.to(DEV), targets.to(DEV), tl)
        loss = head(enc.to(DEV), il, targets.to(DEV), tl)
    assert logits.shape == (3, 11, 6, NTOK) and logits.dtype == torch.float32 and loss.shape == (3,)
    want = rr.reference(logits.cpu().numpy(), targets.numpy(), ils, tls, BLANK)
    err = np.abs(-loss.cpu().double().numpy() - want["ll"])
    assert (err <= 1e-5 * np.abs(want["ll"]) + 1e-6).all(), err
    # host lengths and None give the same logits / the full lattice
    assert torch.equal(head.joint_logits(enc.to(DEV), targets.to(DEV), tls), logits)
    full = head(enc.to(DEV), None, targets.to(DEV), None)
    assert torch.equal(full, head(enc.to(DEV), [11] * 3, targets.to(DEV), [5] * 3)) and full.requires_grad


def test_head_parameter_gradients_against_fp64():
    head = _head()
    enc, targets, ils, tls = _problem()
    x = enc.to(DEV).requires_grad_()
    head(x, torch.tensor(ils, device=DEV), targets.to(DEV), torch.tensor(tls, device=DEV)).sum().backward()
    h64 = _Head64(head)
    x64 = enc.double().requires_grad_()
    logits = h64.joint_logits(x64, targets, tls)
    want = rr.reference(logits.detach().numpy(), targets.numpy(), ils, tls, BLANK)
    logits.backward(torch.from_numpy(want["grad"]))          # d (sum_b -ll_b) / d logits, the pinned closed form
    errs = {"enc": ((x.grad.double().cpu() - x64.grad).norm() / x64.grad.norm()).item()}
    ref_grads = dict(h64.named_parameters())
    for k, p in head.named_parameters():
        g64 = ref_grads[k].grad
        assert g64.norm() > 0, k
        errs[k] = ((p.grad.double().cpu() - g64).norm() / g64.norm()).item()
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert set(errs) == {"enc"} | set(ref_grads) and len(errs) == 12
    for k, v in errs.items():
        assert v <= 2e-4, (k, v)


def _greedy64(h64, enc, lens, max_symbols):
    """Time-synchronous greedy search, utterance by utterance, in fp64 -> (token lists, the smallest top-2 margin)."""
    out, margin = [], np.inf
    with torch.no_grad():
        ep = h64.enc_proj(enc)
        for b in range(enc.shape[0]):
            _, state = h64.prediction(h64.embedding(torch.tensor([h64.blank])))
            toks = []
            for t in range(lens[b]):
                for _ in range(max_symbols):
                    logits = h64.out(torch.tanh(ep[b, t] + h64.pred_proj(state[0][0])))
                    top = logits.topk(2).values
                    margin = min(margin, float(top[0] - top[1]))
                    tok = int(logits.argmax())
                    if tok == h64.blank:
                        break
                    toks.append(tok)
                    _, state = h64.prediction(h64.embedding(torch.tensor([tok])), state)
            out.append(toks)
    return out, margin


@pytest.mark.parametrize("max_symbols", [1, 2, 3])
def test_greedy_decode_equals_the_plain_loop(max_symbols):
    head = _head(seed=3, out_scale=12.0, blank_bias=4.0)
    enc = torch.randn(4, 9, ENC, generator=torch.Generator().manual_seed(8))
    lens = [9, 4, 0, 6]
    want, margin = _greedy64(_Head64(head), enc.double(), lens, max_symbols)
    assert margin > 1e-3, margin
    tokens, counts = head.greedy_decode(enc.to(DEV), torch.tensor(lens, device=DEV), max_symbols=max_symbols)
    assert tokens.shape == (4, 9 * max_symbols) and tokens.dtype == torch.int32 and counts.dtype == torch.int32
    assert counts.tolist() == [len(w) for w in want]
    for b, w in enumerate(want):
        assert tokens[b, :len(w)].tolist() == w and bool((tokens[b, len(w):] == -1).all()), b
    assert want[2] == [] and 0 < sum(len(w) for w in want) < sum(lens) * max_symbols     # blanks and labels both occur
    # host lengths and None; no host synchronisation with device lengths
    assert torch.equal(head.greedy_decode(enc.to(DEV), lens, max_symbols=max_symbols)[0], tokens)
    assert torch.equal(head.greedy_decode(enc.to(DEV)[:1], None, max_symbols=max_symbols)[0], tokens[:1])
    dl, de = torch.tensor(lens, device=DEV), enc.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = head.greedy_decode(de, dl, max_symbols=max_symbols)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again[0], tokens) and torch.equal(again[1], counts)


# ------------------------------------------------------------------------------------------------ ASRNN
def _model(weight="unset", seed=4, **kw):
    from nn_conformer_for_speech_recognition_amd.lib.standard.asrnn import ASRNN
    vocab = _vocab()
    hp = _hp(vocab)
    if weight != "unset":
        hp.set_transducer(weight, **kw)
    ds = _dataset(hp, vocab, 31)
    torch.manual_seed(seed)
    return vocab, hp, ds, ASRNN(hp)


def test_hparams_switch():
    hp = _hp(_vocab())
    assert hp.transducer_weight is None
    hp.set_transducer(0.25, embed=32, hidden=64, joint=48)
    assert (hp.transducer_weight, hp.transducer_embed, hp.transducer_hidden, hp.transducer_joint) == (0.25, 32, 64, 48)
    hp.set_transducer(None)
    assert hp.transducer_weight is None and (hp.transducer_embed, hp.transducer_hidden, hp.transducer_joint) == (128, 256, 256)
    for hidden in (0, 12, 1032):
        with pytest.raises(ValueError, match="hidden"):
            hp.set_transducer(1.0, hidden=hidden)


def test_asrnn_without_the_option_is_unchanged_and_with_it_returns_the_encoder():
    _, hp0, ds, plain = _model()
    _, _, _, none = _model(None)
    _, hp1, _, with_head = _model(0.5, embed=32, hidden=64, joint=48)
    s0, s1 = plain.state_dict(), with_head.state_dict()
    assert not hasattr(plain, "transducer") and not hasattr(none, "transducer")
    assert not any("transducer" in k for k in s0) and list(none.state_dict()) == list(s0)
    extra = [k for k in s1 if k not in s0]
    assert list(s1)[:len(s0)] == list(s0) and extra and all(k.startswith("transducer.") for k in extra)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)          # the head is built last: the same initial values
    assert isinstance(with_head.transducer, TransducerHead) and with_head.transducer.blank == hp1.blank_idx
    assert with_head.transducer.out.out_features == hp1.ntokens and with_head.transducer.prediction.hidden_size == 64
    batch = ds.get_batch(1, "train")          # the short last batch: two clips, two padding rows
    mels, tau = batch["input"]["mels"], batch["input"]["tau"]
    outs = []
    for m in (plain, with_head):
        m.to(DEV).eval()
        with torch.no_grad():
            outs.append(m(mels, tau))
    assert len(outs[0]) == 2 and len(outs[1]) == 2
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with torch.no_grad():
        x, lens, (enc, enc_lens) = with_head(mels, tau, return_encoder=True)
        xp, lensp, (encp, _) = plain(mels, tau, return_encoder=True)
    assert torch.equal(x, outs[0][0]) and torch.equal(lens, outs[0][1]) and torch.equal(enc, encp)
    B, T_enc = x.shape[:2]
    assert enc.shape == (B, T_enc, hp1.projection_out_size) and B == hp1.batch_size
    assert enc_lens.shape == (B,) and enc_lens.dtype == torch.int32 and enc_lens.is_cuda
    assert torch.equal(enc_lens, with_head.decoder_lengths(lens.to(DEV), B, T_enc))
    assert bool((enc_lens >= 0).all()) and bool((enc_lens <= T_enc).all()) and int(enc_lens.max()) > 1


# ------------------------------------------------------------------------------------------------ Runner
def _fresh(weight="unset", mwer=None):
    from nn_conformer_for_speech_recognition_amd.lib.standard.runner import Runner
    vocab, hp, ds, m = _model(weight, embed=32, hidden=64, joint=48) if weight not in ("unset", None) else _model(weight)
    if mwer is not None:
        hp.set_mwer(mwer, 3)
    with torch.no_grad():
        m.final_fc.weight.mul_(8.0)          # (as tests/test_gpu_runner_mwer.py's starting point)
    return vocab, hp, ds, Runner(m, hp)


@pytest.fixture(scope="module")
def trained_before():
    _, _, ds, runner = _fresh()
    _seed()
    _train_as_before(runner, ds, 1)
    return runner


def test_weight_none_is_the_step_as_before(trained_before, monkeypatch):
    _, hp, ds, runner = _fresh(None)
    monkeypatch.setattr(runner, "_rnnt", lambda *a, **k: pytest.fail("the transducer term with the weight None"))
    _seed()
    runner.train(ds, 1)
    assert _same_parameters(runner, trained_before)
    assert runner.history == trained_before.history and set(runner.history) == {"loss", "metric", "val_loss",
                                                                                 "val_metric"}
    assert np.isfinite(runner.history["loss"][0])


def test_weight_zero_leaves_the_shared_parameters_as_with_none(trained_before):
    _, hp, ds, runner = _fresh(0.0)
    _seed()
    runner.train(ds, 1)
    sa, sb = runner.model.state_dict(), trained_before.model.state_dict()
    assert set(sb) < set(sa)
    assert all(torch.equal(sa[k], sb[k]) for k in sb)
    assert runner.history["loss"] == trained_before.history["loss"]
    assert len(runner.history["rnnt"]) == 1 and np.isfinite(runner.history["rnnt"][0])
    assert runner.history["rnnt"][0] > 0.0          # the term itself is there, its weight is 0


def test_weight_set_without_a_head_raises():
    _, hp, ds, runner = _fresh()
    hp.set_transducer(0.5)
    with pytest.raises(ValueError, match="before the model is built"):
        runner.train(ds, 1)


@pytest.fixture(scope="module")
def half():
    return _fresh(0.5)


@pytest.mark.parametrize("device_wer", [False, True])
def test_weight_half_gradient_at_the_joint_logits(half, monkeypatch, device_wer):
    vocab, hp, ds, runner = half
    hp.set_device_wer(device_wer)
    steps = []
    loss_fn, step = transducer.rnnt_loss, runner.optimizer.step

    def loss_spy(logits, targets, logit_lengths, target_lengths, **kw):
        logits.retain_grad()
        steps.append(dict(logits=logits, targets=targets, il=logit_lengths, tl=target_lengths, kw=kw))
        return loss_fn(logits, targets, logit_lengths, target_lengths, **kw)

    def step_spy(*a, **k):
        steps[-1]["grad"] = steps[-1]["logits"].grad.clone()
        return step(*a, **k)

    monkeypatch.setattr(transducer, "rnnt_loss", loss_spy)
    monkeypatch.setattr(runner.optimizer, "step", step_spy)
    n0 = len(runner.history["loss"])
    try:
        _seed()
        runner.train(ds, 1)
    finally:
        hp.set_device_wer(False)
    assert len(steps) == 2 and len(runner.history["rnnt"]) == n0 + 1 == len(runner.history["loss"])
    assert np.isfinite(runner.history["rnnt"][-1]) and np.isfinite(runner.history["loss"][-1])
    assert set(runner.history) == {"loss", "metric", "val_loss", "val_metric", "rnnt"}
    total = 0.0
    saw_empty_target = saw_padded_row = False
    for s in steps:
        x = s["logits"].detach()
        B, T, U1, V = x.shape
        assert B == hp.batch_size and V == hp.ntokens and s["kw"]["zero_infinity"] and s["kw"]["blank"] == vocab.blank_idx
        ils, tls = s["il"].clamp(0, T).tolist(), s["tl"].clamp(0, U1 - 1).tolist()
        args = (x.cpu().numpy(), s["targets"].cpu().numpy(), ils, tls, vocab.blank_idx)
        ref, ref32 = rr.reference(*args), rr.reference(*args, dtype=np.float32)
        total += -ref["ll"][np.isfinite(ref["ll"])].sum() / B
        saw_empty_target |= any(t == 0 and i > 0 for t, i in zip(tls, ils))
        saw_padded_row |= 0 in ils
        w = 0.5 / hp.batch_size          # (a power of two: the scaling is exact)
        got = s["grad"].double().cpu().numpy() / w
        e, e32 = np.abs(got - ref["grad"]).max(), np.abs(ref32["grad"] - ref["grad"]).max()
        bound = 2 * e32 + 1e-7 * np.abs(ref["grad"]).max()
        print(f"  device_wer {device_wer}: err {e:.3g}  fp32 reference err {e32:.3g}  bound {bound:.3g}"
              f"  max |ref| {np.abs(ref['grad']).max():.3g}")
        assert e <= bound, (e, e32, bound)
    assert saw_empty_target and saw_padded_row
    assert abs(runner.history["rnnt"][-1] - total / 2) <= 1e-4 * max(1.0, abs(total / 2))


def test_together_with_mwer():
    _, hp, ds, runner = _fresh(0.5, mwer=0.5)
    _seed()
    runner.train(ds, 1)
    assert set(runner.history) == {"loss", "metric", "val_loss", "val_metric", "mwer", "rnnt"}
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in runner.history.values())


def test_finetune_runs_under_the_flag():
    from nn_conformer_for_speech_recognition_amd.lib.finetuning.finetune import FineTune
    from nn_conformer_for_speech_recognition_amd.lib.standard.asrnn import ASRNN
    vocab = _vocab()
    hp = _hp(vocab, dropout=0.1)
    hp.ft_epochs, hp.ft_train_epochs, hp.nst = 1, 1, True
    hp.set_transducer(0.5, embed=32, hidden=64, joint=48)
    hp.set_device_wer(True)
    ds = _dataset(hp, vocab, 9)
    U = _dataset(hp, vocab, 10, n_unlab=5)
    torch.manual_seed(0)
    runner = FineTune(hp).fine_tuning(ASRNN(hp), ds, U)
    assert len(runner.history["loss"]) == 2 and len(runner.history["rnnt"]) == 2
    assert all(np.isfinite(x) for k in runner.history for x in runner.history[k])
