"""Runner.train with hp.mwer_weight (HParams.set_mwer): ctc + weight * mean_b(mwer_b), the MWER term from
ctc.mwer_loss on the step's own logits.  With the weight None the step is the one the Runner took before the switch
existed (restated here); with 0.0 the term contributes exact zeros; with 0.5 the gradient that reaches the logits is
the CTC gradient plus 0.5 / batch_size times the fp64 reference's gradient (tests/ctc_nbest_ref.py) on the device's own
n-best list, within the bound of tests/test_gpu_ctc_nbest.py."""
import random
from math import ceil, isnan
from statistics import mean

import numpy as np
import pytest
import torch
import torch.nn as nn

from nn_conformer_for_speech_recognition_amd import ctc
from tests import ctc_nbest_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORDS = "yes no up down left right on off stop go zero one two three four five six seven eight nine".split()


def _vocab():
    from nn_conformer_for_speech_recognition_amd.lib.standard.myvocab import build_vocab
    return build_vocab([" ".join(WORDS)])


def _hp(vocab, B=4, dropout=0.0):
    from nn_conformer_for_speech_recognition_amd.lib.hparams import HParams
    hp = HParams(None)
    hp.batch_size = B
    hp.standard_linear_nodes, hp.mhsa_num_heads, hp.conformer_ff1_linear1_nodes = 144, 4, 576
    hp.conformer_depthwise_conv_kernel, hp.n_conformers, hp.dropout = 15, 1, dropout
    hp.frontend_proj, hp.compute_dtype = "frame", "bf16"
    hp.projection_out_size, hp.standard_decoder_nodes = 256, 128
    hp.set_blank_index(vocab.blank_idx)
    hp.device = torch.device(DEV)
    hp.plots_dir = None
    return hp


def _dataset(hp, vocab, seed, n_unlab=0):
    """train: 6 clips (a last batch of 2 at batch size 4), one with an empty transcript; validation: 2."""
    from nn_conformer_for_speech_recognition_amd.lib.standard.speechcommands import MelDataset
    rng = np.random.default_rng(seed)
    T = 201

    def mk(n, words=3, empty=()):
        return [(rng.random((80, int(T - rng.integers(0, T // 3))), dtype=np.float32),
                 "" if i in empty else " ".join(rng.choice(WORDS, words))) for i in range(n)]
    splits = {"train": mk(6, empty=(2,)), "validation": mk(2)}
    if n_unlab:
        splits["pretrain"] = [(m, None) for m, _ in mk(n_unlab)]
    return MelDataset(hp, vocab, splits)


def _fresh(weight="unset", nbest=4):
    """A Runner over a freshly seeded model and dataset: every call gives the same starting point."""
    from nn_conformer_for_speech_recognition_amd.lib.standard.asrnn import ASRNN
    from nn_conformer_for_speech_recognition_amd.lib.standard.runner import Runner
    vocab = _vocab()
    hp = _hp(vocab)
    if weight != "unset":
        hp.set_mwer(weight, nbest)
    ds = _dataset(hp, vocab, 31)
    torch.manual_seed(4)
    m = ASRNN(hp)
    with torch.no_grad():
        m.final_fc.weight.mul_(8.0)          # confident frames: hypotheses that are not all blank
    return vocab, hp, ds, Runner(m, hp)


def _seed():
    random.seed(11)
    torch.manual_seed(11)


def _train_as_before(runner, train_set, epochs):
    """Runner.train's host-metric branch as it stood before hp.mwer_weight (no validation split handling changed)."""
    self = runner
    train_size = ceil(len(train_set.idxes["train"]) / self.hp.batch_size)
    for _ in range(epochs):
        self.model.train()
        train_set.shuffle("train")
        eloss, emetric = [], []
        for i in range(train_size):
            batch = train_set.get_batch(i, "train")
            inbatch, input_lens = batch["input"]["mels"], batch["input"]["tau"]
            target, target_lens = batch["target"]["transcripts"], batch["target"]["lens"]
            self.optimizer.zero_grad()
            logits, output_lengths = self.model(inbatch, input_lens, False, finetuning=False)
            output_lengths = nn.functional.pad(output_lengths, (0, self.hp.batch_size - output_lengths.shape[0]))
            output_lengths = output_lengths.clamp(max=logits.shape[1])
            loss = self.loss(logits.transpose(0, 1), target, output_lengths, target_lens)
            cur = loss.item()
            loss.backward()
            self.optimizer.step()
            eloss.append(cur)
            emetric.append(self._metric(train_set, logits.detach(), target, output_lengths))
        self.history["loss"].append(mean([100 if isnan(x) else x for x in eloss]))
        self.history["metric"].append(mean(emetric) if emetric else float("nan"))
        vl, vm = self.test(train_set, "validation", finetuning=False)
        self.history["val_loss"].append(vl)
        self.history["val_metric"].append(vm)


def _same_parameters(a, b):
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert sa.keys() == sb.keys()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.fixture(scope="module")
def trained_before():
    _, _, ds, runner = _fresh()
    _seed()
    _train_as_before(runner, ds, 1)
    return runner


def test_hparams_switch():
    vocab = _vocab()
    hp = _hp(vocab)
    assert hp.mwer_weight is None and hp.mwer_nbest == 4
    hp.set_mwer(0.25, nbest=6)
    assert hp.mwer_weight == 0.25 and hp.mwer_nbest == 6
    hp.set_mwer(None)
    assert hp.mwer_weight is None and hp.mwer_nbest == 4
    with pytest.raises(ValueError):
        hp.set_mwer(1.0, nbest=0)


def test_weight_none_is_the_step_as_before(trained_before, monkeypatch):
    _, hp, ds, runner = _fresh(None)
    monkeypatch.setattr(runner, "_mwer", lambda *a, **k: pytest.fail("the MWER term with the weight None"))
    _seed()
    runner.train(ds, 1)
    assert _same_parameters(runner, trained_before)
    assert runner.history == trained_before.history and set(runner.history) == {"loss", "metric", "val_loss",
                                                                                 "val_metric"}
    assert np.isfinite(runner.history["loss"][0])


def test_weight_zero_contributes_exact_zeros(trained_before):
    _, hp, ds, runner = _fresh(0.0)
    _seed()
    runner.train(ds, 1)
    assert _same_parameters(runner, trained_before)
    assert runner.history["loss"] == trained_before.history["loss"]
    assert len(runner.history["mwer"]) == 1 and np.isfinite(runner.history["mwer"][0])
    assert runner.history["mwer"][0] != 0.0          # the term itself is there, its weight is 0


@pytest.fixture(scope="module")
def half():
    return _fresh(0.5)


@pytest.mark.parametrize("device_wer,beam_size", [(False, 0), (False, 4), (True, 0), (True, 4)])
def test_weight_half_gradient_is_ctc_plus_half_the_reference(half, monkeypatch, device_wer, beam_size):
    vocab, hp, ds, runner = half
    hp.set_device_wer(device_wer)
    hp.set_beam_size(beam_size)
    steps = []
    mwer, step = runner._mwer, runner.optimizer.step

    def mwer_spy(voc, logits, target, target_lens, lengths):
        logits.retain_grad()
        steps.append(dict(logits=logits, target=target, tl=target_lens, lengths=lengths))
        return mwer(voc, logits, target, target_lens, lengths)

    def step_spy(*a, **k):
        steps[-1]["grad"] = steps[-1]["logits"].grad.clone()
        return step(*a, **k)

    monkeypatch.setattr(runner, "_mwer", mwer_spy)
    monkeypatch.setattr(runner.optimizer, "step", step_spy)
    n0 = len(runner.history["loss"])
    try:
        _seed()
        runner.train(ds, 1)
    finally:
        hp.set_device_wer(False)
        hp.set_beam_size(0)
    assert len(steps) == 2 and len(runner.history["mwer"]) == n0 + 1 == len(runner.history["loss"])
    assert np.isfinite(runner.history["mwer"][-1]) and np.isfinite(runner.history["loss"][-1])
    total = 0.0
    saw_empty_target = saw_padded_row = False
    for s in steps:
        x = s["logits"].detach().float()
        B, T, V = x.shape
        assert B == hp.batch_size
        il = s["lengths"].clamp(0, T)
        # the CTC part, from the same kernels on the same logits
        xc = x.clone().requires_grad_()
        ctc.ctc_loss(xc.transpose(0, 1), s["target"], s["lengths"], s["tl"], blank=vocab.blank_idx,
                     zero_infinity=True).backward()
        # the MWER part, from the fp64 reference on the device's own n-best list
        tokens, lens, scores = ctc.beam_search_decode(x, il, beam_size=max(beam_size, 4), blank=vocab.blank_idx,
                                                      pad=vocab.pad_idx, nbest=4)
        risk = ctc.edit_distance(tokens, s["target"], lens, s["tl"]).distance
        tokens, lens, scores = tokens.cpu(), lens.cpu(), scores.cpu()
        hyps = [[None if scores[b, n] == -np.inf else tokens[b, n, :int(lens[b, n])].tolist() for n in range(4)]
                for b in range(B)]
        args = (x.cpu().numpy(), il.tolist(), hyps, risk.cpu().tolist(), vocab.blank_idx, min(T, 511))
        ref, ref32 = nr.reference(*args), nr.reference(*args, dtype=torch.float32)
        total += ref["loss"].sum() / B
        saw_empty_target |= bool((s["tl"] == 0).any())
        saw_padded_row |= bool((il == 0).any())
        w = 0.5 / hp.batch_size
        got = (s["grad"].float() - xc.grad).double().cpu().numpy() / w
        e = np.abs(got - ref["grad"]).max()
        e32 = np.abs(ref32["grad"] - ref["grad"]).max()
        # + the one fp32 addition autograd makes when it adds the two gradients (and this test's subtraction)
        bound = 2 * e32 + 1e-7 * np.abs(ref["grad"]).max() + 2.0 ** -22 * float(s["grad"].abs().max()) / w
        print(f"  device_wer {device_wer} beam {beam_size}: err {e:.3g}  fp32 reference err {e32:.3g}  bound {bound:.3g}"
              f"  max |ref| {np.abs(ref['grad']).max():.3g}")
        assert e <= bound, (e, e32, bound)
    assert saw_empty_target and saw_padded_row
    assert abs(runner.history["mwer"][-1] - total / 2) <= 1e-4 * max(1.0, abs(total / 2))


def test_finetune_runs_under_the_flag():
    from nn_conformer_for_speech_recognition_amd.lib.finetuning.finetune import FineTune
    from nn_conformer_for_speech_recognition_amd.lib.standard.asrnn import ASRNN
    vocab = _vocab()
    hp = _hp(vocab, dropout=0.1)
    hp.ft_epochs, hp.ft_train_epochs, hp.nst = 1, 1, True
    hp.set_mwer(0.5, nbest=3)
    hp.set_device_wer(True)
    ds = _dataset(hp, vocab, 9)
    U = _dataset(hp, vocab, 10, n_unlab=5)
    torch.manual_seed(0)
    runner = FineTune(hp).fine_tuning(ASRNN(hp), ds, U)
    assert len(runner.history["loss"]) == 2 and len(runner.history["mwer"]) == 2
    assert all(np.isfinite(x) for k in runner.history for x in runner.history[k])
