"""ASRNN with hp.decoder_batched: the BiLSTM decoder runs one sequence per utterance, bounded by the Conformer's own
frame counts.  Small frame-mode configuration of tests/test_gpu_nst.py (L 1, d 144, 4 heads, ffn 576, K 15, B 4,
T 201 mels, ragged clips).  Eval parity is fp32 against tests/lstm_batched_ref.ref (float64 torch.nn.LSTM per
utterance) on the model's own encoder output: relative L2 <= 1e-4 over the valid frames (the bound of the
reference-fixture ASRNN test), and equal argmax ids wherever the top-2 margin exceeds 1e-3."""
import numpy as np
import pytest
import torch

from nn_conformer_for_speech_recognition_amd.lib.finetuning.finetune import FineTune
from nn_conformer_for_speech_recognition_amd.lib.standard.asrnn import ASRNN
from nn_conformer_for_speech_recognition_amd.lib.standard.runner import Runner
from tests.lstm_batched_ref import ref
from tests.test_gpu_nst import _dataset, _hp, _vocab

pytestmark = pytest.mark.gpu


def _model(cd, seed):
    vocab = _vocab()
    hp = _hp(vocab, 1, 144, 4, 576, 15, cd, 4)
    hp.set_decoder_batched(True)
    ds = _dataset(hp, vocab, 6, 5, 201, 9)
    torch.manual_seed(seed)
    m = ASRNN(hp).to(hp.device)
    return hp, ds, m


def test_eval_output_is_the_per_utterance_decoder_and_flag_off_is_todays_path():
    hp, ds, m = _model("fp32", 0)
    m.eval()
    with torch.no_grad():
        m.final_fc.weight.mul_(8.0)                         # sharper posteriors: fewer near-tied frames
        batch = ds.get_batch(0, "train")["input"]
        x, tau = batch["mels"], batch["tau"]
        B = x.shape[0]
        out, out_lens = m(x, tau)
        enc, lens = m.encoder(x.unsqueeze(1), tau)
        T_enc = enc.shape[0] // B
        lens_l = [int(v) for v in lens.tolist()]
        assert out.shape[:2] == (B, T_enc) and torch.equal(out_lens.cpu(), lens.cpu())
        assert len(set(lens_l)) > 1 and all(1 <= n <= T_enc for n in lens_l)      # ragged, inside the clamps
        assert m.decoder_lengths(lens, B, T_enc).tolist() == lens_l

        lstm64 = torch.nn.LSTM(256, 128, bidirectional=True).double()
        lstm64.load_state_dict({k: v.double().cpu() for k, v in m.lstm.state_dict().items()})
        y = ref(lstm64, enc.view(B, T_enc, -1).double().cpu(), lens_l)[0]
        w, b = m.final_fc.weight.double().cpu(), m.final_fc.bias.double().cpu()
        want = torch.log_softmax(y @ w.t() + b, -1)
        got = out.double().cpu()
        valid = torch.arange(T_enc)[None, :] < torch.tensor(lens_l)[:, None]
        rel = ((got - want)[valid].norm() / want[valid].norm()).item()
        top2 = want.topk(2, -1).values
        sure = valid & ((top2[..., 0] - top2[..., 1]) > 1e-3)
        print("rel", rel, "valid frames", int(valid.sum()), "of them compared by argmax", int(sure.sum()))
        assert rel <= 1e-4
        assert sure.sum().item() > 0.5 * valid.sum().item()
        assert torch.equal(got.argmax(-1)[sure], want.argmax(-1)[sure])

        # the flag off: the same model object runs today's path, one sequence over the batch
        hp.set_decoder_batched(False)
        off, _ = m(x, tau)
        today = m.log_softmax(m.final_fc(m.lstm(enc)[0]).view(B, T_enc, -1))
        assert torch.equal(off, today)
        assert not torch.equal(off, out)


def test_runner_and_finetune_under_the_flag():
    hp, ds, m = _model("bf16", 0)
    hp.ft_epochs, hp.ft_train_epochs, hp.nst = 1, 1, True
    U = _dataset(hp, _vocab(), 1, 5, 201, 10)
    r = Runner(m, hp)
    r.train(ds, 1)
    assert len(r.history["loss"]) == 1 and np.isfinite(r.history["loss"][0])
    loss, metric = r.test(ds, "validation")
    assert np.isfinite(loss) and 0.0 <= metric
    labels = r.generate_labels(U)
    assert len(labels) >= 5 and all(s is not None for s in labels)
    runner = FineTune(hp).fine_tuning(m, ds, U)
    assert "mix" in ds.data and len(ds.data["mix"]) >= len(ds.data["train"])
    assert len(runner.history["loss"]) >= 2 and all(np.isfinite(v) for v in runner.history["loss"])
