"""CPU side of the per-utterance (batched) LSTM decoder: the fp64 reference of the GPU tests pinned against torch's
packed-sequence call, the reason the feature exists, the HParams switch, LSTM.forward's argument checks (raised
before any device work) and the header / binding entries."""
import os

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from nn_conformer_for_speech_recognition_amd import _lib
from nn_conformer_for_speech_recognition_amd.lib.hparams import HParams
from nn_conformer_for_speech_recognition_amd.lstm import LSTM
from tests.lstm_batched_ref import ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("cfm_lstm_batched_ws_bytes", "cfm_lstm_batched_fwd", "cfm_lstm_batched_bwd")


def _case(layers=1):
    torch.manual_seed(11)
    lstm = torch.nn.LSTM(6, 8, num_layers=layers, bidirectional=True).double()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(3, 5, 6, generator=g, dtype=torch.float64)
    dy = torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
    return lstm, x, dy, [5, 2, 4]


@pytest.mark.parametrize("layers", [1, 2])
def test_ref_equals_packed_sequence(layers):
    lstm, x, dy, lens = _case(layers)
    xa = x.clone().requires_grad_(True)
    ya, ha, ca = ref(lstm, xa, lens)
    (ya * dy).sum().backward()
    xb = x.clone().requires_grad_(True)
    packed = pack_padded_sequence(xb.transpose(0, 1), torch.tensor(lens), enforce_sorted=False)
    yp, (hb, cb) = lstm(packed)
    yb = pad_packed_sequence(yp, total_length=5)[0].transpose(0, 1)
    (yb * dy).sum().backward()
    for a, b in ((ya, yb), (ha, hb), (ca, cb), (xa.grad, xb.grad)):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 1e-12
    for t in range(3):                      # zeros at padding, in the output and in the input gradient
        assert ya[t, lens[t]:].abs().sum().item() == 0 and xa.grad[t, lens[t]:].abs().sum().item() == 0


def test_ref_zero_length_row():
    lstm, x, _, _ = _case()
    y, h, c = ref(lstm, x, [0, 5, 1])
    assert y.shape == (3, 5, 16) and h.shape == (2, 3, 8) and c.shape == (2, 3, 8)
    assert y[0].abs().sum().item() == 0 and h[:, 0].abs().sum().item() == 0 and c[:, 0].abs().sum().item() == 0
    assert y[1].abs().min().item() > 0


def test_one_sequence_call_differs_from_per_utterance():
    """The reference's decoder call (the 2-D (B*T, In) input = ONE sequence over the batch) is not the per-utterance
    LSTM: utterance b starts from utterance b-1's last state, and the reverse direction leaks the other way."""
    lstm, x, _, _ = _case()
    with torch.no_grad():
        y, _, _ = ref(lstm, x, [5, 5, 5])
        y1 = lstm(x.reshape(15, 6))[0].view(3, 5, 16)
    assert (y - y1).abs().max().item() > 1e-3


def test_hparams_decoder_batched_switch():
    hp = HParams(None)
    assert hp.decoder_batched is False
    hp.set_decoder_batched(1)
    assert hp.decoder_batched is True
    hp.set_decoder_batched(False)
    assert hp.decoder_batched is False


def test_forward_argument_checks_need_no_device():
    m = LSTM(6, 8, bidirectional=True)
    with pytest.raises(ValueError):
        m(torch.zeros(5, 6), lengths=[5])                    # lengths with the unbatched 2-D form
    with pytest.raises(ValueError):
        m(torch.zeros(5, 3, 6), lengths=[5, 5])              # 3 sequences, 2 lengths
    with pytest.raises(ValueError):
        m(torch.zeros(5, 3, 6), lengths=torch.tensor([5, 5, 5, 5]))
    with pytest.raises(ValueError):
        m(torch.zeros(5, 3, 6), lengths=[5, -1, 2])          # a negative host length
    with pytest.raises(NotImplementedError):
        m(torch.zeros(5, 3, 6), hx=(torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)))
    with pytest.raises(NotImplementedError):
        m(pack_padded_sequence(torch.zeros(5, 3, 6), torch.tensor([5, 4, 1])))
    with pytest.raises(NotImplementedError):
        LSTM(6, 8, proj_size=4)


def test_header_and_bindings_name_the_batched_entry_points():
    src = open(os.path.join(REPO, "include", "cfm.h")).read()
    for sym in SYMS:
        assert sym + "(" in src, sym
        assert sym in _lib._SIGS and sym in _lib.EXPORTED, sym
    assert _lib._SIGS[SYMS[0]][0] is _lib.c_size_t and len(_lib._SIGS[SYMS[0]][1]) == 4
    assert len(_lib._SIGS[SYMS[1]][1]) == 15 and len(_lib._SIGS[SYMS[2]][1]) == 14
