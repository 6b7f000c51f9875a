"""Reference of the per-utterance (batched) LSTM: torch.nn.LSTM in float64, run utterance by utterance on each
utterance's own valid frames.  tests/test_lstm_batched_cpu.py pins it against torch's packed-sequence call."""
import torch


def ref(lstm64, x, lengths):
    """lstm64: a float64 torch.nn.LSTM (any layers / directions, batch_first irrelevant); x (B, T, In) float64,
    batch-major; lengths: B ints in [0, T].  Returns (y (B, T, ndir*H) zero at padding, h_n, c_n (layers*ndir, B, H));
    a zero-length row is all zeros.  Differentiable with respect to x and the parameters."""
    B, T, _ = x.shape
    ndir = 2 if lstm64.bidirectional else 1
    H, nstate = lstm64.hidden_size, lstm64.num_layers * ndir
    ys, hs, cs = [], [], []
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            ys.append(x.new_zeros(T, ndir * H))
            hs.append(x.new_zeros(nstate, H))
            cs.append(x.new_zeros(nstate, H))
            continue
        y, (h, c) = lstm64(x[b, :n])                       # 2-D input: one unbatched sequence of n steps
        ys.append(torch.cat([y, y.new_zeros(T - n, ndir * H)]))
        hs.append(h)
        cs.append(c)
    return torch.stack(ys), torch.stack(hs, 1), torch.stack(cs, 1)
