"""The oracle's mask provider (oracle/conformer.py): every dropout site of ConformerRef asks it in train mode, an
all-ones provider reproduces the dropout-free oracle exactly (outputs and every gradient, fp64), and a provider that
is not all ones is really applied, at the site it names and with the scale it returns.  CPU only."""
import pytest
import torch

from oracle import conformer as oc


def _run(ref, x, lens, gy):
    ref.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_()
    y, _ = ref(xr, lens)
    y.backward(gy)
    return y.detach(), xr.grad, {n: p.grad.clone() for n, p in ref.named_parameters()}


@pytest.mark.parametrize("pos,gn,conv_first", [("none", False, False), ("rel", False, True), ("none", True, False)])
def test_all_ones_provider_is_the_plain_oracle(pos, gn, conv_first):
    d, H, ffn, K, L, B, T = 32, 2, 48, 7, 2, 2, 11
    torch.manual_seed(3)
    plain = oc.ConformerRef(d, H, ffn, L, K, 0.0, use_group_norm=gn, convolution_first=conv_first, pos_enc=pos)
    plain = plain.double().train()
    seen = []

    def ones(site, shape):
        seen.append((site, shape))
        return torch.ones(shape, dtype=torch.float64)

    masked = oc.ConformerRef(d, H, ffn, L, K, 0.3, use_group_norm=gn, convolution_first=conv_first, pos_enc=pos,
                             mask_provider=ones).double().train()
    masked.load_state_dict(plain.state_dict())
    x = torch.randn(B, T, d, dtype=torch.float64)
    lens = torch.tensor([T, 6])
    gy = torch.randn(B, T, d, dtype=torch.float64)
    y0, gx0, g0 = _run(plain, x, lens, gy)
    y1, gx1, g1 = _run(masked, x, lens, gy)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    if not gn:
        for (n, b0), (_, b1) in zip(plain.named_buffers(), masked.named_buffers()):
            assert torch.equal(b0, b1), n
    want = {}
    for i in range(L):
        s = f"layers.{i}."
        want.update({s + "ffn1.act": (B, T, ffn), s + "ffn1.out": (B, T, d), s + "attn.probs": (B, H, T, T),
                     s + "attn.out": (B, T, d), s + "conv.out": (B, d, T), s + "ffn2.act": (B, T, ffn),
                     s + "ffn2.out": (B, T, d)})
    assert dict(seen) == want and len(seen) == len(want)       # every site once per forward, with its tensor's shape
    # eval mode and a removed provider never ask
    seen.clear()
    masked.eval()
    masked(x, lens)
    masked.train().set_mask_provider(None)
    for m in masked.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, oc.RelPosMHARef):
            m.dropout = 0.0
    y2, _ = masked(x, lens)
    assert not seen and torch.equal(y2.detach(), y0)


def test_a_real_mask_is_applied_where_it_says():
    """Dropping everything at one layer's ffn2.out with factor 2 elsewhere-ones: the layer equals the plain layer
    with that module's second Linear zeroed (weight and bias), and a 2x factor on attn.probs equals doubling the
    values; a dropped site passes no gradient to what feeds only it."""
    d, H, ffn, K, B, T = 16, 2, 24, 3, 2, 5
    torch.manual_seed(5)
    plain = oc.ConformerRef(d, H, ffn, 1, K, 0.0).double().train()
    x = torch.randn(B, T, d, dtype=torch.float64)
    lens = torch.tensor([T, 3])
    gy = torch.randn(B, T, d, dtype=torch.float64)

    def drop_ffn2(site, shape):
        return torch.zeros(shape, dtype=torch.float64) if site == "layers.0.ffn2.out" else torch.ones(shape).double()

    masked = oc.ConformerRef(d, H, ffn, 1, K, 0.1, mask_provider=drop_ffn2).double().train()
    masked.load_state_dict(plain.state_dict())
    y1, gx1, g1 = _run(masked, x, lens, gy)
    zeroed = oc.ConformerRef(d, H, ffn, 1, K, 0.0).double().train()
    zeroed.load_state_dict(plain.state_dict())
    with torch.no_grad():
        zeroed.conformer_layers[0].ffn2.sequential[4].weight.zero_()
        zeroed.conformer_layers[0].ffn2.sequential[4].bias.zero_()
    y0, gx0, _ = _run(zeroed, x, lens, gy)
    torch.testing.assert_close(y1, y0, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gx1, gx0, rtol=1e-12, atol=1e-12)
    assert g1["conformer_layers.0.ffn2.sequential.1.weight"].abs().max() == 0
    assert g1["conformer_layers.0.ffn1.sequential.1.weight"].abs().max() > 0

    def double_probs(site, shape):
        return torch.full(shape, 2.0 if site == "layers.0.attn.probs" else 1.0, dtype=torch.float64)

    masked.set_mask_provider(double_probs)
    y2, _, _ = _run(masked, x, lens, gy)
    doubled = oc.ConformerRef(d, H, ffn, 1, K, 0.0).double().train()
    doubled.load_state_dict(plain.state_dict())
    with torch.no_grad():       # 2 P V == P (2 V): double the value rows of the packed projection
        doubled.conformer_layers[0].self_attn.in_proj_weight[2 * d:] *= 2
        doubled.conformer_layers[0].self_attn.in_proj_bias[2 * d:] *= 2
    y3, _, _ = _run(doubled, x, lens, gy)
    torch.testing.assert_close(y2, y3, rtol=1e-12, atol=1e-12)
