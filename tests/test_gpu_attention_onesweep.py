"""The one-sweep whole-head dK/dV kernel (attn_bwd_dkdv_sweep_kernel, the default) against fp32 torch and against the
two-pass kernel it replaces (cfm_attn_set_mode ATTN_MODE_DKDV_TWO_PASS).

The sweep keeps the 32x32x16 MFMAs, the operand order and the query-step order of the two passes, so identity was not
given up: dK, dV and the stored dS^T are compared bit for bit between the two mode settings, and no error bound between
the kernels is needed.  Measured on MI355X for the record, relative Frobenius error against fp32 torch, worst of dQ /
dK / dV, one-sweep kernel | two-pass kernel (the same figure, because their outputs are the same bits), dropout 0 and 0.1:
    T 33  dk 64   2.68e-3 | 2.68e-3    2.68e-3 | 2.68e-3
    T 97  dk 64   2.48e-3 | 2.48e-3    2.51e-3 | 2.51e-3
    T 130 dk 64   2.49e-3 | 2.49e-3    2.41e-3 | 2.41e-3
    T 373 dk 64   2.50e-3 | 2.50e-3    2.52e-3 | 2.52e-3
    T 373 dk 36   2.51e-3 | 2.51e-3    2.53e-3 | 2.53e-3   (one and four workgroups per head alike)
The test prints the three errors of both kernels before it asserts.

Bound against torch (TOL): the reference reads the same bf16 q, k, v and dO and works in fp32, so the kernels' error is
their own roundings to bf16 -- P before dO^T P, dS before Q^T dS and the dS^T store, o before D = rowsum(dO o), and the
output -- each a relative error uniform in +-2^-9, RMS 2^-9 / sqrt(3) = 1.1e-3, independent from element to element.
Sums of products of such terms keep that relative RMS, and the four stages add in quadrature to 2.3e-3 in the relative
Frobenius norm; the fp32 accumulation and v_exp_f32 (1 ulp) are two orders below.  The bound is four times that, 1e-2:
half the 2e-2 the existing whole-tensor check allows, and far below what one wrong mask bit pattern (about 10 % of the
entries at p 0.1) or one dropped query step (1 / 12 of the sum at T 373) would cost.

Shapes: B 2, H 2, one full-length utterance and one shorter than a 32-key block (whole key blocks past len: zero
gradients, nothing stored).  Every shape runs with one workgroup per head (the flagship's launch: ceil(T / 32) waves,
12 at T 373; ATTN_MODE_REL_ZERO_FILL pins qs = 1, its only effect off the rel-pos path); the dk 36 shape also runs
with the plan's own split (qs > 1 on any device with at least 8 CUs), which the test reads back from cfm_attn_plan."""
import ctypes
import functools

import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib, ops
from tests import dropout_hash as dh

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 2, 2
SEED = 11
TOL = 1e-2
BAND = 256                 # guard floats on each side of the workspace (1 KiB: section offsets stay 256-aligned)
PATTERN = -7.25
ONE_WG = _lib.ATTN_MODE_REL_ZERO_FILL
TWO_PASS = _lib.ATTN_MODE_DKDV_TWO_PASS

# T, dk, lengths, mode bits that shape the launch
SHAPES = [
    pytest.param(33, 64, (33, 7), ONE_WG, id="T33-dk64"),            # one full key block plus a 1-key tail
    pytest.param(97, 64, (97, 20), ONE_WG, id="T97-dk64"),           # not a multiple of 32 or 64
    pytest.param(130, 64, (130, 31), ONE_WG, id="T130-dk64"),        # a key tile past the staged image
    pytest.param(373, 64, (373, 19), ONE_WG, id="T373-dk64"),        # the workload's 12 waves
    pytest.param(373, 36, (373, 29), ONE_WG, id="T373-dk36"),        # 8-byte staging (Conformer-S)
    pytest.param(373, 36, (373, 29), 0, id="T373-dk36-split"),       # ... with split workgroups
]


@pytest.fixture
def attn_mode():
    yield lambda m: _lib.call("cfm_attn_set_mode", m)
    _lib.call("cfm_attn_set_mode", 0)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _inputs(T, dk, lens):
    g = torch.Generator().manual_seed(1000 * T + dk)
    qkv = torch.randn(B * T, 3 * H * dk, generator=g).to(DEV, torch.bfloat16)
    do = torch.randn(B * T, H * dk, generator=g).to(DEV, torch.bfloat16)
    return qkv, do, torch.tensor(lens, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _reference(T, dk, lens, drop_p):
    """fp32 torch gradient (B*T, 3, H*dk) of softmax(q k^T / sqrt(dk) + mask) [* keep * keep_scale] v, the keep mask
    from the numpy restatement of the hash; computed once per (shape, p) and shared by the launch variants"""
    qkv, do, lt = _inputs(T, dk, lens)
    x = qkv.float().view(B, T, 3, H, dk).requires_grad_()
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) / dk ** 0.5
    pad = torch.arange(T, device=DEV)[None, :] >= lt[:, None].long()
    probs = s.masked_fill(pad[:, None, None, :], float("-inf")).softmax(-1)
    if drop_p > 0:
        keep = torch.from_numpy(dh.attn_keep(B, H, T, drop_p, SEED)).to(DEV)
        probs = probs * keep.to(probs) * dh.keep_scale(drop_p)
    (probs @ v).transpose(1, 2).reshape(B * T, H * dk).backward(do.float())
    return x.grad.reshape(B * T, 3, H * dk).detach()


def _plan(T, dk, mode):
    q = _lib.AttnQuery(B, T, H, dk, _lib.BF16, 0, 0, 0, 0, mode,
                       torch.cuda.get_device_properties(0).multi_processor_count, -1)
    c = _lib.AttnChoice()
    assert _lib.load().cfm_attn_plan(ctypes.byref(q), ctypes.byref(c)) == 0
    return c


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("T,dk,lens,shape_mode", SHAPES)
def test_one_sweep_dkdv(attn_mode, T, dk, lens, shape_mode, drop_p):
    qkv, do, lt = _inputs(T, dk, lens)
    HD = H * dk
    c = _plan(T, dk, shape_mode)
    assert c.path == _lib.ATTN_PATH_HEAD and c.dq_stored
    nb = (T + 31) // 32
    if shape_mode & ONE_WG:
        assert (c.qs, c.waves) == (1, nb)
    elif torch.cuda.get_device_properties(0).multi_processor_count >= 2 * B * H:
        assert c.qs > 1 and c.waves == -(-nb // c.qs)
    off, size = c.ws_off[_lib.ATTN_WS_DS] // 4, c.ws_size[_lib.ATTN_WS_DS] // 4
    assert size * 4 == B * H * (32 * nb) ** 2 * 2 and c.ws_total % 4 == 0

    attn_mode(shape_mode)
    o, lse = ops.attn_fwd(qkv, lt, B, T, H, dk, drop_p=drop_p, seed=SEED)

    def run(mode):
        """(dqkv as (B*T, 3, HD) fp32, the dS^T section's bits, the guarded buffer) of one backward whose workspace
        starts out all NaN"""
        attn_mode(mode)
        buf = torch.full((2 * BAND + c.ws_total // 4,), PATTERN, device=DEV)
        ws = buf[BAND:BAND + c.ws_total // 4]
        ws.fill_(float("nan"))
        dqkv = ops.attn_bwd(qkv, o, do, lse, lt, B, T, H, dk, drop_p=drop_p, seed=SEED, ws=ws)[0]
        torch.cuda.synchronize()
        return dqkv.float().view(B * T, 3, HD), ws[off:off + size].view(torch.int32).clone(), buf

    got, ds_new, buf = run(shape_mode)
    old, ds_old, buf_old = run(shape_mode | TWO_PASS)

    # 1. against fp32 torch: dQ (through the stored dS^T), dK, dV, each on its own
    ref = _reference(T, dk, lens, drop_p)
    errs = [_rel(got[:, i], ref[:, i]) for i in range(3)]
    errs_old = [_rel(old[:, i], ref[:, i]) for i in range(3)]
    print(f"T {T} dk {dk} p {drop_p} qs {c.qs}: rel err dQ/dK/dV one-sweep {errs} two-pass {errs_old}")
    assert max(errs) < TOL
    # keys at or past len: exactly zero dK and dV
    g4 = got.view(B, T, 3, HD)
    for b, n in enumerate(lens):
        assert not g4[b, n:, 1:].any()

    # 2. bit identity with the two-pass kernel: dK, dV, the stored dS^T (unwritten words keep the NaN fill in both)
    assert torch.equal(got[:, 1:], old[:, 1:])
    assert torch.equal(ds_new, ds_old)
    assert torch.equal(got[:, 0], old[:, 0])          # dQ: the same consumer on the same dS^T

    # 3. the NaN-filled workspace: dQ never reads a word the dK/dV kernel did not write; the bands are untouched
    assert torch.isfinite(got).all()
    for bf in (buf, buf_old):
        assert bool((bf[:BAND] == PATTERN).all()) and bool((bf[-BAND:] == PATTERN).all())

    # 4. graph replay reproduces the eager launch
    attn_mode(shape_mode)
    ws = torch.full((c.ws_total // 4,), float("nan"), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture
        ops.attn_bwd(qkv, o, do, lse, lt, B, T, H, dk, drop_p=drop_p, seed=SEED, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    ws.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = ops.attn_bwd(qkv, o, do, lse, lt, B, T, H, dk, drop_p=drop_p, seed=SEED, ws=ws)[0]
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.float().view(B * T, 3, HD), got)
