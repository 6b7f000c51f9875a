"""The conv-module test helpers checked without a GPU: tests/convmod_ref.py's fp64 references against torch autograd,
its comparators against planted mistakes, the workspace formulas against the documented layouts, the index-exact
margin, and cfm_convmod_plan pinned for every row of the table.

Where each kernel family of csrc/convmod.hip is reached (tests/test_gpu_convmod.py runs every row through every entry
point; the row ids are convmod_ref.IDS):
  forward      vectorised 2x37x64-k31-bf16 ..., compiled-K scalar 2x50x66-k31-bf16 / 3x100x96-k3-f32, runtime-K 2x70x72-k9-*
  backward     the same rows (plain); folded BatchNorm / GroupNorm: the vectorised and compiled-K rows, the runtime-K
               rows are UNSUPPORTED there and take the unfused pair
  apply        vec8 C % 8 == 0 rows, scalar 1x128x12-k7 / 2x1x4-k5 / 2x50x66-k31 / 1x65x68-k63 and any unaligned z
test_plan_of_every_row asserts exactly this."""
import pytest
import torch
import torch.nn.functional as F

from nn_conformer_for_speech_recognition_amd import _lib, ops
from tests import convmod_ref as R

f64 = torch.float64
EPS, MOM = 1e-5, 0.1


def _close(name, got, want, tol=1e-12):
    got, want = got.double(), want.double()
    err = (got - want).abs().max().item()
    assert err <= tol * max(1.0, want.abs().max().item()), (name, err)


def _inputs(case, ratios=R.RATIOS):
    g = torch.Generator().manual_seed(1000 * case.B + case.T + case.C + case.K)
    d = R.real_inputs(*case.shape, g, ratios=ratios)
    return {k: v.double() for k, v in d.items()}


# ------------------------------------------------------------------------------------------ 1. references vs torch
@pytest.mark.parametrize("case", R.CASES[:10:3] + R.CASES[-1:], ids=lambda c: c.id)
@pytest.mark.parametrize("norm", ["bn_train", "bn_eval", "gn", "bn_train_noact"])
def test_references_equal_torch_autograd(case, norm):
    B, T, C, K = case.shape
    M = B * T
    d = _inputs(case, ratios=(0.0, 1.0))
    leaf = {k: d[k].clone().requires_grad_() for k in ("a", "w", "bias", "gamma", "beta")}
    u = F.glu(leaf["a"].view(B, T, 2 * C), dim=-1).transpose(1, 2)
    y = F.conv1d(u, leaf["w"].view(C, 1, K), leaf["bias"], padding=(K - 1) // 2, groups=C)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    act = norm != "bn_train_noact"
    if norm == "gn":
        n = F.group_norm(y, 1, leaf["gamma"], leaf["beta"], EPS)
    else:
        n = F.batch_norm(y, rm, rv, leaf["gamma"], leaf["beta"], norm != "bn_eval", MOM, EPS)
    z = (F.silu(n) if act else n).transpose(1, 2).reshape(M, C)
    (z * d["dz"]).sum().backward()

    yr, S = R.glu_dwconv_fwd(d["a"], d["w"], d["bias"], B, T, C, K)
    _close("y", yr, y.detach().transpose(1, 2).reshape(M, C))
    assert (S >= yr.abs() - 1e-12).all()
    if norm == "gn":
        st = R.gn_stats(yr, B, T, C, EPS)
        zr, _ = R.gn_apply(yr, st.mean, st.invstd, d["gamma"], d["beta"], T)
        dbeta, dgamma, coef, *_ = R.gn_bwd_sums(d["dz"], yr, st.mean, st.invstd, d["gamma"], d["beta"], B, T)
        dy, Sdy = R.gn_bwd_dy(d["dz"], yr, st.mean, st.invstd, d["gamma"], d["beta"], coef, T)
        folded = R.gn_folded_bwd(d["dz"], yr, st.mean, st.invstd, d["gamma"], d["beta"], coef, d["a"], d["w"], B, T, C, K)
    else:
        training = norm != "bn_eval"
        st = R.bn_stats(yr, M, EPS, MOM, d["rm"], d["rv"]) if training else R.eval_stats(d["rm"], d["rv"], EPS)
        if training:
            _close("running_mean", st.rm, rm)
            _close("running_var", st.rv, rv)
            one = R.stats_from_sums(yr.sum(0), (yr * yr).sum(0), M, EPS)      # the one-pass form the kernels use
            _close("one-pass var", one.var, st.var, 1e-9)
        else:
            assert torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"])
        zr, _ = R.bn_apply(yr, st.mean, st.invstd, d["gamma"], d["beta"], act)
        dbeta, dgamma, *_ = R.bn_bwd_sums(d["dz"], yr, st.mean, st.invstd, d["gamma"], d["beta"], act)
        dy, Sdy = R.bn_bwd_dy(d["dz"], yr, st.mean, st.invstd, d["gamma"], d["beta"], dbeta, dgamma, M, training, act)
        folded = None
        if act:
            folded = R.bn_folded_bwd(d["dz"], yr, st.mean, st.invstd, d["gamma"], d["beta"], dbeta, dgamma, M,
                                     training, d["a"], d["w"], B, T, C, K)
    da, dw, db, S_da, S_dw, S_db = R.glu_dwconv_bwd(dy, d["a"], d["w"], B, T, C, K)
    _close("z", zr, z.detach())
    _close("dbeta", dbeta, leaf["beta"].grad, 1e-11)
    _close("dgamma", dgamma, leaf["gamma"].grad, 1e-11)
    _close("da", da, leaf["a"].grad, 1e-11)
    _close("dw", dw, leaf["w"].grad, 1e-11)
    # (batch statistics cancel the depthwise bias: its gradient is rounding noise on the scale of sum |dy|)
    assert (db - leaf["bias"].grad).abs().max() <= 1e-11 * max(1.0, S_db.max().item())
    assert (S_da >= da.abs() - 1e-12).all() and (S_dw >= dw.abs() - 1e-12).all() and (Sdy >= dy.abs() - 1e-12).all()
    if folded is not None:
        for name, f, g in zip(("da", "dw", "db"), folded[:3], (da, dw, db)):
            assert torch.equal(f, g), name
        assert (folded[3] >= S_da - 1e-12).all()


def test_bn_stats_single_row_and_joined_shards():
    """M = 1 (torch refuses it in train mode): variance 0, running variance guarded as the kernel does; and the
    statistics of a joined batch from the sums of its shards"""
    y = torch.tensor([[0.5, -2.0, 3.0]], dtype=f64)
    st = R.bn_stats(y, 1, EPS, MOM, torch.zeros(3), torch.ones(3))
    assert torch.equal(st.mean, y[0]) and torch.equal(st.var, torch.zeros(3, dtype=f64))
    _close("invstd", st.invstd, torch.full((3,), EPS ** -0.5, dtype=f64))
    _close("rv", st.rv, torch.full((3,), 1 - MOM, dtype=f64))
    g = torch.Generator().manual_seed(3)
    y = torch.randn(40, 5, generator=g, dtype=f64) + 2
    s = R.stats_from_sums(y[:20].sum(0) + y[20:].sum(0), (y[:20] ** 2).sum(0) + (y[20:] ** 2).sum(0), 40, EPS)
    j = R.bn_stats(y, 40, EPS)
    _close("mean", s.mean, j.mean)
    _close("var", s.var, j.var, 1e-10)


# ------------------------------------------------------------------------------------------ 2. planted mistakes
def _stored(t, dtype):
    """a correct fp64 result as the kernel would store it"""
    return t.to(dtype)


def _reject(name, got, ref, n, S, bf16=False):
    c = R.check(name, got, ref, n, S, bf16)
    assert not c.ok, f"planted mistake passed -- {c}"
    assert c.index is not None


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_comparators_reject_planted_mistakes(case):
    B, T, C, K = case.shape
    M, pad, dt = B * T, (K - 1) // 2, case.dtype
    bf = dt == torch.bfloat16
    d = _inputs(case, ratios=(0.0, 1.0))
    a, w, bias, dz, gamma, beta = (d[k] for k in ("a", "w", "bias", "dz", "gamma", "beta"))
    u, _, _ = R.glu(a, C)
    y, S = R.dwconv(u, w, bias, B, T, C, K)
    y3, u3 = y.view(B, T, C), u.view(B, T, C)
    st = R.bn_stats(y, M, EPS, MOM, d["rm"], d["rv"])
    dbeta, dgamma, Sb, Sg = R.bn_bwd_sums(dz, y, st.mean, st.invstd, gamma, beta)
    dy, Sdy = R.bn_bwd_dy(dz, y, st.mean, st.invstd, gamma, beta, dbeta, dgamma, M, True)
    # the depthwise backward of a dy that is not a BatchNorm gradient (whose column sums cancel)
    da, dw, db, S_da, S_dw, S_db = R.glu_dwconv_bwd(dz, a, w, B, T, C, K)
    z, Sz = R.bn_apply(y, st.mean, st.invstd, gamma, beta, 1)

    # the unmutated results pass after rounding to the stored dtype
    ok = [R.check("y", _stored(y, torch.float32), y, K, S), R.check("da", _stored(da, dt), da, K, S_da, bf),
          R.check("dw", _stored(dw, torch.float32), dw, M, S_dw), R.check("db", _stored(db, torch.float32), db, M, S_db),
          R.check("dgamma", dgamma.float(), dgamma, M, Sg), R.check("dbeta", dbeta.float(), dbeta, M, Sb),
          R.check("z", _stored(z, dt), z, 4, Sz, bf), R.check("dy", dy.float(), dy, R.DY_OPS, Sdy)]
    ok += R.check_stats("", st, st.mean.float(), st.invstd.float(), st.rm.float(), st.rv.float(), MOM, d["rm"], d["rv"])
    R.assert_all(ok, show=False)

    # one halo row at a tile boundary taken from the neighbouring utterance (needs a second tile and a second utterance)
    if T > R.TT and B > 1:
        m = y3.clone()
        for t in range(R.TT, min(T, R.TT + pad)):
            k = R.TT - 1 - t + pad
            m[:, t] += w[:, k] * (u3.roll(-1, 0)[:, R.TT - 1] - u3[:, R.TT - 1])
        _reject("halo row of the neighbouring utterance", m.reshape(M, C).float(), y, K, S)
    # one halo row left non-zero at t < 0 (the clamped staging load returns row 0) and at t >= T
    m = y3.clone()
    m[:, 0] += w[:, pad - 1] * u3[:, 0]
    _reject("halo row t = -1 not zeroed", m.reshape(M, C).float(), y, K, S)
    m = y3.clone()
    m[:, T - 1] += w[:, pad + 1] * u3[:, T - 1]
    _reject("halo row t = T not zeroed", m.reshape(M, C).float(), y, K, S)
    # taps k and k + 1 swapped in the last time tile only
    t0 = (T - 1) // R.TT * R.TT
    ws = w.clone()
    ws[:, [pad, pad + 1]] = w[:, [pad + 1, pad]]
    m = y3.clone()
    m[:, t0:] = R.dwconv(u, ws, bias, B, T, C, K)[0].view(B, T, C)[:, t0:]
    _reject("taps swapped in the last tile", m.reshape(M, C).float(), y, K, S)
    # lane C - 1 reading channel C - 2
    am = a.clone()
    am[:, C - 1], am[:, 2 * C - 1] = a[:, C - 2], a[:, 2 * C - 2]
    m = y.clone()
    m[:, C - 1] = R.glu_dwconv_fwd(am, w, bias, B, T, C, K)[0][:, C - 1]
    _reject("lane C-1 reads channel C-2", m.float(), y, K, S)
    m = da.clone()
    m[:, C - 1] = R.glu_dwconv_bwd(dz, am, w, B, T, C, K)[0][:, C - 1]
    _reject("lane C-1 reads channel C-2 (da)", _stored(m, dt), da, K, S_da, bf)
    # the padded frames of the last tile counted into dw / db / the statistics (the clamped loads return row T - 1)
    npad = -T % R.TT
    if npad:
        dy3 = dz.view(B, T, C)
        _reject("padded frames in db", (db + npad * dy3[:, T - 1].sum(0)).float(), db, M, S_db)
        m = dw.clone()
        m[:, pad] += npad * (dy3[:, T - 1] * u3[:, T - 1]).sum(0)
        _reject("padded frames in dw", m.float(), dw, M, S_dw)
        s1, s2 = y.sum(0) + npad * y3[:, T - 1].sum(0), (y * y).sum(0) + npad * (y3[:, T - 1] ** 2).sum(0)
        bad = R.stats_from_sums(s1, s2, M, EPS)
        assert not all(c.ok for c in R.check_stats("", st, bad.mean.float(), bad.invstd.float()))
    # the biased variance written to running_var
    if M > 1:
        rv_bad = (1 - MOM) * d["rv"] + MOM * st.var
        cs = R.check_stats("", st, rm=st.rm.float(), rv=rv_bad.float(), momentum=MOM, rm_old=d["rm"], rv_old=d["rv"])
        assert cs[0].ok and not cs[1].ok, [str(c) for c in cs]
    # M instead of M_total under world = 2: the sums of both shards divided by one shard's rows
    if B % 2 == 0:
        half = R.stats_from_sums(y.sum(0), (y * y).sum(0), M // 2, EPS)
        assert not all(c.ok for c in R.check_stats("", st, half.mean.float(), half.invstd.float()))
        m, _ = R.bn_bwd_dy(dz, y, st.mean, st.invstd, gamma, beta, dbeta, dgamma, M // 2, True)
        _reject("dy with M instead of M_total", m.float(), dy, R.DY_OPS, Sdy)
    # dgamma and dbeta swapped
    _reject("dgamma <- dbeta", dbeta.float(), dgamma, M, Sg)
    _reject("dbeta <- dgamma", dgamma.float(), dbeta, M, Sb)
    # eval mode using batch statistics
    ev = R.eval_stats(d["rm"], d["rv"], EPS)
    ze, Sze = R.bn_apply(y, ev.mean, ev.invstd, gamma, beta, 1)
    _reject("eval mode with batch statistics", _stored(z, dt), ze, 4, Sze, bf)


def test_every_planted_mistake_is_expressible_somewhere():
    """the conditional mutations (a neighbouring utterance, padded frames, two shards) each apply to some row"""
    assert any(c.T > R.TT and c.B > 1 for c in R.CASES)
    assert any(c.T % R.TT for c in R.CASES) and any(c.B % 2 == 0 for c in R.CASES)


# ------------------------------------------------------------------------------------------ 3. index-exact margin
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_index_exact_bound_is_below_an_eighth_of_the_grid_step(case):
    B, T, C, K = case.shape
    a, w, bias, dy = R.exact_inputs(*case.shape, torch.Generator().manual_seed(7))
    y, S = R.glu_dwconv_fwd(a, w, bias, B, T, C, K)
    da, dw, db, S_da, S_dw, S_db = R.glu_dwconv_bwd(dy, a, w, B, T, C, K)
    for name, v in (("y", y), ("da", da), ("dw", dw), ("db", db)):
        assert torch.equal(v / R.GRID, torch.round(v / R.GRID)), f"{name} is off the grid"
        assert torch.equal(v.float().double(), v) and v.abs().max() < 2 ** 22
    assert torch.equal(da.to(torch.bfloat16).double(), da)          # exact in bf16: equality is the check
    margins = {"y": R.exact_margin(K, S), "da": R.exact_margin(K, S_da), "dw": R.exact_margin(B * T, S_dw),
               "db": R.exact_margin(B * T, S_db)}
    assert max(margins.values()) < 1 / 8, margins
    # a whole grid step is rejected, in either dtype
    i = (0, C - 1)
    for dt in (torch.float32, torch.bfloat16):
        m = da.clone()
        m[i] += R.GRID
        assert R.check_exact("da", da.to(dt), da, K, S_da, dt).ok
        assert not R.check_exact("da", m.to(dt), da, K, S_da, dt).ok


# ------------------------------------------------------------------------------------------ 4. workspace formulas
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_workspace_covers_every_launch(case):
    B, T, C, K = case.shape
    have = _lib.size_call("cfm_convmod_ws_bytes", B, T, C, K)
    assert _lib.size_call("cfm_convmod_nparts", B, T) == R.nparts(B, T)
    for what, floats in R.ws_extents(B, T, C, K).items():
        assert have >= 4 * floats, (what, have, 4 * floats)
    assert have % 4 == 0


@pytest.mark.parametrize("M,C", R.BN_SHAPES)
def test_bn_workspace_covers_the_row_chunk_partials(M, C):
    assert _lib.size_call("cfm_bn_ws_bytes", C) >= 4 * R.bn_ws_extent(C)
    assert R.BN_PARTS == 256


# ------------------------------------------------------------------------------------------ 5. the plan
ALIGNED = 1 << 20


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_plan_of_every_row(case):
    B, T, C, K = case.shape
    dta = R.code(case.dt)
    for name, op in R.OPS.items():
        fam, dz16, apply = R.plan(op, dta, C, K)
        assert fam == getattr(case, name), (name, fam)
        assert dz16 == int(fam == R.V and name in ("bwd_bn", "bwd_gn") and case.dt == "bf16")
        assert apply == _lib.CONVMOD_APPLY_NONE
        # the A/B switch: everything vectorised becomes the compiled-K scalar kernel, nothing else moves
        forced = R.plan(op, dta, C, K, force_scalar=1)[0]
        assert forced == (R.KT if fam == R.V else fam)
    for norm in (0, 1):
        for dtz in (_lib.BF16, _lib.F32):
            kw = dict(dt_z=dtz, M=B * T, norm=norm)
            assert R.plan(R.OPS["fwd"], dta, C, K, y=ALIGNED, z=2 * ALIGNED, **kw)[2] == case.apply
            for off in (4, 8):      # a 4-byte-aligned z (or y) that is not 16-byte aligned: the scalar apply
                assert R.plan(R.OPS["fwd"], dta, C, K, y=ALIGNED, z=2 * ALIGNED + off, **kw)[2] == R.A1
                assert R.plan(R.OPS["fwd"], dta, C, K, y=ALIGNED + off, z=2 * ALIGNED, **kw)[2] == R.A1


def test_table_reaches_every_family_and_apply_kernel():
    for name in ("fwd", "bwd"):
        assert {getattr(c, name) for c in R.CASES} == {R.V, R.KT, R.KRT}, name
    for name in ("bwd_bn", "bwd_gn"):
        assert {getattr(c, name) for c in R.CASES} == {R.V, R.KT, R.UNS}, name
    # fp32 a and bf16 a with C % 4 != 0 both take the compiled-K scalar kernels (the float and bf16 instantiations)
    assert {c.dt for c in R.CASES if c.fwd == R.KT} == {"bf16", "f32"}
    assert {c.dt for c in R.CASES if c.fwd == R.KRT} == {"bf16", "f32"}
    # both apply kernels; test_gpu_convmod.py runs each row with z in bf16 and in fp32
    assert {c.apply for c in R.CASES} == {R.A8, R.A1}
    # mixed dtypes: a bf16 with an fp32 da is not the vectorised backward; an fp32 dz is staged as fp32
    assert R.plan(R.OPS["bwd"], _lib.BF16, 64, 31, dt_da=_lib.F32)[0] == R.KT
    assert R.plan(R.OPS["bwd_bn"], _lib.BF16, 64, 31, dt_dz=_lib.F32)[:2] == (R.V, 0)
    # kernel sizes no kernel exists for
    for K in (0, 4, 65):
        assert R.plan(R.OPS["fwd"], _lib.BF16, 64, K)[0] == R.UNS
    lib = _lib.load()
    assert lib.cfm_convmod_plan(None, None) == -1
    assert set(R.COMPILED_K) == {K for K in range(1, 64, 2) if R.plan(R.OPS["bwd_bn"], _lib.F32, 64, K)[0] == R.KT}
    # the one fold-or-not predicate the Python callers share says the same
    for K in range(66):
        assert ops.dwconv_bwd_folds(K) == (K in R.COMPILED_K), K
