"""The conv-module kernels (csrc/convmod.hip) launch by launch against the fp64 references and derived bounds of
tests/convmod_ref.py, on guarded buffers.

Every call goes through _lib.call.  Inputs sit in NaN-filled buffers with 64 KiB of NaN on either side, outputs (y, z,
da, dw, db, the statistics, the running statistics, and the workspace sized exactly by the *_ws_bytes call) are
pre-poisoned with NaN and carry a sentinel outside; after every launch every output's guard is compared bit for bit
and the values are compared element by element -- a NaN left inside fails whatever the bound.  Each reference is fed the
operands that launch read, as stored on the device (the kernel's own y, mean, invstd, dgamma ...), so no bound absorbs
an upstream stage; each test prints its stages' worst error / bound."""
import functools

import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib
from tests import convmod_ref as R
from tests.gemm_exact import Guarded, assert_untouched

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
EPS, MOM = 1e-5, 0.1
ZDT = [pytest.param(BF, id="z-bf16"), pytest.param(F32, id="z-f32")]
CASE = pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)


# ------------------------------------------------------------------------------------------ guarded buffers, launches
def gin(t, dtype=None):
    """an input: the tensor (1-D or 2-D) as `dtype` inside a NaN-filled guarded device buffer"""
    t = t if dtype is None else t.to(dtype)
    t = t.reshape(1, -1) if t.dim() == 1 else t
    return Guarded(t.shape[0], t.shape[1], t.shape[1], t.dtype, "nan", device=DEV).set(t)


def gout(rows, cols, dtype=F32):
    """an output: NaN inside, the sentinel outside"""
    return Guarded(rows, cols, cols, dtype, "sentinel", device=DEV).poison()


def gstate(t):
    """an in/out buffer (running statistics): values inside, the sentinel outside"""
    return Guarded(1, t.numel(), t.numel(), F32, "sentinel", device=DEV).set(t.reshape(1, -1).float())


def P(g, off=0):
    return g.view.data_ptr() + off * g.view.element_size()


def host(g):
    """the logical tensor as stored, on the CPU: (rows, cols), or (cols,) for a vector"""
    v = g.view[0].cpu()
    return v[0] if g.rows == 1 else v


def launch(name, *args, outs=()):
    _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()
    for i, g in enumerate(outs):
        assert_untouched(g, f"{name} output {i}")


def ws_for(B, T, C, K):
    nbytes = _lib.size_call("cfm_convmod_ws_bytes", B, T, C, K)
    return gout(1, nbytes // 4)


def gen(case, salt=0):
    return torch.Generator().manual_seed(1000 * case.B + case.T + case.C + case.K + 7919 * salt)


def forward(case, a, w, bias):
    """cfm_glu_dwconv_fwd on guarded buffers -> (ga, gw, gy, ws)"""
    B, T, C, K = case.shape
    ga, gw, gb = gin(a, case.dtype), gin(w), gin(bias)
    gy, ws = gout(B * T, C), ws_for(B, T, C, K)
    launch("cfm_glu_dwconv_fwd", P(ga), R.code(case.dt), P(gw), P(gb), P(gy), B, T, C, K, P(ws), outs=(gy, ws))
    return ga, gw, gy, ws


def partial_checks(case, gy, ws):
    """the (sum, sumsq) partials the forward left in ws against the fp64 sums of the kernel's own y"""
    B, T, C, K = case.shape
    part, mag, frames = R.tile_sums(host(gy), B, T, C)
    got = host(ws)[:part.numel()].reshape(part.shape)
    return [R.check("partials", got, part, frames[None, :, None], mag)]


@functools.lru_cache(maxsize=None)
def _real(case_id, ratios):
    case = R.CASES[R.IDS.index(case_id)]
    return R.real_inputs(*case.shape, gen(case), ratios=ratios)


def real(case, shifted=True):
    """the real-valued operands of a row, generated once.  shifted: channel means at |mean| / sigma = 0, 4, 16, 64
    through the depthwise bias (the forward and statistics tests); the backward tests use the unshifted ones"""
    return _real(case.id, R.RATIOS if shifted else (0.0,))


def agree(tag, folded, unfused):
    """the folded launch equals the unfused pair to 1e-5 in relative L2.  Every kernel that forms the BatchNorm /
    GroupNorm input gradient does so in one operation order (convmod.hip bn_dy_elem / gn_dy_elem and their packed
    twins in the vectorised kernel), so on the MI355X the pair is bit-identical in every row -- before that, a
    last-bit fp32 difference in dy now and then flipped one bf16 rounding of da, and one flipped element of ~10^4
    is 1e-5 to 3e-5 in relative L2.  The count of differing elements is printed with the figure."""
    f, u = host(folded).double(), host(unfused).double()
    err = ((f - u).norm() / u.norm().clamp_min(1e-30)).item()
    ndiff = int((f != u).sum())
    spacing = 2.0 ** (torch.floor(torch.log2(u.abs().clamp_min(2.0 ** -126))) - (7 if unfused.dtype == BF else 23))
    steps = ((f - u).abs() / spacing).max().item()
    name = (f"folded = unfused {tag} (relative L2 against 1e-5; {ndiff} of {u.numel()} elements differ, by at most "
            f"{steps:.3g} steps of the stored format)")
    return R.Check(name, err < 1e-5, err / 1e-5, (), err, 0.0, 1e-5)


# ------------------------------------------------------------------------------------------ forward
@CASE
def test_forward_index_exact(case):
    B, T, C, K = case.shape
    a, w, bias, _ = R.exact_inputs(*case.shape, gen(case, 1))
    ga, gw, gy, ws = forward(case, a, w, bias)
    y, S = R.glu_dwconv_fwd(host(ga), w, bias, B, T, C, K)
    print(f"\nforward, index-exact {case.id}")
    R.assert_all([R.check_exact("y", host(gy), y, K, S, F32)] + partial_checks(case, gy, ws))


@CASE
def test_forward_real(case):
    B, T, C, K = case.shape
    d = real(case)
    ga, gw, gy, ws = forward(case, d["a"], d["w"], d["bias"])
    y, S = R.glu_dwconv_fwd(host(ga), d["w"], d["bias"], B, T, C, K)
    print(f"\nforward, real {case.id}")
    R.assert_all([R.check("y", host(gy), y, K, S)] + partial_checks(case, gy, ws))


# ------------------------------------------------------------------------------------------ BatchNorm stats and apply
def bn_forward(case, d, gy, ws, training, zdt, z_off=0):
    """cfm_bn_silu_fwd -> (gmean, ginvstd, grm, grv, gz)"""
    B, T, C, K = case.shape
    gg, gbt = gin(d["gamma"]), gin(d["beta"])
    grm, grv = gstate(d["rm"]), gstate(d["rv"])
    gmean, ginv = gout(1, C), gout(1, C)
    gz = gout(1, B * T * C + z_off, zdt)
    launch("cfm_bn_silu_fwd", P(gy), P(gg), P(gbt), P(grm), P(grv), MOM, EPS, int(training), P(gmean), P(ginv),
           P(gz, z_off), R.code(zdt), B, T, C, P(ws), outs=(gmean, ginv, grm, grv, gz, gy, ws))
    return gmean, ginv, grm, grv, gz


def bn_forward_checks(case, d, gy, out, training, zdt, z_off=0):
    B, T, C, K = case.shape
    gmean, ginv, grm, grv, gz = out
    yk = host(gy)
    mean, invstd = host(gmean), host(ginv)
    checks = []
    if training:
        st = R.bn_stats(yk, B * T, EPS, MOM, d["rm"], d["rv"])
        checks += R.check_stats("", st, mean, invstd, host(grm), host(grv), MOM, d["rm"], d["rv"])
        rel = ((invstd.double() - st.invstd) / st.invstd).abs()
        by = {int(r): f"{rel[d['ratio'] == r].max().item():.2e}" for r in R.RATIOS if (d["ratio"] == r).any()}
        print(f"    invstd relative error by |mean|/sigma (measured r^2 up to {st.r2.max().item():.0f}): {by}")
    else:
        ev = R.eval_stats(d["rm"], d["rv"], EPS)
        assert torch.equal(mean, d["rm"]) and torch.equal(host(grm), d["rm"]) and torch.equal(host(grv), d["rv"])
        # rsqrtf(rv + eps): the sum's rounding (a quarter ulp of the result) and the instruction's accuracy
        checks.append(R.within("invstd (eval)", invstd, ev.invstd, 4 * R.U24 * ev.invstd))
    z, Sz = R.bn_apply(yk, mean, invstd, d["gamma"], d["beta"], 1)
    zk = host(gz)
    if z_off:
        assert torch.isnan(zk[:z_off]).all(), "the elements before an offset z were written"
    checks.append(R.check("z", zk[z_off:].reshape(B * T, C), z, 4, Sz, zdt == BF))
    return checks


@CASE
@pytest.mark.parametrize("zdt", ZDT)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_stats_and_apply(case, training, zdt):
    d = real(case)
    ga, gw, gy, ws = forward(case, d["a"], d["w"], d["bias"])
    out = bn_forward(case, d, gy, ws, training, zdt)
    B, T, C, K = case.shape
    fam, _, apply = R.plan(R.OPS["fwd"], R.code(case.dt), C, K, dt_z=R.code(zdt), M=B * T, y=P(gy), z=P(out[4]))
    assert (fam, apply) == (case.fwd, case.apply)
    print(f"\nBatchNorm forward {case.id} {'train' if training else 'eval'}")
    R.assert_all(bn_forward_checks(case, d, gy, out, training, zdt))


@pytest.mark.parametrize("zdt", ZDT)
def test_bn_apply_of_a_misaligned_z_is_the_scalar_kernel_with_the_same_values(zdt):
    case = R.CASES[1]                   # C % 8 == 0: an aligned z takes the 8-wide apply
    B, T, C, K = case.shape
    d = real(case)
    ga, gw, gy, ws = forward(case, d["a"], d["w"], d["bias"])
    z_off = 1 if zdt == F32 else 2      # 4 bytes past a 16-byte boundary
    out = bn_forward(case, d, gy, ws, True, zdt, z_off)
    kw = dict(dt_z=R.code(zdt), M=B * T, y=P(gy))
    assert R.plan(R.OPS["fwd"], R.code(case.dt), C, K, z=P(out[4], z_off), **kw)[2] == R.A1
    assert R.plan(R.OPS["fwd"], R.code(case.dt), C, K, z=P(out[4]), **kw)[2] == R.A8
    print(f"\nBatchNorm forward, z 4 bytes off {case.id}")
    R.assert_all(bn_forward_checks(case, d, gy, out, True, zdt, z_off))
    ws2 = ws_for(B, T, C, K)
    ws2.view.copy_(ws.view)
    aligned = bn_forward(case, d, gy, ws2, True, zdt)
    assert torch.equal(host(out[4])[z_off:], host(aligned[4])), "scalar and 8-wide apply differ"
    for i in range(4):
        assert torch.equal(host(out[i]), host(aligned[i]))


# ------------------------------------------------------------------------------------------ backward
def dwconv_bwd(case, gdy, ga, gw, ws, defer):
    """cfm_glu_dwconv_bwd (defer: dw == NULL, then cfm_glu_dwconv_bwd_wgrad) -> (gda, gdw, gdb)"""
    B, T, C, K = case.shape
    gda, gdw, gdb = gout(B * T, 2 * C, case.dtype), gout(C, K), gout(1, C)
    dt = R.code(case.dt)
    if defer:
        launch("cfm_glu_dwconv_bwd", P(gdy), P(ga), dt, P(gw), P(gda), dt, None, None, B, T, C, K, P(ws),
               outs=(gda, ws))
        launch("cfm_glu_dwconv_bwd_wgrad", P(ws), B, T, C, K, P(gdw), P(gdb), outs=(gdw, gdb, ws))
    else:
        launch("cfm_glu_dwconv_bwd", P(gdy), P(ga), dt, P(gw), P(gda), dt, P(gdw), P(gdb), B, T, C, K, P(ws),
               outs=(gda, gdw, gdb, ws))
    return gda, gdw, gdb


def same_bits(x, y, what):
    for name, p, q in zip(("da", "dw", "db"), x, y):
        assert torch.equal(host(p), host(q)), f"{what}: {name} differs"


@CASE
def test_backward_plain_index_exact(case):
    B, T, C, K = case.shape
    a, w, _, dy = R.exact_inputs(*case.shape, gen(case, 2))
    ga, gw, gdy, ws = gin(a, case.dtype), gin(w), gin(dy), ws_for(B, T, C, K)
    now = dwconv_bwd(case, gdy, ga, gw, ws, defer=False)
    later = dwconv_bwd(case, gdy, ga, gw, ws_for(B, T, C, K), defer=True)
    da, dw, db, S_da, S_dw, S_db = R.glu_dwconv_bwd(dy, host(ga), w, B, T, C, K)
    assert R.plan(R.OPS["bwd"], R.code(case.dt), C, K)[0] == case.bwd
    print(f"\nbackward, plain, index-exact {case.id}")
    R.assert_all([R.check_exact("da", host(now[0]), da, K, S_da, case.dtype),
                  R.check_exact("dw", host(now[1]), dw, B * T, S_dw, F32),
                  R.check_exact("db", host(now[2]), db, B * T, S_db, F32)])
    same_bits(now, later, "deferred weight gradient")


def backward_stage_checks(case, tag, gdy, Sdy_ref, ga, gw, got, n_extra=0, pair=None):
    """da, dw, db of one depthwise-backward launch against the fp64 backward of the dy it consumed; pair: the
    unfused launches' outputs a folded launch must agree with"""
    B, T, C, K = case.shape
    da, dw, db, S_da, S_dw, S_db = R.glu_dwconv_bwd(gdy, host(ga), host(gw), B, T, C, K, Sdy_ref)
    bf = case.dtype == BF
    out = [R.check(tag + "da", host(got[0]), da, K + n_extra, S_da, bf),
           R.check(tag + "dw", host(got[1]), dw, B * T + n_extra, S_dw),
           R.check(tag + "db", host(got[2]), db, B * T + n_extra, S_db)]
    if pair is not None:      # same formula, same summation order as the unfused pair
        out += [agree(name, f, u) for name, f, u in zip(("da", "dw", "db"), got, pair)]
    return out


@CASE
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_backward_bn(case, training):
    """cfm_bn_silu_bwd_sums, the unfused cfm_bn_silu_bwd + cfm_glu_dwconv_bwd and the folded cfm_glu_dwconv_bwd_bn"""
    B, T, C, K = case.shape
    M, dt = B * T, R.code(case.dt)
    d = real(case, shifted=False)
    ga, gw, gy, ws = forward(case, d["a"], d["w"], d["bias"])
    gmean, ginv, _, _, _ = bn_forward(case, d, gy, ws, training, case.dtype)
    gg, gbt, gdz = gin(d["gamma"]), gin(d["beta"]), gin(d["dz"], case.dtype)
    stat = (P(gy), P(gg), P(gbt), P(gmean), P(ginv))
    yk, mean, invstd, dz = host(gy), host(gmean), host(ginv), host(gdz)
    norm = (dz, yk, mean, invstd, d["gamma"], d["beta"])
    # the parameter-gradient sums
    gdbeta, gdgamma = gout(1, C), gout(1, C)
    launch("cfm_bn_silu_bwd_sums", P(gdz), dt, *stat, M, C, P(ws), P(gdbeta), P(gdgamma), outs=(gdbeta, gdgamma, ws))
    dbeta, dgamma, Sb, Sg = R.bn_bwd_sums(*norm)
    checks = [R.check("dbeta", host(gdbeta), dbeta, M, Sb), R.check("dgamma", host(gdgamma), dgamma, M, Sg)]
    # unfused: dy, then the plain depthwise backward of that dy
    gdy, gdg2, gdb2 = gout(M, C), gout(1, C), gout(1, C)
    launch("cfm_bn_silu_bwd", P(gdz), dt, *stat, int(training), P(gdy), P(gdg2), P(gdb2), M, C, P(ws),
           outs=(gdy, gdg2, gdb2, ws))
    assert torch.equal(host(gdg2), host(gdgamma)) and torch.equal(host(gdb2), host(gdbeta))
    dy, Sdy = R.bn_bwd_dy(*norm, host(gdbeta), host(gdgamma), M, training)
    checks.append(R.check("dy", host(gdy), dy, R.DY_OPS, Sdy))
    unfused = dwconv_bwd(case, gdy, ga, gw, ws, defer=False)
    checks += backward_stage_checks(case, "unfused ", host(gdy), None, ga, gw, unfused)
    # folded
    args = (P(gdz), dt, *stat, P(gdbeta), P(gdgamma), 1.0 / M, int(training), P(ga), dt, P(gw))
    if not case.folded:
        assert R.plan(R.OPS["bwd_bn"], dt, C, K)[0] == R.UNS
        gda, gdw, gdb = gout(M, 2 * C, case.dtype), gout(C, K), gout(1, C)
        with pytest.raises(_lib.CfmError, match="compiled variant"):
            _lib.call("cfm_glu_dwconv_bwd_bn", *args, P(gda), dt, P(gdw), P(gdb), B, T, C, K, P(ws), _lib.stream())
        torch.cuda.synchronize()
        for g in (gda, gdw, gdb):       # rejected before any launch
            assert_untouched(g, "rejected cfm_glu_dwconv_bwd_bn")
            assert torch.isnan(host(g)).all()
    else:
        assert R.plan(R.OPS["bwd_bn"], dt, C, K, dt_dz=dt)[0] == case.bwd_bn
        folded, deferred = [], []
        for defer, out in ((False, folded), (True, deferred)):
            gda, gdw, gdb = gout(M, 2 * C, case.dtype), gout(C, K), gout(1, C)
            w2 = ws_for(B, T, C, K)
            if defer:
                launch("cfm_glu_dwconv_bwd_bn", *args, P(gda), dt, None, None, B, T, C, K, P(w2), outs=(gda, w2))
                launch("cfm_glu_dwconv_bwd_wgrad", P(w2), B, T, C, K, P(gdw), P(gdb), outs=(gdw, gdb, w2))
            else:
                launch("cfm_glu_dwconv_bwd_bn", *args, P(gda), dt, P(gdw), P(gdb), B, T, C, K, P(w2),
                       outs=(gda, gdw, gdb, w2))
            out += [gda, gdw, gdb]
        checks += backward_stage_checks(case, "folded ", dy, Sdy, ga, gw, folded, R.DY_OPS, pair=unfused)
        same_bits(folded, deferred, "deferred weight gradient")
    print(f"\nbackward, BatchNorm {case.id} {'train' if training else 'eval'}")
    R.assert_all(checks)


@CASE
def test_backward_gn(case):
    """cfm_gn_silu_fwd, cfm_gn_silu_bwd_sums, the unfused cfm_gn_silu_bwd + cfm_glu_dwconv_bwd and the folded
    cfm_glu_dwconv_bwd_gn"""
    B, T, C, K = case.shape
    M, dt = B * T, R.code(case.dt)
    d = real(case, shifted=False)
    ga, gw, gy, ws = forward(case, d["a"], d["w"], d["bias"])
    gg, gbt, gdz = gin(d["gamma"]), gin(d["beta"]), gin(d["dz"], case.dtype)
    gmean, grstd, gz = gout(1, B), gout(1, B), gout(M, C, case.dtype)
    launch("cfm_gn_silu_fwd", P(gy), P(gg), P(gbt), EPS, P(gmean), P(grstd), P(gz), dt, B, T, C, P(ws),
           outs=(gmean, grstd, gz, ws))
    yk, mean, rstd, dz = host(gy), host(gmean), host(grstd), host(gdz)
    mean, rstd = mean.reshape(B), rstd.reshape(B)
    checks = R.check_stats("gn ", R.gn_stats(yk, B, T, C, EPS), mean, rstd)
    z, Sz = R.gn_apply(yk, mean, rstd, d["gamma"], d["beta"], T)
    checks.append(R.check("gn z", host(gz), z, 4, Sz, case.dtype == BF))
    stat = (P(gy), P(gg), P(gbt), P(gmean), P(grstd))
    norm = (dz, yk, mean, rstd, d["gamma"], d["beta"])
    gdbeta, gdgamma, gcoef = gout(1, C), gout(1, C), gout(B, 2)
    launch("cfm_gn_silu_bwd_sums", P(gdz), dt, *stat, B, T, C, P(ws), P(gdbeta), P(gdgamma), P(gcoef),
           outs=(gdbeta, gdgamma, gcoef, ws))
    dbeta, dgamma, coef, Sb, Sg, Sk = R.gn_bwd_sums(*norm, B, T)
    coefk = host(gcoef).reshape(B, 2)
    checks += [R.check("dbeta", host(gdbeta), dbeta, M, Sb), R.check("dgamma", host(gdgamma), dgamma, M, Sg),
               R.check("coef", coefk, coef, T, Sk)]      # per sample: nt partial rows of <= 64 frames, then in double
    gdy, gdg2, gdb2, gcoef2 = gout(M, C), gout(1, C), gout(1, C), gout(B, 2)
    launch("cfm_gn_silu_bwd", P(gdz), dt, *stat, P(gdy), P(gdg2), P(gdb2), P(gcoef2), B, T, C, P(ws),
           outs=(gdy, gdg2, gdb2, gcoef2, ws))
    assert torch.equal(host(gdg2), host(gdgamma)) and torch.equal(host(gdb2), host(gdbeta))
    assert torch.equal(host(gcoef2), host(gcoef))
    dy, Sdy = R.gn_bwd_dy(*norm, coefk, T)
    checks.append(R.check("dy", host(gdy), dy, R.DY_OPS, Sdy))
    unfused = dwconv_bwd(case, gdy, ga, gw, ws, defer=False)
    checks += backward_stage_checks(case, "unfused ", host(gdy), None, ga, gw, unfused)
    if case.folded:
        assert R.plan(R.OPS["bwd_gn"], dt, C, K)[0] == case.bwd_gn
        gda, gdw, gdb = gout(M, 2 * C, case.dtype), gout(C, K), gout(1, C)
        w2 = ws_for(B, T, C, K)
        launch("cfm_glu_dwconv_bwd_gn", P(gdz), dt, *stat, P(gcoef), P(ga), dt, P(gw), P(gda), dt, P(gdw), P(gdb),
               B, T, C, K, P(w2), outs=(gda, gdw, gdb, w2))
        folded = (gda, gdw, gdb)
        checks += backward_stage_checks(case, "folded ", dy, Sdy, ga, gw, folded, R.DY_OPS, pair=unfused)
    else:
        assert R.plan(R.OPS["bwd_gn"], dt, C, K)[0] == R.UNS
    print(f"\nbackward, GroupNorm {case.id}")
    R.assert_all(checks)


# ------------------------------------------------------------------------------------------ SyncBatchNorm, two shards
@pytest.mark.parametrize("T,C,K,dt", [(37, 64, 31, "bf16"), (100, 96, 3, "f32"), (50, 66, 31, "bf16")])
def test_sync_bn_two_shards_in_one_process(T, C, K, dt):
    """B = 4 as two shards of 2: reduce_sums adds the other shard's sums.  The statistics against the fp64 ones of the
    joined batch, everything downstream stage-wise with M_total = 4 T."""
    shard = next(c for c in R.CASES if (c.T, c.C, c.K, c.dt) == (T, C, K, dt))
    shard = R.Case(2, T, C, K, dt, shard.fwd, shard.bwd, shard.bwd_bn, shard.bwd_gn, shard.apply, "shard")
    Ms, Mt, code = 2 * T, 4 * T, R.code(dt)
    d = R.real_inputs(4, T, C, K, torch.Generator().manual_seed(T + C + K))
    gg, gbt = gin(d["gamma"]), gin(d["beta"])
    fw, sums = [], []
    for s in range(2):
        rows = slice(s * Ms, (s + 1) * Ms)
        ga, gw, gy, ws = forward(shard, d["a"][rows], d["w"], d["bias"])
        gs = gout(1, 2 * C)
        launch("cfm_bn_silu_fwd_sums", P(ws), 2, T, C, P(gs), outs=(gs, ws))
        fw.append((ga, gw, gy, ws, gin(d["dz"][rows], shard.dtype)))
        sums.append(gs)
    total = gin(host(sums[0]) + host(sums[1]))                       # the all-reduce
    yk = torch.cat([host(f[2]) for f in fw])
    st = R.bn_stats(yk, Mt, EPS, MOM, d["rm"], d["rv"])
    checks, fwd_out = [], []
    for s in range(2):
        ga, gw, gy, ws, gdz = fw[s]
        grm, grv, gmean, ginv, gz = gstate(d["rm"]), gstate(d["rv"]), gout(1, C), gout(1, C), gout(Ms, C, shard.dtype)
        launch("cfm_bn_silu_fwd_apply", P(gy), P(gg), P(gbt), P(grm), P(grv), MOM, EPS, P(total), Mt, P(gmean),
               P(ginv), P(gz), code, Ms, C, outs=(grm, grv, gmean, ginv, gz))
        checks += R.check_stats(f"shard {s} ", st, host(gmean), host(ginv), host(grm), host(grv), MOM, d["rm"], d["rv"])
        z, Sz = R.bn_apply(host(gy), host(gmean), host(ginv), d["gamma"], d["beta"], 1)
        checks.append(R.check(f"shard {s} z", host(gz), z, 4, Sz, shard.dtype == BF))
        fwd_out.append((gmean, ginv))
    assert torch.equal(host(fwd_out[0][0]), host(fwd_out[1][0])) and torch.equal(host(fwd_out[0][1]), host(fwd_out[1][1]))
    mean, invstd = host(fwd_out[0][0]), host(fwd_out[0][1])
    part = []
    for s in range(2):
        ga, gw, gy, ws, gdz = fw[s]
        gdbeta, gdgamma = gout(1, C), gout(1, C)
        launch("cfm_bn_silu_bwd_sums", P(gdz), code, P(gy), P(gg), P(gbt), P(fwd_out[s][0]), P(fwd_out[s][1]), Ms, C,
               P(ws), P(gdbeta), P(gdgamma), outs=(gdbeta, gdgamma, ws))
        dbeta, dgamma, Sb, Sg = R.bn_bwd_sums(host(gdz), host(gy), mean, invstd, d["gamma"], d["beta"])
        checks += [R.check(f"shard {s} dbeta", host(gdbeta), dbeta, Ms, Sb),
                   R.check(f"shard {s} dgamma", host(gdgamma), dgamma, Ms, Sg)]
        part.append((gdbeta, gdgamma))
    tb, tg = gin(host(part[0][0]) + host(part[1][0])), gin(host(part[0][1]) + host(part[1][1]))
    dz_all = torch.cat([host(f[4]) for f in fw])
    jb, jg, Sjb, Sjg = R.bn_bwd_sums(dz_all, yk, mean, invstd, d["gamma"], d["beta"])      # the joined batch of 4
    checks += [R.check("joined dbeta", host(tb), jb, Mt, Sjb), R.check("joined dgamma", host(tg), jg, Mt, Sjg)]
    for s in range(2):
        ga, gw, gy, ws, gdz = fw[s]
        stat = (P(gy), P(gg), P(gbt), P(fwd_out[s][0]), P(fwd_out[s][1]))
        gdy = gout(Ms, C)
        launch("cfm_bn_silu_bwd_apply", P(gdz), code, *stat, P(tb), P(tg), Mt, P(gdy), Ms, C, outs=(gdy,))
        dy, Sdy = R.bn_bwd_dy(host(gdz), host(gy), mean, invstd, d["gamma"], d["beta"], host(tb), host(tg), Mt, True)
        checks.append(R.check(f"shard {s} dy", host(gdy), dy, R.DY_OPS, Sdy))
        gda, gdw, gdb = gout(Ms, 2 * C, shard.dtype), gout(C, K), gout(1, C)
        w2 = ws_for(2, T, C, K)
        launch("cfm_glu_dwconv_bwd_bn", P(gdz), code, *stat, P(tb), P(tg), 1.0 / Mt, 1, P(ga), code, P(gw), P(gda),
               code, P(gdw), P(gdb), 2, T, C, K, P(w2), outs=(gda, gdw, gdb, w2))
        checks += backward_stage_checks(shard, f"shard {s} folded ", dy, Sdy, ga, gw, (gda, gdw, gdb), R.DY_OPS)
    print(f"\nSyncBatchNorm, two shards 4x{T}x{C}-k{K}-{dt}")
    R.assert_all(checks)


@pytest.mark.parametrize("B,T,C,K,dt", [(2, 37, 64, 31, "bf16"), (1, 100, 96, 3, "f32")])
def test_sync_bn_single_shard_is_the_plain_backward(B, T, C, K, dt):
    """One shard (M_total = M): cfm_bn_silu_bwd_sums then cfm_bn_silu_bwd_apply is cfm_bn_silu_bwd in training mode bit
    for bit -- one apply kernel serves both, forming 1 / M from the row count it is handed (the SyncBatchNorm route
    used to be handed 1 / M_total formed on the host: both are one correctly rounded fp32 division)."""
    row = next(c for c in R.CASES if (c.T, c.C, c.K, c.dt) == (T, C, K, dt))
    case = R.Case(B, T, C, K, dt, row.fwd, row.bwd, row.bwd_bn, row.bwd_gn, row.apply, "single shard")
    M, code = B * T, R.code(dt)
    d = R.real_inputs(B, T, C, K, torch.Generator().manual_seed(B + T + C + K))
    ga, gw, gy, ws = forward(case, d["a"], d["w"], d["bias"])
    gmean, ginv, _, _, _ = bn_forward(case, d, gy, ws, True, case.dtype)
    gg, gbt, gdz = gin(d["gamma"]), gin(d["beta"]), gin(d["dz"], case.dtype)
    stat = (P(gy), P(gg), P(gbt), P(gmean), P(ginv))
    gdy, gdg, gdb = gout(M, C), gout(1, C), gout(1, C)
    launch("cfm_bn_silu_bwd", P(gdz), code, *stat, 1, P(gdy), P(gdg), P(gdb), M, C, P(ws), outs=(gdy, gdg, gdb, ws))
    gdbeta, gdgamma, gdy2 = gout(1, C), gout(1, C), gout(M, C)
    launch("cfm_bn_silu_bwd_sums", P(gdz), code, *stat, M, C, P(ws), P(gdbeta), P(gdgamma), outs=(gdbeta, gdgamma, ws))
    launch("cfm_bn_silu_bwd_apply", P(gdz), code, *stat, P(gdbeta), P(gdgamma), M, P(gdy2), M, C, outs=(gdy2,))
    assert torch.equal(host(gdgamma), host(gdg)) and torch.equal(host(gdbeta), host(gdb))
    assert not torch.isnan(host(gdy)).any()
    assert torch.equal(host(gdy2), host(gdy)), "the sums + apply pair and cfm_bn_silu_bwd differ"


# ------------------------------------------------------------------------------------------ generic BatchNorm
@pytest.mark.parametrize("M,C", R.BN_SHAPES)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("zdt", ZDT)
def test_generic_bn_fwd_bwd(M, C, act, training, zdt):
    """cfm_bn_fwd / cfm_bn_bwd (the projection block's BatchNorm1d): M = 1 in train mode against the plain formula
    (variance 0, running variance as the kernel guards it), fewer rows than the 256 chunks, a ragged last chunk"""
    g = torch.Generator().manual_seed(M * 1000 + C)
    y = torch.randn(M, C, generator=g)
    ratio = torch.tensor(R.RATIOS)[torch.arange(C) % 4]
    if M > 1:       # channel means at |mean| / sigma = 0, 4, 16, 64
        y = y * (1 + torch.arange(C) % 3)[None, :] + ratio[None, :] * (1 + torch.arange(C) % 3)[None, :]
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    dz = torch.randn(M, C, generator=g)
    gy, gg, gbt, gdz = gin(y), gin(gamma), gin(beta), gin(dz, zdt)
    grm, grv, gmean, ginv, gz = gstate(rm), gstate(rv), gout(1, C), gout(1, C), gout(M, C, zdt)
    ws = gout(1, _lib.size_call("cfm_bn_ws_bytes", C) // 4)
    launch("cfm_bn_fwd", P(gy), P(gg), P(gbt), P(grm), P(grv), MOM, EPS, int(training), P(gmean), P(ginv), P(gz),
           R.code(zdt), M, C, act, P(ws), outs=(grm, grv, gmean, ginv, gz, ws))
    mean, invstd = host(gmean), host(ginv)
    if training:
        st = R.bn_stats(y, M, EPS, MOM, rm, rv)
        checks = R.check_stats("", st, mean, invstd, host(grm), host(grv), MOM, rm, rv)
    else:
        ev = R.eval_stats(rm, rv, EPS)
        assert torch.equal(mean, rm) and torch.equal(host(grm), rm) and torch.equal(host(grv), rv)
        checks = [R.within("invstd (eval)", invstd, ev.invstd, 4 * R.U24 * ev.invstd)]
    z, Sz = R.bn_apply(y, mean, invstd, gamma, beta, act)
    checks.append(R.check("z", host(gz).reshape(M, C), z, 4, Sz, zdt == BF))
    gdy, gdgamma, gdbeta = gout(M, C), gout(1, C), gout(1, C)
    launch("cfm_bn_bwd", P(gdz), R.code(zdt), P(gy), P(gg), P(gbt), P(gmean), P(ginv), int(training), act, P(gdy),
           P(gdgamma), P(gdbeta), M, C, P(ws), outs=(gdy, gdgamma, gdbeta, ws))
    dzk = host(gdz).reshape(M, C)
    dbeta, dgamma, Sb, Sg = R.bn_bwd_sums(dzk, y, mean, invstd, gamma, beta, act)
    dy, Sdy = R.bn_bwd_dy(dzk, y, mean, invstd, gamma, beta, host(gdbeta), host(gdgamma), M, training, act)
    checks += [R.check("dbeta", host(gdbeta), dbeta, M, Sb), R.check("dgamma", host(gdgamma), dgamma, M, Sg),
               R.check("dy", host(gdy).reshape(M, C), dy, R.DY_OPS, Sdy)]
    print(f"\ngeneric BatchNorm {M}x{C} act {act} {'train' if training else 'eval'}")
    R.assert_all(checks)
