"""The BatchNorm kernels (csrc/ocm_bn.hip) one entry point at a time against
float64: ocm_bn_fwd_train, ocm_bn_bwd and ocm_bn_fwd_eval through the C ABI,
then FastBatchNorm1d against torch.nn.BatchNorm1d in float64 with autograd.

Every reference is computed on the CPU in float64 on exactly the values the
kernel read: bf16 inputs are rounded first and then widened, float32
parameters (γ, β, ε, momentum, the running statistics, save_mean and
save_invstd of the backward) are widened as they are.  The backward is tested
as its own entry point: x, dy, y, save_mean and save_invstd are independent
random inputs and the reference is the formula of include/ocm.h.

Which shape reaches which kernel and which lap of its loop (bn_split(C) is 256
for C ≤ 8, 170 for C = 12, 64 for C ≥ 32; "8-wide" = L % 8 = 0 and every
pointer 16-byte aligned; t = the float32 terms one thread adds, T_TERMS):

  (1, 3, 1)        k_bn_stats + k_bn_apply, k_bn_bwd_stats + k_bn_bwd_apply; M = 1: var = 0, unb = var
  (1, 1, 8)        k_bn_stats8 + k_bn_apply8, k_bn_bwd_stats8 + k_bn_bwd_apply8 with bn_split8 = 1:
  (2, 3, 8)          one workgroup per channel, one ticket, one thread holds the channel
  (7, 5, 33)       the scalar kernels, ragged rows; 255 of the 256 workgroups per channel are empty
  (125, 2, 1088)   8-wide, bn_split8 = 17: the last ticket subgroup holds one workgroup; 17000 groups,
                   4 per thread in one lap (two laps of k_bn_bwd_stats8), the last of them partial
  (64, 12, 512)    8-wide with C = 12 (bn_split8 = 4); offset by one element the scalar kernels with
                   bn_split = 170 (ticket subgroups of 16 and a last one of 10); dx alone misaligned:
                   k_bn_bwd_stats8 + k_bn_bwd_apply
  (129, 32, 4120)  8-wide, 66435 groups > 64·1024: second lap of k_bn_stats8 with 899 groups (zero
                   padding of bn_ld8_or0), third partial lap of k_bn_bwd_stats8
  (257, 32, 1023)  scalar, 262911 = 2·131072 + 767 elements: third lap of k_bn_stats / k_bn_bwd_stats
                   with 767 elements (zero padding of bn_ld_or0)
  (3, 12, 33), (2, 12, 8)   the scratch-reuse sequence: scalar with split 170, 8-wide with split 1
  eval (3, 5, 33), (2, 3, 16), (5, 3, 24)   k_bn_eval<V = 1> and <V = 8> (offset by one element: V = 1)

The one-launch kernels (k_bn_fused8, k_bn_bwd_fused8) are an opt-in experiment with a
child-process test of their own in tests/test_vae_train.py; nothing here selects them.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

DEV = torch.device("cuda", 0)
F32, BF16 = 0, 1  # include/ocm.h OCM_DTYPE_*
ACT_NONE, ACT_ELU = 0, 1  # OCM_ACT_*
EPS, MOM = 1e-5, 0.1
EPS32, MOM32 = float(np.float32(EPS)), float(np.float32(MOM))  # as the kernels read them

# ---- tolerances ------------------------------------------------------------
U = 2.0 ** -24  # the unit roundoff of float32: one rounding moves a value by at most U·|value|
# Elementwise outputs (y of the forward and of eval, dx), float32:
#   y = fma(x, a, b), a = fl(invstd·γ), b = fl(β − fl(μ·a)), invstd and μ stored as float32.
#   a carries two roundings (the stored invstd, the product): 2U on |x·a| and on |μ·a|; the stored
#   mean, the product μ·a and the subtraction one each on |μ·a|, the subtraction one on |β|; the
#   fma rounds once, ≤ U·(|x·a| + |μ·a| + |β|).  Together 3U·|x·a| + 6U·|μ·a| + 2U·|β|.  (Eval forms
#   invstd = 1 / sqrtf(rv + ε) in float32: 2.5U in place of the stored invstd's U, 6.5U on |μ·a|.)
#   C_ELEM = 8 leaves 2U of every term for the accumulation error of the statistics themselves.
#   The bound is in the terms' magnitudes, not in |y|: that is the contract of the fma form.
#   dx = k·(dz − m1 − x̂·m2): x̂ = fl(fl(x − μ)·invstd) 2U, m2 and the product one each, the two
#   subtractions and the product with k = fl(invstd·γ) one each on their operands, dz of the ELU
#   branch fl(dy·fl(y + 1)) 2U: ≤ 5U·|dz| + 3U·|m1| + 7U·|x̂·m2|, times |k|.  The same constant.
#   This form asks m1 = Σdz/M and m2 = Σdz·x̂/M to be right to a float32 ulp or so of THEMSELVES, though
#   both sums cancel to ~ √M of M terms: the elements with dz ≈ 0 and x̂ ≈ 0 see nothing else.  With
#   float32 accumulators (the kernels before this file) the sums were off by up to 17 ulps of
#   themselves and dx reached 3.1 times its bound at (129, 32, 4120); they are f64 now (float
#   inputs: the terms too; bf16 inputs keep float32 terms, whose random roundings leave the sums
#   within an ulp or so of themselves on these inputs, not for every cancellation).
#   Measured worst error / bound on an MI355X: y 0.37, 0.86 with |μ|/σ = 100; dx 0.63; eval y 0.29;
#   through the module y 0.29 and dx 0.53.
C_ELEM = 8
# ELU branch: expf within one float32 ulp of a value ≤ 1 and the rounding of expf(z) − 1
ELU_ABS = 2 * U
# Statistics and parameter gradients (save_mean, save_invstd, running_mean, running_var, dγ, dβ) are
# float64 sums of per-thread float32 accumulators.  A thread that adds t float32 terms rounds t − 1
# times (the fma chain of Σx² and of Σdz·x̂: t times), each by at most U of the running sum of
# absolute terms: ≤ t·U·Σ|term| over the channel.  Two more U for the terms themselves (x̂ and the
# ELU's dz are float32 results), then one float32 rounding of the stored result:
#   |mean − ref| ≤ (t + 2)·U·Σ|x|/M + U·|ref|
#   |var − ref|  ≤ (t + 2)·U·Σx²/M, i.e. relative (t + 2)·U·(1 + (μ/σ)²); half of that (relative, plus
#                  U) for save_invstd = 1/√(var + ε), momentum·that·M/(M − 1) plus U·|ref| for running_var
#   |dβ − ref| ≤ (t + 2)·U·Σ|dz| + U·|ref|,  |dγ − ref| ≤ (t + 2)·U·Σ|dz·x̂| + U·|ref|
# never the absolute value of the sum.  t is read off the kernel's constants (T_TERMS below).
# (The backward's sums are f64 per thread since this file; its bounds stay as derived for float32.)
# Measured worst error / bound on an MI355X: save_mean 0.23, save_invstd 0.29, running_mean 0.51,
# running_var 0.82 (all at shapes with t = 1, where the bound is three or four roundings; 0.31 at
# t = 40), dγ 0.26, dβ 0.19.
ACC_EXTRA = 2
# bf16 outputs: the float32 value rounded to nearest, i.e. half a bf16 ulp of the reference plus the
# float32 term above: tests/test_gpu_vaestep.py _assert_bf16_rounded, reused as it is (no tie
# exemption, no cap on skipped elements).  Measured worst error / bound: 1.000 (a rounding to
# nearest reaches its half ulp).

# the kernel's constants (csrc/ocm_bn.hip)
BN_T, BN_U, BN_U8, BN_SPLIT, BN_SPLIT_MAX = 256, 8, 4, 64, 256


def bn_split(C):
    return min(max(2048 // C, BN_SPLIT), BN_SPLIT_MAX)


def bn_split8(N, C, L):
    g8 = N * (L // 8)
    return max(1, min(-(-g8 // (BN_T * BN_U8)), bn_split(C)))


# (N, C, L): (t of the 8-wide reductions, t of the scalar reductions).  A scalar thread takes the
# elements e ≡ its index mod bn_split·256: ceil(N·L / (bn_split·256)) of them; an 8-wide thread
# the 8-element groups ≡ its index mod bn_split8·256: 8·ceil(N·L/8 / (bn_split8·256)) elements.
T_TERMS = {
    (1, 3, 1): (None, 1),
    (1, 1, 8): (8, 1),
    (2, 3, 8): (8, 1),
    (7, 5, 33): (None, 1),
    (125, 2, 1088): (32, 3),
    (64, 12, 512): (32, 1),
    (129, 32, 4120): (40, 33),
    (257, 32, 1023): (None, 17),
    (3, 12, 33): (None, 1),
    (2, 12, 8): (8, 1),
}


def _t(shape, vec):
    """The largest number of float32 terms one thread adds: the table's entry, checked
    against the kernel's launch geometry."""
    N, C, L = shape
    t8 = 8 * -(-(N * (L // 8)) // (bn_split8(N, C, L) * BN_T)) if L % 8 == 0 else None
    t1 = -(-(N * L) // (bn_split(C) * BN_T))
    assert T_TERMS[shape] == (t8, t1), (shape, t8, t1)
    assert not vec or t8 is not None
    return t8 if vec else t1


def _vs():
    """The bf16 helpers of tests/test_gpu_vaestep.py (_assert_bf16_rounded asserts half a
    bf16 ulp of the reference plus the float32 term)."""
    import test_gpu_vaestep

    return test_gpu_vaestep


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _lib():
    from ocm import _lib as L

    return L


def _h():
    return _lib().Context.get(DEV.index).handle


# ---- tensors carved out of flat buffers between sentinels -------------------
PAD = 64  # elements before and after: 128 bytes of bf16, 256 of float32, so offset 0 stays 16-byte aligned
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
_SENT = {torch.float32: 0x7FA5A5A5, torch.bfloat16: 0x7FA5}  # NaNs: an element left unwritten shows too


def _flat(n, dtype, off=0):
    """(buffer, view): n elements at element offset PAD + off of a sentinel-filled flat buffer."""
    buf = torch.full((PAD + off + n + PAD,), _SENT[dtype], dtype=_INT[dtype], device=DEV).view(dtype)
    view = buf[PAD + off:PAD + off + n]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (off * buf.element_size()) % 16
    return buf, view


def _put(t, off=0):
    buf, view = _flat(t.numel(), t.dtype, off)
    view.copy_(t.reshape(-1))
    return buf, view


def _assert_pads(buf, off, n, what):
    bits = buf.view(_INT[buf.dtype]).cpu()
    s = _SENT[buf.dtype]
    assert bool((bits[:PAD + off] == s).all()) and bool((bits[PAD + off + n:] == s).all()), \
        f"{what}: a sentinel beside it was overwritten"


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _scratch(C):
    nbytes = int(_lib().load().ocm_bn_scratch_bytes(C))
    return torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=DEV)


# ---- inputs ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(N, C, L, bf16, ratio=2.0):
    """Host inputs of one shape, as the kernels read them.  x = μ_c + σ_c·randn with a different
    μ_c and σ_c per channel and |μ_c|/σ_c ≤ 2 (ratio > 2: |μ_c|/σ_c = ratio, the common-offset
    case).  The backward's dy, y, save_mean and save_invstd are independent of any forward."""
    g = _gen(9000 + 7919 * N + 131 * C + L + (1 if bf16 else 0))
    sig = torch.linspace(0.5, 3.0, C) if C > 1 else torch.tensor([0.75])
    sign = torch.tensor([(-1.0) ** c for c in range(C)])
    frac = torch.tensor([0.25 + 0.75 * ((5 * c) % 8) / 7 for c in range(C)])
    mu = ratio * sign * (frac if ratio <= 2 else 1.0) * sig
    x = mu[None, :, None] + sig[None, :, None] * torch.randn(N, C, L, generator=g)
    dy = torch.randn(N, C, L, generator=g)
    yin = 1.5 * torch.randn(N, C, L, generator=g) - 0.25  # an ELU output in its own right: both branches
    special = torch.tensor([0.0, -0.0, -90.0])[:min(3, L)]
    yin[0, 0, :special.numel()] = special
    if bf16:
        x, dy, yin = (t.to(torch.bfloat16) for t in (x, dy, yin))
    return dict(
        shape=(N, C, L), bf16=bf16, key=(N, C, L, bf16, ratio), x=x, dy=dy, yin=yin,
        smean_in=(mu + 0.1 * sig * torch.randn(C, generator=g)).float(),
        sinv_in=((0.8 + 0.4 * torch.rand(C, generator=g)) / sig).float(),
        gamma=(sign * torch.linspace(0.5, 1.5, C)).float(), beta=torch.linspace(-0.2, 0.3, C).float(),
        rm0=(0.5 * torch.randn(C, generator=g)).float(), rv0=(0.5 + torch.rand(C, generator=g)).float())


# ---- float64 references, one channel at a time ------------------------------
def _fwd_channel(xc, mean, inv, g, b, act):
    """(reference, float32 term) of y for one channel: xc float64, the rest Python floats."""
    a = g * inv
    z = (xc - mean) * a + b
    ref = torch.where(z > 0, z, torch.expm1(z)) if act else z
    term = C_ELEM * U * ((xc * a).abs() + abs(mean * a) + abs(b)) + (ELU_ABS if act else 0.0)
    return ref, term


def _dz_channel(dyc, yc, act):
    return dyc * torch.where(yc > 0, torch.ones_like(yc), yc + 1.0) if act else dyc


def _bwd_channel(xc, dyc, yc, mu, inv, g, act):
    """One channel of the backward by include/ocm.h's formula, in float64: the reference
    dx, its float32 term, dβ, dγ, Σ|dz| and Σ|dz·x̂|."""
    M = xc.numel()
    xh = (xc - mu) * inv
    dz = _dz_channel(dyc, yc, act)
    db, dg = float(dz.sum()), float((dz * xh).sum())
    k, m1, m2 = g * inv, db / M, dg / M
    ref = k * (dz - m1 - xh * m2)
    term = C_ELEM * U * abs(k) * (dz.abs() + abs(m1) + (xh * m2).abs())
    return ref, term, db, dg, float(dz.abs().sum()), float((dz * xh).abs().sum())


@functools.lru_cache(maxsize=None)
def _stats_ref(key):
    """Float64 statistics of every channel of _case(*key): mean, biased variance, Σ|x|, Σx²."""
    x = _case(*key)["x"]
    mean, var, sabs, ssq = [], [], [], []
    for c in range(x.shape[1]):
        v = x[:, c, :].double()
        mean.append(float(v.mean()))
        var.append(float(((v - mean[-1]) ** 2).mean()))
        sabs.append(float(v.abs().sum()))
        ssq.append(float((v * v).sum()))
    return dict(mean=np.array(mean), var=np.array(var), sabs=np.array(sabs), ssq=np.array(ssq))


_WORST = {}


def _note(what, ratio):
    _WORST[what] = max(_WORST.get(what, 0.0), float(ratio))
    print(f"[bn] {what}: err / bound = {float(ratio):.3f}")


def _assert_elem(got, ref, term, bf16, what):
    """got (float64 tensor of the kernel's output) within the float32 term of ref, or for
    a bf16 output within half a bf16 ulp of the reference plus that term."""
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    if bf16:
        _vs()._assert_bf16_rounded(got.numpy(), ref.numpy(), term.numpy(), what)
        return
    err = (got - ref).abs()
    _note(what, (err / term).max())
    assert bool((err <= term).all()), what


def _assert_vec(got, ref, bound, what):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    _note(what, (err / bound).max())
    assert (err <= bound).all(), f"{what}: {got} against {ref}, bound {bound}"


def _stat_bounds(st, M, t, rm0, rv0):
    """References and bounds of the forward's per-channel outputs (the derivation above)."""
    acc = (t + ACC_EXTRA) * U
    mean, var = st["mean"], st["var"]
    mean_e, var_e = acc * st["sabs"] / M, acc * st["ssq"] / M
    inv = 1.0 / np.sqrt(var + EPS32)
    f = M / (M - 1.0) if M > 1 else 1.0
    rm = (1.0 - MOM32) * rm0 + MOM32 * mean
    rv = (1.0 - MOM32) * rv0 + MOM32 * var * f
    return dict(mean=(mean, mean_e + U * np.abs(mean)), inv=(inv, inv * (0.5 * var_e / (var + EPS32) + U)),
                rm=(rm, MOM32 * mean_e + U * np.abs(rm)), rv=(rv, MOM32 * var_e * f + U * np.abs(rv)))


# ---- the entry points --------------------------------------------------------
def _run_fwd(case, act, x_off=0, y_off=0, gamma=True, beta=True, running=True, nbt=41, scratch=None):
    """ocm_bn_fwd_train on tensors carved at the given element offsets; every output lies
    between sentinels, which must survive.  Results on the host."""
    L_ = _lib()
    N, C, L = case["shape"]
    n = N * C * L
    _, xv = _put(case["x"], x_off)
    yb, yv = _flat(n, case["x"].dtype, y_off)
    g = case["gamma"].to(DEV) if gamma else None
    b = case["beta"].to(DEV) if beta else None
    smb, sm = _flat(C, torch.float32)
    sib, si = _flat(C, torch.float32)
    rmb, rm = _put(case["rm0"]) if running else (None, None)
    rvb, rv = _put(case["rv0"]) if running else (None, None)
    nb = torch.tensor([nbt, -7], dtype=torch.int64, device=DEV) if nbt is not None else None
    scratch = _scratch(C) if scratch is None else scratch
    rc = L_.load().ocm_bn_fwd_train(_h(), BF16 if case["bf16"] else F32, L_.ptr(xv), N, C, L, L_.ptr(g), L_.ptr(b),
                                    EPS, MOM, L_.ptr(rm), L_.ptr(rv), L_.ptr(nb), act, L_.ptr(yv), L_.ptr(sm),
                                    L_.ptr(si), L_.ptr(scratch), L_.stream_handle(DEV))
    L_.check(rc, "ocm_bn_fwd_train")
    torch.cuda.synchronize()
    _assert_pads(yb, y_off, n, "y")
    _assert_pads(smb, 0, C, "save_mean")
    _assert_pads(sib, 0, C, "save_invstd")
    if running:
        _assert_pads(rmb, 0, C, "running_mean")
        _assert_pads(rvb, 0, C, "running_var")
    if nb is not None:
        assert int(nb[1]) == -7
    return dict(y=yv.cpu().view(N, C, L), smean=sm.cpu(), sinv=si.cpu(), rm=rm.cpu() if running else None,
                rv=rv.cpu() if running else None, nbt=int(nb[0]) if nb is not None else None)


def _check_fwd(case, out, act, t, tag, gamma=True, beta=True):
    N, C, L = case["shape"]
    st = _stats_ref(case["key"])
    sb = _stat_bounds(st, N * L, t, case["rm0"].double().numpy(), case["rv0"].double().numpy())
    _assert_vec(out["smean"], *sb["mean"], f"{tag} save_mean")
    _assert_vec(out["sinv"], *sb["inv"], f"{tag} save_invstd")
    if out["rm"] is not None:
        _assert_vec(out["rm"], *sb["rm"], f"{tag} running_mean")
        _assert_vec(out["rv"], *sb["rv"], f"{tag} running_var")
    for c in range(C):
        ref, term = _fwd_channel(case["x"][:, c, :].double(), float(st["mean"][c]), float(sb["inv"][0][c]),
                                 float(case["gamma"][c]) if gamma else 1.0, float(case["beta"][c]) if beta else 0.0,
                                 act)
        _assert_elem(out["y"][:, c, :].double(), ref, term, case["bf16"], f"{tag} y[{c}]")


def _run_bwd(case, act, x_off=0, dy_off=0, y_off=0, dx_off=0, gamma=True, dgamma=True, dbeta=True, scratch=None):
    """ocm_bn_bwd on independent inputs; dx, dγ and dβ between sentinels."""
    L_ = _lib()
    N, C, L = case["shape"]
    n = N * C * L
    _, xv = _put(case["x"], x_off)
    _, dyv = _put(case["dy"], dy_off)
    yv = _put(case["yin"], y_off)[1] if act else None
    dxb, dxv = _flat(n, case["x"].dtype, dx_off)
    g = case["gamma"].to(DEV) if gamma else None
    sm, si = case["smean_in"].to(DEV), case["sinv_in"].to(DEV)
    dgb, dg = _flat(C, torch.float32) if dgamma else (None, None)
    dbb, db = _flat(C, torch.float32) if dbeta else (None, None)
    scratch = _scratch(C) if scratch is None else scratch
    rc = L_.load().ocm_bn_bwd(_h(), BF16 if case["bf16"] else F32, L_.ptr(xv), L_.ptr(dyv), N, C, L, L_.ptr(g),
                              L_.ptr(sm), L_.ptr(si), act, L_.ptr(yv), L_.ptr(dxv), L_.ptr(dg), L_.ptr(db),
                              L_.ptr(scratch), L_.stream_handle(DEV))
    L_.check(rc, "ocm_bn_bwd")
    torch.cuda.synchronize()
    _assert_pads(dxb, dx_off, n, "dx")
    if dgamma:
        _assert_pads(dgb, 0, C, "dgamma")
    if dbeta:
        _assert_pads(dbb, 0, C, "dbeta")
    return dict(dx=dxv.cpu().view(N, C, L), dgamma=dg.cpu() if dgamma else None, dbeta=db.cpu() if dbeta else None)


def _check_bwd(case, out, act, t, tag, gamma=True):
    N, C, L = case["shape"]
    acc = (t + ACC_EXTRA) * U
    dbs, dgs, sdz, sdzx = [], [], [], []
    for c in range(C):
        ref, term, db, dg, a1, a2 = _bwd_channel(
            case["x"][:, c, :].double(), case["dy"][:, c, :].double(), case["yin"][:, c, :].double(),
            float(case["smean_in"][c]), float(case["sinv_in"][c]), float(case["gamma"][c]) if gamma else 1.0, act)
        _assert_elem(out["dx"][:, c, :].double(), ref, term, case["bf16"], f"{tag} dx[{c}]")
        dbs.append(db), dgs.append(dg), sdz.append(a1), sdzx.append(a2)
    dbs, dgs, sdz, sdzx = (np.array(v) for v in (dbs, dgs, sdz, sdzx))
    if out["dbeta"] is not None:
        _assert_vec(out["dbeta"], dbs, acc * sdz + U * np.abs(dbs), f"{tag} dbeta")
    if out["dgamma"] is not None:
        _assert_vec(out["dgamma"], dgs, acc * sdzx + U * np.abs(dgs), f"{tag} dgamma")


def _name(case, act):
    return f"{case['shape']} {'bf16' if case['bf16'] else 'f32'} {'elu' if act else 'none'}"


# ---------------------------------------------------------------------------
# 1. values, path by path
# ---------------------------------------------------------------------------
SMALL = [(1, 3, 1), (1, 1, 8), (2, 3, 8), (7, 5, 33), (125, 2, 1088), (64, 12, 512)]
LARGE = [(129, 32, 4120), (257, 32, 1023)]  # the multi-lap shapes: once per dtype, ELU on
VALUE_CASES = [(s, bf, act) for s in SMALL for bf in (False, True) for act in (ACT_NONE, ACT_ELU)] + \
              [(s, bf, ACT_ELU) for s in LARGE for bf in (False, True)]
VALUE_IDS = [f"{s[0]}x{s[1]}x{s[2]}-{'bf16' if bf else 'f32'}-{'elu' if act else 'none'}" for s, bf, act in VALUE_CASES]


@pytest.mark.parametrize("shape,bf16,act", VALUE_CASES, ids=VALUE_IDS)
def test_fwd_train_matches_float64(shape, bf16, act):
    """y, save_mean, save_invstd, running_mean, running_var and num_batches_tracked of
    ocm_bn_fwd_train against float64 statistics."""
    case = _case(*shape, bf16)
    out = _run_fwd(case, act)
    _check_fwd(case, out, act, _t(shape, shape[2] % 8 == 0), "fwd " + _name(case, act))
    assert out["nbt"] == 42
    if shape[0] * shape[2] == 1:
        # M = 1: the mean is x itself, the variance 0 (bf16: x² is exact in float32), unb = var, and
        # the reference y is β (ELU: of β) exactly
        assert torch.equal(out["smean"], case["x"].float().view(-1))
        st = _stats_ref(case["key"])
        assert (st["var"] == 0).all()
        ref, _ = _fwd_channel(case["x"][:, 0, :].double(), float(st["mean"][0]), 1.0 / np.sqrt(EPS32),
                              float(case["gamma"][0]), float(case["beta"][0]), ACT_NONE)
        assert float(ref) == float(case["beta"][0])
        if bf16:
            assert float(out["sinv"][0]) == float(np.float32(1.0 / np.sqrt(EPS32)))
            np.testing.assert_array_equal(out["rv"].numpy(), ((1.0 - MOM32) * case["rv0"].double()).float().numpy())


@pytest.mark.parametrize("shape,bf16,act", VALUE_CASES, ids=VALUE_IDS)
def test_bwd_matches_float64(shape, bf16, act):
    """dx, dγ and dβ of ocm_bn_bwd on independent x, dy, y, save_mean and save_invstd
    against the formula of include/ocm.h in float64."""
    case = _case(*shape, bf16)
    out = _run_bwd(case, act)
    _check_bwd(case, out, act, _t(shape, shape[2] % 8 == 0), "bwd " + _name(case, act))


@pytest.mark.parametrize("shape", [(125, 2, 1088), (7, 5, 33)], ids=["8wide", "scalar"])
def test_fwd_train_common_offset(shape):
    """|μ|/σ = 100, float32: the variance is Σx²/M − mean² with Σx² in float32 per thread, so
    its relative error grows as (μ/σ)²·2⁻²⁴·t.  The derived bounds hold as they stand
    ((t + 2)·2⁻²⁴·(1 + 10⁴) relative for the variance); the measured errors are printed.
    On an MI355X: variance 3.5e-5 relative at (125, 2, 1088) (t = 32) and 3.3e-5 at
    (7, 5, 33) (t = 1, one term per thread: the float32 rounding of each x² alone); y is
    off by at most 1.2e-4 and 4.6e-5 absolute, 0.86 and 0.48 of its bound."""
    N, C, L = shape
    case = _case(N, C, L, False, 100.0)
    st = _stats_ref(case["key"])
    assert np.allclose(np.abs(st["mean"]) / np.sqrt(st["var"]), 100.0, rtol=0.2)
    outs = {}
    for act in (ACT_NONE, ACT_ELU):
        outs[act] = _run_fwd(case, act)
        _check_fwd(case, outs[act], act, _t(shape, L % 8 == 0), f"offset fwd {_name(case, act)}")
    out = outs[ACT_NONE]
    var_k = 1.0 / out["sinv"].double().numpy() ** 2 - EPS32  # (the stored invstd's rounding: 1.2e-7 of it)
    inv_ref = 1.0 / np.sqrt(st["var"] + EPS32)
    yerr = 0.0
    for c in range(C):
        ref, _ = _fwd_channel(case["x"][:, c, :].double(), float(st["mean"][c]), float(inv_ref[c]),
                              float(case["gamma"][c]), float(case["beta"][c]), ACT_NONE)
        yerr = max(yerr, float((out["y"][:, c, :].double() - ref).abs().max()))
    print(f"[bn] common offset {shape}: relative error of the variance {np.abs(var_k / st['var'] - 1.0).max():.3e} "
          f"(bound {(_t(shape, L % 8 == 0) + ACC_EXTRA) * U * (1 + 100.0 ** 2):.3e}), "
          f"largest absolute error of y {yerr:.3e}")


# ---------------------------------------------------------------------------
# 2. eval
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 33), (2, 3, 16), (5, 3, 24)])
def test_fwd_eval_matches_float64(shape, bf16):
    """ocm_bn_fwd_eval (k_bn_eval with V = 8 and V = 1): aligned and offset by one element,
    γ/β given and NULL, with and without the ELU."""
    L_ = _lib()
    N, C, L = shape
    n = N * C * L
    case = _case(N, C, L, bf16)
    rm, rv = case["rm0"], case["rv0"]
    inv = 1.0 / np.sqrt(rv.double().numpy() + EPS32)
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    for off in (0, 1):
        for affine in (True, False):
            for act in (ACT_NONE, ACT_ELU):
                _, xv = _put(case["x"], off)
                yb, yv = _flat(n, case["x"].dtype, off)
                g = case["gamma"].to(DEV) if affine else None
                b = case["beta"].to(DEV) if affine else None
                rc = L_.load().ocm_bn_fwd_eval(_h(), BF16 if bf16 else F32, L_.ptr(xv), N, C, L, L_.ptr(rmd),
                                               L_.ptr(rvd), EPS, L_.ptr(g), L_.ptr(b), act, L_.ptr(yv),
                                               L_.stream_handle(DEV))
                L_.check(rc, "ocm_bn_fwd_eval")
                torch.cuda.synchronize()
                _assert_pads(yb, off, n, "eval y")
                y = yv.cpu().view(N, C, L)
                for c in range(C):
                    ref, term = _fwd_channel(case["x"][:, c, :].double(), float(rm[c]), float(inv[c]),
                                             float(case["gamma"][c]) if affine else 1.0,
                                             float(case["beta"][c]) if affine else 0.0, act)
                    _assert_elem(y[:, c, :].double(), ref, term, bf16,
                                 f"eval {shape} off {off} affine {affine} act {act} y[{c}]")


# ---------------------------------------------------------------------------
# 3. alignment
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 8), (64, 12, 512)])
def test_misaligned_tensors_take_the_scalar_kernels(shape, bf16):
    """L % 8 = 0 with one tensor at a time (then all) one element into its flat buffer: 4
    bytes in float32, 2 in bf16, either breaks the 16-byte alignment the 8-wide kernels
    need.  Same bounds (with the t of the kernel the dispatcher picks), sentinels intact
    (_run_fwd / _run_bwd assert them).  dx alone misaligned: k_bn_bwd_stats8 followed by
    the scalar k_bn_bwd_apply."""
    case = _case(*shape, bf16)
    for act in (ACT_NONE, ACT_ELU):
        for offs in (dict(x_off=1), dict(y_off=1), dict(x_off=1, y_off=1)):
            out = _run_fwd(case, act, **offs)
            _check_fwd(case, out, act, _t(shape, False), f"fwd {_name(case, act)} {offs}")
        variants = [dict(x_off=1), dict(dy_off=1), dict(dx_off=1), dict(x_off=1, dy_off=1, y_off=1, dx_off=1)]
        if act:
            variants.append(dict(y_off=1))
        for offs in variants:
            out = _run_bwd(case, act, **offs)
            # dx alone (and y without the ELU, which is not read): the 8-wide reduction
            vec = set(offs) == {"dx_off"}
            _check_bwd(case, out, act, _t(shape, vec), f"bwd {_name(case, act)} {offs}")


def test_scalar_path_fingerprint():
    """The scalar reductions hand element e = n·L + l of a channel to a thread by e alone,
    so their sums depend on the channel's sequence of values and not on how N·L factors;
    the 8-wide reductions add in another order.  (64, 12, 512) offset by one element must
    therefore give the very bits of the same sequences laid out as (8192, 12, 4), which
    only the scalar kernels can take, and the aligned 8-wide call gives other bits
    somewhere: the dispatcher did send the misaligned tensors to the scalar kernels."""
    case = _case(64, 12, 512, False)
    N, C, L = case["shape"]
    re = dict(case, shape=(N * L // 4, C, 4))
    for k in ("x", "dy", "yin"):
        re[k] = case[k].permute(1, 0, 2).reshape(C, N * L // 4, 4).permute(1, 0, 2).contiguous()
    keys_f, keys_b = ("smean", "sinv", "rm", "rv"), ("dgamma", "dbeta")
    f_off, f_re, f_al = _run_fwd(case, ACT_ELU, x_off=1), _run_fwd(re, ACT_ELU), _run_fwd(case, ACT_ELU)
    b_off, b_re, b_al = _run_bwd(case, ACT_ELU, x_off=1), _run_bwd(re, ACT_ELU), _run_bwd(case, ACT_ELU)
    assert all(torch.equal(_bits(f_off[k]), _bits(f_re[k])) for k in keys_f)
    assert all(torch.equal(_bits(b_off[k]), _bits(b_re[k])) for k in keys_b)
    # (the backward's sums are accumulated in float64 per thread and round to the same float32 either way)
    same = [torch.equal(_bits(f_off[k]), _bits(f_al[k])) for k in keys_f]
    assert not all(same), "the 8-wide and the scalar reductions gave the same bits: the input tells nothing apart"


# ---------------------------------------------------------------------------
# 4. nullable arguments, the batch counter, argument errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(7, 5, 33), (2, 3, 8)])
def test_nullable_arguments(shape, bf16):
    """γ/β NULL (affine=False), the running statistics NULL (track_running_stats=False),
    num_batches_tracked NULL, dγ or dβ NULL singly: what is given is still right."""
    case = _case(*shape, bf16)
    t = _t(shape, shape[2] % 8 == 0)
    for act in (ACT_NONE, ACT_ELU):
        tag = _name(case, act)
        for gam, bet in ((False, False), (False, True), (True, False)):
            out = _run_fwd(case, act, gamma=gam, beta=bet)
            _check_fwd(case, out, act, t, f"fwd {tag} gamma {gam} beta {bet}", gamma=gam, beta=bet)
        out = _run_fwd(case, act, running=False)
        assert out["rm"] is None and out["nbt"] == 42
        _check_fwd(case, out, act, t, f"fwd {tag} running NULL")
        out = _run_fwd(case, act, nbt=None)
        _check_fwd(case, out, act, t, f"fwd {tag} nbt NULL")
        out = _run_bwd(case, act, gamma=False)
        _check_bwd(case, out, act, t, f"bwd {tag} gamma NULL", gamma=False)
        for dg, db in ((False, True), (True, False), (False, False)):
            out = _run_bwd(case, act, dgamma=dg, dbeta=db)
            assert (out["dgamma"] is None) == (not dg) and (out["dbeta"] is None) == (not db)
            _check_bwd(case, out, act, t, f"bwd {tag} dgamma {dg} dbeta {db}")


@pytest.mark.parametrize("C", [1, 5, 32])
def test_num_batches_tracked_rises_by_one_per_call(C):
    """Channel 0's last workgroup counts the batch: exactly once whatever C is."""
    case = _case(3, C, 40, False)
    L_ = _lib()
    N, _, L = case["shape"]
    x = case["x"].to(DEV)
    y = torch.empty_like(x)
    sm, si = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm, rv = case["rm0"].to(DEV), case["rv0"].to(DEV)
    nb = torch.tensor([-9, 2 ** 40 + 5, -9], dtype=torch.int64, device=DEV)
    scratch = _scratch(C)
    for k in (1, 2, 3):
        rc = L_.load().ocm_bn_fwd_train(_h(), F32, L_.ptr(x), N, C, L, None, None, EPS, MOM, L_.ptr(rm), L_.ptr(rv),
                                        L_.ptr(nb[1:]), ACT_NONE, L_.ptr(y), L_.ptr(sm), L_.ptr(si), L_.ptr(scratch),
                                        L_.stream_handle(DEV))
        L_.check(rc, "ocm_bn_fwd_train")
        assert nb.tolist() == [-9, 2 ** 40 + 5 + k, -9]


def test_argument_errors():
    """Bad shapes (N·L ≥ 2³¹ − 1 by the shape alone: the check precedes any launch), an unknown
    dtype or act, the ELU backward without y, running_mean without running_var: an
    argument error each, nothing written."""
    L_ = _lib()
    lib = L_.load()
    bufs = [torch.full((64,), 7.0, device=DEV) for _ in range(12)]
    x, dy, yin, y, dx, gam, bet, sm, si, rm_, rv_, dgb = (L_.ptr(v) for v in bufs)
    i64 = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    scratch = _scratch(2)
    s, st = L_.ptr(scratch), L_.stream_handle(DEV)

    def fwd(N=2, C=2, L=8, dtype=F32, act=ACT_NONE, rm=rm_, rv=rv_):
        return lib.ocm_bn_fwd_train(_h(), dtype, x, N, C, L, gam, bet, EPS, MOM, rm, rv, L_.ptr(i64), act, y, sm, si,
                                    s, st)

    def bwd(N=2, C=2, L=8, dtype=F32, act=ACT_NONE, y=yin):
        return lib.ocm_bn_bwd(_h(), dtype, x, dy, N, C, L, gam, sm, si, act, y, dx, dgb, dgb + 64, s, st)

    def ev(N=2, C=2, L=8, dtype=F32, act=ACT_NONE):
        return lib.ocm_bn_fwd_eval(_h(), dtype, x, N, C, L, rm_, rv_, EPS, gam, bet, act, y, st)

    bad_shapes = [dict(N=0), dict(C=0), dict(L=0), dict(N=-1), dict(C=-3), dict(L=-8)]
    too_long = [dict(N=65536, C=1, L=32768), dict(N=1, C=1, L=2 ** 31 - 1), dict(N=2 ** 31 - 1, C=1, L=1)]
    calls = [(fwd, kw) for kw in bad_shapes + too_long] + [(bwd, kw) for kw in bad_shapes + too_long] + \
            [(ev, kw) for kw in bad_shapes] + \
            [(f, dict(dtype=d)) for f in (fwd, bwd, ev) for d in (2, -1)] + \
            [(f, dict(act=a)) for f in (fwd, bwd, ev) for a in (2, -1)] + \
            [(bwd, dict(act=ACT_ELU, y=None)), (fwd, dict(rv=None)), (fwd, dict(rm=None))]
    for f, kw in calls:
        with pytest.raises(ValueError):
            L_.check(f(**kw), f"{f.__name__} {kw}")
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in bufs) and int(i64) == 7 and bool((scratch == 0).all())
    # and the calls are fine as they stand
    for f in (fwd, bwd, ev):
        L_.check(f(), f.__name__)
    L_.check(bwd(act=ACT_ELU), "bwd elu")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 5. determinism and the scratch contract
# ---------------------------------------------------------------------------
_FWD_KEYS = ("y", "smean", "sinv", "rm", "rv")
_BWD_KEYS = ("dx", "dgamma", "dbeta")


def _same_bits(a, b, keys, what):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in bits"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(125, 2, 1088), (257, 32, 1023), (129, 32, 4120)])
def test_two_calls_give_the_same_bits(shape, bf16):
    """"fixed-order combine: deterministic": every output of two calls on the same inputs
    is identical, whichever workgroup arrives last."""
    case = _case(*shape, bf16)
    _same_bits(_run_fwd(case, ACT_ELU), _run_fwd(case, ACT_ELU), _FWD_KEYS, f"fwd {shape}")
    _same_bits(_run_bwd(case, ACT_ELU), _run_bwd(case, ACT_ELU), _BWD_KEYS, f"bwd {shape}")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_one_scratch_serves_every_split_count(bf16):
    """"every call leaves them zero", through the ABI alone: one zero-filled scratch for
    C = 12 runs 4 workgroups per channel (8-wide), 170 (scalar, ticket subgroups of 16 and
    10, most of them empty), 170 again on the first shape offset by one element, and 1; each result equals the same call on a freshly
    zeroed scratch bit for bit.  A counter left non-zero would end a later reduction early
    or never."""
    shared = _scratch(12)
    for shape, off in (((64, 12, 512), 0), ((3, 12, 33), 0), ((64, 12, 512), 1), ((2, 12, 8), 0)):
        case = _case(*shape, bf16)
        _t(shape, False)
        offs_f = dict(x_off=off, y_off=off)
        offs_b = dict(x_off=off, dy_off=off, y_off=off, dx_off=off)
        _same_bits(_run_fwd(case, ACT_ELU, scratch=shared, **offs_f), _run_fwd(case, ACT_ELU, **offs_f), _FWD_KEYS,
                   f"fwd {shape} off {off}")
        _same_bits(_run_bwd(case, ACT_ELU, scratch=shared, **offs_b), _run_bwd(case, ACT_ELU, **offs_b), _BWD_KEYS,
                   f"bwd {shape} off {off}")


# ---------------------------------------------------------------------------
# 6. FastBatchNorm1d against torch.nn.BatchNorm1d in float64 with autograd
# ---------------------------------------------------------------------------
MODULE_KINDS = ["no_affine", "no_running_stats", "offset_view"]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", MODULE_KINDS)
@pytest.mark.parametrize("shape", [(7, 5, 33), (64, 12, 512)])
def test_module_matches_float64_batchnorm(shape, kind, bf16):
    """affine=False, track_running_stats=False, and a contiguous view that starts one
    element into a flat buffer: outputs, input gradients, parameter gradients and buffers
    against nn.BatchNorm1d in float64 on the CPU, at the bounds above.  (Without the fused
    ELU: its backward starts from the stored, rounded output, which these bounds do not
    describe; test_bwd_matches_float64 covers that formula on the values the kernel reads.)
    The backward here runs on the forward's own float32 statistics: their stored rounding
    moves x̂ by U·|x̂| and by U·|μ|/σ, constant over the channel, so it reaches dγ as
    U·|dγ| + U·(|μ|/σ)·|dβ| and dx inside its 2U of slack (the derivation at C_ELEM)."""
    from ocm.bn import FastBatchNorm1d

    N, C, L = shape
    M = N * L
    case = _case(N, C, L, bf16)
    affine, track = kind != "no_affine", kind != "no_running_stats"
    act = ACT_NONE
    off = 1 if kind == "offset_view" else 0
    t = _t(shape, L % 8 == 0 and not off)
    ref_m = torch.nn.BatchNorm1d(C, eps=EPS32, momentum=MOM32, affine=affine, track_running_stats=track).double()
    fast = FastBatchNorm1d(C, eps=EPS, momentum=MOM, affine=affine, track_running_stats=track).to(DEV)
    with torch.no_grad():
        if affine:
            ref_m.weight.copy_(case["gamma"].double()), ref_m.bias.copy_(case["beta"].double())
            fast.weight.copy_(case["gamma"]), fast.bias.copy_(case["beta"])
        if track:
            ref_m.running_mean.copy_(case["rm0"].double()), ref_m.running_var.copy_(case["rv0"].double())
            fast.running_mean.copy_(case["rm0"]), fast.running_var.copy_(case["rv0"])
    # the float64 module
    x64 = case["x"].double().requires_grad_(True)
    gy = case["dy"]
    y64 = ref_m(x64)
    (y64 * gy.double()).sum().backward()
    # FastBatchNorm1d on the device
    _, xv = _put(case["x"], off)
    xd = xv.view(N, C, L).detach().requires_grad_(True)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == (off * xd.element_size()) % 16
    y = fast(xd)
    assert y.dtype == xd.dtype
    (y.float() * gy.to(DEV).float()).sum().backward()
    torch.cuda.synchronize()
    tag = f"module {kind} {_name(case, act)}"
    st = _stats_ref(case["key"])
    sb = _stat_bounds(st, M, t, case["rm0"].double().numpy(), case["rv0"].double().numpy())
    inv = sb["inv"][0]
    yk, dxk = y.detach().cpu(), xd.grad.cpu()
    dbs, dgs, sdz, sdzx = [], [], [], []
    for c in range(C):
        g, b = (float(case["gamma"][c]), float(case["beta"][c])) if affine else (1.0, 0.0)
        xc = case["x"][:, c, :].double()
        yh, yterm = _fwd_channel(xc, float(st["mean"][c]), float(inv[c]), g, b, act)
        # the written-out formulas are the module's, to float64 accuracy
        assert float((yh - y64.detach()[:, c, :]).abs().max()) <= 1e-12 * float(yterm.max()) / U
        _assert_elem(yk[:, c, :].double(), y64.detach()[:, c, :], yterm, bf16, f"{tag} y[{c}]")
        dxh, dxterm, db, dg, a1, a2 = _bwd_channel(xc, gy[:, c, :].double(), y64.detach()[:, c, :], float(st["mean"][c]),
                                                   float(inv[c]), g, act)
        assert float((dxh - x64.grad[:, c, :]).abs().max()) <= 1e-12 * float(dxterm.max()) / U
        _assert_elem(dxk[:, c, :].double(), x64.grad[:, c, :], dxterm, bf16, f"{tag} dx[{c}]")
        dbs.append(db), dgs.append(dg), sdz.append(a1), sdzx.append(a2)
    dbs, dgs, sdz, sdzx = (np.array(v) for v in (dbs, dgs, sdz, sdzx))
    acc = (t + ACC_EXTRA) * U
    if affine:
        assert np.allclose(ref_m.bias.grad.numpy(), dbs, rtol=1e-10, atol=1e-10 * sdz.max())
        assert np.allclose(ref_m.weight.grad.numpy(), dgs, rtol=1e-10, atol=1e-10 * sdzx.max())
        _assert_vec(fast.bias.grad.cpu(), ref_m.bias.grad.numpy(), acc * sdz + U * np.abs(dbs), f"{tag} bias.grad")
        _assert_vec(fast.weight.grad.cpu(), ref_m.weight.grad.numpy(), acc * sdzx + U * np.abs(dgs),
                    f"{tag} weight.grad")
    else:
        assert fast.weight is None and fast.bias is None
    if track:
        assert np.allclose(ref_m.running_mean.numpy(), sb["rm"][0], rtol=1e-12, atol=1e-14)
        assert np.allclose(ref_m.running_var.numpy(), sb["rv"][0], rtol=1e-12, atol=1e-14)
        _assert_vec(fast.running_mean.cpu(), ref_m.running_mean.numpy(), sb["rm"][1], f"{tag} running_mean")
        _assert_vec(fast.running_var.cpu(), ref_m.running_var.numpy(), sb["rv"][1], f"{tag} running_var")
        assert int(fast.num_batches_tracked) == int(ref_m.num_batches_tracked) == 1
    else:
        assert fast.running_mean is None and fast.running_var is None and fast.num_batches_tracked is None


def test_module_rejects_one_value_per_channel():
    """N·L = 1 in training mode: nn.BatchNorm1d raises ValueError and so does
    FastBatchNorm1d, before it launches (the C entry point keeps its documented M = 1
    behaviour: test_fwd_train_matches_float64 at (1, 3, 1))."""
    from ocm.bn import FastBatchNorm1d

    x = torch.randn(1, 3, 1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        torch.nn.BatchNorm1d(3)(x)
    fast = FastBatchNorm1d(3).to(DEV)
    before = {k: v.clone() for k, v in fast.state_dict().items()}
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        fast(x.to(DEV))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        fast.fuse_elu()(x.to(DEV).bfloat16())
    assert all(torch.equal(v, before[k]) for k, v in fast.state_dict().items())
    fast.eval()
    assert fast(x.to(DEV)).shape == (1, 3, 1)  # eval mode takes one value per channel, as torch's does
