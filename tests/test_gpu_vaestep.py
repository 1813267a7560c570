"""The VAE step's fused kernels (csrc/ocm_vaestep.hip, and ocm_chan_sum of
csrc/ocm_conv.hip) one entry point at a time against float64 references.

Every reference is the project's own definition (vae_model.py: kl_term,
bce_recon_term, mse_recon_term, reparameterize written out with a given ε;
torch's ELU; torch's Adam formula) evaluated on the CPU in float64 on exactly
the values the kernel read (bf16 inputs are rounded first, then widened), with
autograd for every gradient.  Shapes are the smallest that reach each code
path: row tails, more than 512 partials of a ticket reduction, a last ticket
subgroup that is not full, the second piece of k_recon_fwd's register loop,
the grid-stride laps of k_adam and k_cast_multi.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

DEV = torch.device("cuda", 0)

# ---- tolerances ------------------------------------------------------------
F32_ULP_REL = 2.0 ** -23  # one float32 ulp relative to a value at the bottom of its binade
# an fp64 sum rounded to float32 once (½ ulp), leaving room for the order of the partials
SUM_F32_ULPS = 4 * F32_ULP_REL  # 4.8e-7
# elementwise float32 formulas: ≈ 8 float32 ulps of the terms' magnitude (a float32 NumPy
# emulation of the same formulas gave 1.0e-7 and 1.7e-7; the rest is the device's expf)
ELEM_F32 = 1e-6
# bf16 outputs: the float32 value rounded to nearest, i.e. half a bf16 ulp.  bf16 keeps 8
# significand bits, so half an ulp is 2⁻⁹ of the top of a binade and 2⁻⁸ of its bottom: the
# unit roundoff is 2⁻⁸, not 2⁻⁹ (torch's own conversion of the float64 reference z reaches
# 0.996·2⁻⁸ on these inputs, and a fifth of its elements lie above 2⁻⁹·(1 + 2⁻⁶)).  The exact
# half ulp of each reference value is asserted (_bf16_half_ulp); this constant is the relative
# form of it, with 2⁻⁶ of headroom for a float32 value that sits beside a binade edge.
BF16_REL = 2.0 ** -8 * (1 + 2.0 ** -6)
# mean signed relative error of a round-to-nearest bf16 output over 131 k elements
# (truncation instead would show ≈ 2⁻⁹)
BF16_MEAN_SIGNED = 2.0 ** -12
# the recon term: an fp64 sum of float32 terms that carry a few ulps each (emulation: 5e-9
# for BCE at (5, 2049)); also covers MSE's single squared rounding
RECON_REL = 1e-6
# d recon / d xs: float32 sigmoid, target and scale, each a few ulps of values ≤ 1
# (emulation: 1.5e-7), in units of std_j / (B·L); MSE: of 2(|x̂| + |x|)·std_j / (B·L)
GXS_REL = 1e-6
# standardise: the float32 quotient of the float32 difference, within 2 float32 ulps
STD_ULPS = 2
# a bf16 result may differ from the rounded reference only where the reference's float32
# value lies within this many float32 ulps of a bf16 tie, and in at most this share of the
# elements (a tie window of 5 in 65536 float32 values: 0.008 % expected)
TIE_ULPS = 2
TIE_CAP = 0.005
# Adam: float32 β₂ makes 1 − β₂ᵗ up to 1.3e-5 relative off at t = 1, the square root halves
# that; the rest covers the float32 rounding of the ratio
ADAM_P_REL_LR = 5e-5
ADAM_P_ULPS = 2
ADAM_M_ULPS = 4

DKL = float(np.float32(0.7))  # cotangent of the KL (as the float32 the kernel reads)
BETA = 0.7
DTOTAL = 0.37
KL_IN = 1.7320508


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _u16(t):
    """The bit patterns of a bf16 tensor (host, uint16)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _u32(t):
    """The bit patterns of a float32 tensor (host, uint32)."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _bf16_half_ulp(v):
    """Half a bf16 ulp at |v| (float64 array): 2^(e − 8) for 2^e ≤ |v| < 2^(e+1),
    never below half the denormal spacing 2⁻¹³³."""
    _, e = np.frexp(np.abs(v))  # |v| = m·2^e, ½ ≤ m < 1
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 8)


def _assert_bf16_rounded(got, ref64, f32_term, what):
    """|got − ref| ≤ half a bf16 ulp of the float32 value (which lies within f32_term of
    the reference) + f32_term, and the same in relative form (BF16_REL)."""
    got, ref64, f32_term = (np.asarray(a, dtype=np.float64) for a in (got, ref64, f32_term))
    err = np.abs(got - ref64)
    tight = _bf16_half_ulp(np.abs(ref64) + f32_term) + f32_term
    rel = BF16_REL * np.abs(ref64) + f32_term
    print(f"{what}: max err / (half bf16 ulp + f32 term) = {float((err / tight).max()):.3f}, "
          f"max err / |ref| = {float((err / np.maximum(np.abs(ref64), 1e-300)).max()):.3e}")
    assert (err <= tight).all(), what
    assert (err <= rel).all(), what


def _assert_rounds_to_bf16(got_bf16, ref64, what):
    """``got_bf16`` is bit-equal to torch's bf16 rounding of float32(ref64), except where
    that float32 lies within TIE_ULPS ulps of a bf16 tie: there one bf16 ulp off is
    allowed, in at most TIE_CAP of the elements (the reference alone must meet the cap)."""
    ref32 = torch.from_numpy(np.ascontiguousarray(ref64, dtype=np.float64)).to(torch.float32)
    want = _u16(ref32.to(torch.bfloat16)).astype(np.int64).ravel()
    got = _u16(got_bf16).astype(np.int64).ravel()
    low = (_u32(ref32).astype(np.int64) & 0xffff).ravel()
    near = np.abs(low - 0x8000) <= TIE_ULPS
    assert near.mean() <= TIE_CAP, f"{what}: the reference itself has {near.mean():.4f} near ties (seed)"
    mism = got != want
    print(f"{what}: {int(mism.sum())} of {mism.size} differ from the rounded reference, {int(near.sum())} near ties")
    assert not (mism & ~near).any(), f"{what}: {int((mism & ~near).sum())} wrong roundings away from ties"
    assert mism.mean() <= TIE_CAP, what

    def order(b):  # sign-magnitude bits → ordered integers
        return np.where(b & 0x8000, -(b & 0x7fff), b & 0x7fff)

    assert (np.abs(order(got) - order(want))[mism] <= 1).all(), f"{what}: more than one bf16 ulp off"


# ---------------------------------------------------------------------------
# 1. bottleneck
# ---------------------------------------------------------------------------
BNECK_SHAPES = [(1, 1), (37, 5), (1089, 4), (2049, 64), (16384, 64)]


@functools.lru_cache(maxsize=None)
def _bneck_case(B, d, bf16):
    """Inputs (as the kernel reads them) and the float64 reference: z, kl, and the
    gradients of Σ dz·z and of dkl·kl separately (they add; either alone is the
    reference with the other cotangent zero)."""
    import vae_model as V

    g = _gen(1000 + 131 * B + d)
    mu = 2.0 * torch.randn(B, d, generator=g)
    lv = torch.rand(B, d, generator=g) * 30.0 - 20.0
    eps = torch.randn(B, d, generator=g)
    dz = torch.randn(B, d, generator=g)
    if bf16:
        mu, lv, eps, dz = (t.to(torch.bfloat16) for t in (mu, lv, eps, dz))
    mu64, lv64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    eps64, dz64 = eps.double(), dz.double()
    z = mu64 + eps64 * torch.exp(0.5 * lv64)  # reparameterize (vae_model.py) with the given ε
    kl = V.kl_term(mu64, lv64)
    dmu_z, dlv_z = torch.autograd.grad(z, [mu64, lv64], dz64, retain_graph=True)
    dmu_k, dlv_k = torch.autograd.grad(kl, [mu64, lv64], torch.tensor(DKL, dtype=torch.float64))
    ref = dict(z=z.detach().numpy(), kl=float(kl.detach()), dmu_z=dmu_z.numpy(), dlv_z=dlv_z.numpy(),
               dmu_k=dmu_k.numpy(), dlv_k=dlv_k.numpy())
    m, l, e, gz = (t.double().numpy() for t in (mu, lv, eps, dz))
    mag = dict(z=np.abs(m) + np.abs(e) * np.exp(0.5 * l),
               dmu_z=np.abs(gz), dmu_k=np.abs(DKL * m) / B,
               dlv_z=np.abs(gz * e * 0.5 * np.exp(0.5 * l)), dlv_k=0.5 * abs(DKL) * (1.0 + np.exp(l)) / B)
    return dict(mu=mu, lv=lv, eps=eps, dz=dz, ref=ref, mag=mag)


def _bneck_run(case, packed, use_dz=True, use_dkl=True):
    """(z, kl, dmu, dlv) of the kernels, on the host; a cotangent that is not
    used reaches the backward kernel as NULL."""
    from ocm import vae_fused as vf

    d = case["mu"].shape[1]
    eps = case["eps"].to(DEV)
    if packed:
        ml = torch.cat([case["mu"], case["lv"]], 1).to(DEV).requires_grad_(True)
        z, kl = vf.bottleneck_packed(ml, eps)
        inputs = [ml]
    else:
        mu, lv = case["mu"].to(DEV).requires_grad_(True), case["lv"].to(DEV).requires_grad_(True)
        z, kl = vf.bottleneck(mu, lv, eps)
        inputs = [mu, lv]
    outs, cots = [], []
    if use_dz:
        outs.append(z)
        cots.append(case["dz"].to(DEV))
    if use_dkl:
        outs.append(kl)
        cots.append(torch.tensor(DKL, dtype=torch.float32, device=DEV))
    grads = torch.autograd.grad(outs, inputs, cots)
    if packed:
        dmu, dlv = grads[0][:, :d], grads[0][:, d:]
    else:
        dmu, dlv = grads
    assert z.dtype == case["mu"].dtype and dmu.dtype == case["mu"].dtype and kl.dtype == torch.float32
    return z.detach().cpu(), kl.detach().cpu(), dmu.detach().cpu(), dlv.detach().cpu()


def _bneck_check_fwd(case, z, kl, tag):
    ref, mag = case["ref"], case["mag"]
    bf16 = case["mu"].dtype == torch.bfloat16
    zk = z.double().numpy()
    assert np.isfinite(zk).all()
    if bf16:
        _assert_bf16_rounded(zk, ref["z"], ELEM_F32 * mag["z"], f"{tag} z")
    else:
        err = np.abs(zk - ref["z"]) / mag["z"]
        print(f"{tag} z: max err / s = {float(err.max()):.3e} (bound {ELEM_F32})")
        assert (np.abs(zk - ref["z"]) <= ELEM_F32 * mag["z"]).all(), tag
    rel = abs(float(kl) - ref["kl"]) / abs(ref["kl"])
    print(f"{tag} kl: rel err {rel:.3e} (bound {SUM_F32_ULPS:.2e})")
    assert rel <= SUM_F32_ULPS, tag


def _bneck_check_bwd(case, dmu, dlv, use_dz, use_dkl, tag):
    ref, mag = case["ref"], case["mag"]
    bf16 = case["mu"].dtype == torch.bfloat16
    for name, got in (("dmu", dmu), ("dlv", dlv)):
        want = (ref[name + "_z"] if use_dz else 0.0) + (ref[name + "_k"] if use_dkl else 0.0)
        m = (mag[name + "_z"] if use_dz else 0.0) + (mag[name + "_k"] if use_dkl else 0.0)
        gk = got.double().numpy()
        assert np.isfinite(gk).all()
        if bf16:
            _assert_bf16_rounded(gk, want, ELEM_F32 * m, f"{tag} {name}")
        else:
            print(f"{tag} {name}: max err / terms = {float((np.abs(gk - want) / m).max()):.3e} (bound {ELEM_F32})")
            assert (np.abs(gk - want) <= ELEM_F32 * m).all(), (tag, name)


def _mean_signed_rel(got, ref64):
    nz = ref64 != 0
    return float(((got[nz] - ref64[nz]) / ref64[nz]).mean())


@pytest.mark.parametrize("packed", [False, True], ids=["separate", "packed"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,d", BNECK_SHAPES)
def test_bottleneck_matches_float64(B, d, bf16, packed):
    """z, kl, dμ and dlogσ² of ocm_vae_bottleneck_fwd/_bwd(_ld) against float64, with both
    cotangents, with dz = NULL and with dkl = NULL."""
    case = _bneck_case(B, d, bf16)
    tag = f"bottleneck ({B}, {d}) {'bf16' if bf16 else 'f32'} {'packed' if packed else 'separate'}"
    z, kl, dmu, dlv = _bneck_run(case, packed)
    _bneck_check_fwd(case, z, kl, tag)
    _bneck_check_bwd(case, dmu, dlv, True, True, tag)
    if bf16 and (B, d) == (2049, 64):
        ref = case["ref"]
        for name, got, want in (("z", z, ref["z"]), ("dmu", dmu, ref["dmu_z"] + ref["dmu_k"]),
                                ("dlv", dlv, ref["dlv_z"] + ref["dlv_k"])):
            ms = _mean_signed_rel(got.double().numpy(), want)
            print(f"{tag} {name}: mean signed rel err {ms:.3e} (bound {BF16_MEAN_SIGNED:.3e})")
            assert abs(ms) < BF16_MEAN_SIGNED, name
    _, _, dmu, dlv = _bneck_run(case, packed, use_dz=False)
    _bneck_check_bwd(case, dmu, dlv, False, True, tag + " dz=NULL")
    _, _, dmu, dlv = _bneck_run(case, packed, use_dkl=False)
    _bneck_check_bwd(case, dmu, dlv, True, False, tag + " dkl=NULL")


def test_bottleneck_shared_scratch_and_determinism():
    """One scratch buffer per device serves every grid size: a completion counter
    left non-zero by one size would break the next.  Two calls on the same
    inputs give the same bits."""
    for B, d in [(2049, 64), (1, 1), (1089, 4), (37, 5)]:
        case = _bneck_case(B, d, False)
        z, kl, _, _ = _bneck_run(case, False)
        _bneck_check_fwd(case, z, kl, f"scratch order ({B}, {d})")
        z2, kl2, _, _ = _bneck_run(case, False)
        assert np.array_equal(_u32(z), _u32(z2)) and np.array_equal(_u32(kl), _u32(kl2)), (B, d)


def test_bottleneck_rejects_more_than_4096_workgroups():
    """B·d = 2²⁰ + 256 is one workgroup past the scratch: an error, nothing launched."""
    from ocm import _lib
    from ocm import vae_fused as vf

    B, d = 4097, 256
    assert B * d == 2 ** 20 + 256
    mu = torch.zeros(B, d, device=DEV)
    z = torch.full((B, d), 7.0, device=DEV)
    kl = torch.full((), 7.0, device=DEV)
    rc = _lib.load().ocm_vae_bottleneck_fwd(vf._h(DEV), 0, mu.data_ptr(), mu.data_ptr(), mu.data_ptr(), B, d,
                                            z.data_ptr(), kl.data_ptr(), vf._bottleneck_scratch(DEV).data_ptr(),
                                            _lib.stream_handle(DEV))
    with pytest.raises(ValueError):
        _lib.check(rc, "ocm_vae_bottleneck_fwd")
    torch.cuda.synchronize()
    assert float(kl) == 7.0 and bool((z == 7.0).all())
    with pytest.raises(ValueError):
        vf.bottleneck(mu, mu, mu)
    # the scratch is untouched: the next call is right
    case = _bneck_case(37, 5, False)
    zz, kk, _, _ = _bneck_run(case, False)
    _bneck_check_fwd(case, zz, kk, "after the rejected call")


# ---------------------------------------------------------------------------
# 2. reconstruction term
# ---------------------------------------------------------------------------
RECON_SHAPES = [(1, 1), (3, 255), (17, 256), (5, 2049), (33, 4100), (513, 7)]
XS_SPECIALS = [0.0, -0.0, 40.0, -40.0, 90.0, -90.0, 1e-6, -1e-6]


@functools.lru_cache(maxsize=None)
def _recon_case(B, L, loss, bf16):
    import vae_model as V

    g = _gen(2000 + 17 * B + L)
    x = 1.0 + 0.3 * torch.randn(B, L, generator=g)
    x[B - 1] = x[B - 1, 0].clone()  # a constant row: hi − lo + eps = eps
    xs = 3.0 * torch.randn(B, L, generator=g)
    n = min(len(XS_SPECIALS), L)
    xs[0, :n] = torch.tensor(XS_SPECIALS[:n])
    mean = 1.0 + 0.1 * torch.randn(L, generator=g)
    std = 0.05 + 0.45 * torch.rand(L, generator=g)
    if bf16:
        xs = xs.to(torch.bfloat16)
    xs64 = xs.double().requires_grad_(True)
    xhat = xs64 * std.double() + mean.double()
    recon = V.bce_recon_term(x.double(), xhat) if loss == "bce" else V.mse_recon_term(x.double(), xhat)
    (gxs,) = torch.autograd.grad(recon, xs64)
    return dict(x=x, xs=xs, mean=mean, std=std, recon=float(recon.detach()), gxs=gxs.numpy(),
                xhat=xhat.detach().numpy())


def _recon_run(case, loss, with_kl):
    from ocm import vae_fused as vf

    B, L = case["x"].shape
    bufs = vf.ReconBuffers(case["mean"].to(DEV), case["std"].to(DEV))
    x = case["x"].to(DEV)
    xs = case["xs"].to(DEV).requires_grad_(True)
    kl = torch.tensor(KL_IN, dtype=torch.float32, device=DEV, requires_grad=True) if with_kl else None
    total, recon = vf.recon_total(x, xs, kl, bufs, loss, BETA)
    gxs, out2 = bufs.get(B, L, DEV)[0].clone().cpu(), bufs.get(B, L, DEV)[1].clone().cpu()
    assert float(total.detach()) == float(out2[0]) and float(recon) == float(out2[1])
    grads = torch.autograd.grad(total, [xs, kl] if with_kl else [xs], torch.tensor(DTOTAL, device=DEV))
    dxs = grads[0].cpu()
    dkl = grads[1].cpu() if with_kl else None
    return out2, gxs, dxs, dkl


@pytest.mark.parametrize("bf16", [False, True], ids=["xs_f32", "xs_bf16"])
@pytest.mark.parametrize("loss", ["bce", "euclidean"])
@pytest.mark.parametrize("B,L", RECON_SHAPES)
def test_recon_total_matches_float64(B, L, loss, bf16):
    """ocm_vae_recon_fwd / _bwd: the term, total = recon + β·kl (kl given and NULL), the
    kept gradient d recon / d xs elementwise, and the backward's single multiply."""
    case = _recon_case(B, L, loss, bf16)
    tag = f"recon ({B}, {L}) {loss} {'bf16' if bf16 else 'f32'}"
    std = case["std"].double().numpy()
    if loss == "bce":
        gbound = GXS_REL * std / (B * L) * np.ones((B, 1))
    else:
        gbound = GXS_REL * 2.0 * (np.abs(case["xhat"]) + np.abs(case["x"].double().numpy())) * std / (B * L)
    beta32 = float(np.float32(BETA))
    for with_kl in (True, False):
        out2, gxs, dxs, dkl = _recon_run(case, loss, with_kl)
        total, recon = float(out2[0]), float(out2[1])
        g = gxs.double().numpy()
        assert np.isfinite(g).all() and np.isfinite(total) and np.isfinite(recon)
        rel = abs(recon - case["recon"]) / abs(case["recon"])
        gerr = float((np.abs(g - case["gxs"]) / gbound).max())
        print(f"{tag} kl={'given' if with_kl else 'NULL'}: recon rel err {rel:.3e} (bound {RECON_REL}), "
              f"max gxs err / bound unit = {gerr * GXS_REL:.3e} (bound {GXS_REL})")
        assert rel <= RECON_REL, tag
        assert (np.abs(g - case["gxs"]) <= gbound).all(), tag
        klv = float(np.float32(KL_IN)) if with_kl else 0.0
        if with_kl:
            terr = abs(total - (recon + beta32 * klv))
            tb = SUM_F32_ULPS * (abs(recon) + beta32 * abs(klv))
            print(f"{tag}: |total − (recon + β·kl)| = {terr:.3e} (bound {tb:.3e})")
            assert terr <= tb, tag
        else:
            assert total == recon, tag
        # the backward: one float32 multiply per element, β·dtotal for the KL
        want = np.float32(DTOTAL) * gxs.numpy()
        if bf16:
            assert dxs.dtype == torch.bfloat16
            assert np.array_equal(_u16(dxs), _u16(torch.from_numpy(want).to(torch.bfloat16))), tag
        else:
            assert np.array_equal(_u32(dxs), want.view(np.uint32)), tag
        if with_kl:
            assert np.array_equal(_u32(dkl), np.array(np.float32(BETA) * np.float32(DTOTAL)).view(np.uint32)), tag
        # a second call gives the same bits
        out2b, gxsb, dxsb, _ = _recon_run(case, loss, with_kl)
        assert np.array_equal(_u32(out2), _u32(out2b)) and np.array_equal(_u32(gxs), _u32(gxsb)), tag
        assert torch.equal(dxs, dxsb), tag


# ---------------------------------------------------------------------------
# 3. standardise
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _std_case(B, L):
    g = _gen(3000 + 7 * B + L)
    x = 1.0 + 0.3 * torch.randn(B, L, generator=g)
    mean = 1.0 + 0.1 * torch.randn(L, generator=g)
    std = 0.05 + 0.45 * torch.rand(L, generator=g)
    diff = x.numpy() - mean.numpy()  # the float32 subtraction (IEEE, as the kernel's)
    assert diff.dtype == np.float32
    ref = diff.astype(np.float64) / std.double().numpy()
    return x, mean, std, ref


@pytest.mark.parametrize("B,L", [(1, 1), (7, 33), (3, 2049)])
def test_standardise_matches_float64(B, L):
    from ocm import vae_fused as vf

    x, mean, std, ref = _std_case(B, L)
    xd, md, sd = x.to(DEV), mean.to(DEV), std.to(DEV)
    out = vf.standardise(xd, md, sd, dtype=torch.float32).cpu().numpy()
    ulps = np.abs(out.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"standardise ({B}, {L}) f32: max err {float(ulps.max()):.3f} ulps (bound {STD_ULPS})")
    assert (ulps <= STD_ULPS).all()
    outb = vf.standardise(xd, md, sd, dtype=torch.bfloat16)
    assert outb.dtype == torch.bfloat16 and outb.shape == (B, L)
    _assert_rounds_to_bf16(outb, ref, f"standardise ({B}, {L}) bf16")


# ---------------------------------------------------------------------------
# 4. cast_multi
# ---------------------------------------------------------------------------
CAST_SIZES = [0, 1, 255, 256, 257, 70001, 3, 1023, 1024, 1025, 7, 64, 65, 4097, 511, 0, 513, 2, 33, 100, 12345, 8, 9,
              129, 2047, 2049, 5, 31, 200003, 640, 19, 0]
# ±0, the smallest and largest denormals, ties to even and to odd, the largest finite value
# (rounds to inf), ±inf, the default NaN
CAST_SPECIALS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x3f808000, 0x3f818000,
                 0xbf808000, 0xbf818000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000]
# NaNs whose payload sits (also) in the low 16 bits: truncation would make ±inf of the first four
CAST_NANS = [0x7f800001, 0xff80ffff, 0x7f80ffff, 0xff800001, 0x7fbfffff, 0x7f808000, 0xffc00001, 0x7fffffff]


def _from_bits32(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.int32)).view(torch.float32)


def test_cast_multi_f32_to_bf16_bit_exact_and_nan_stays_nan():
    """ocm_cast_multi over 32 tensors (empty ones first, in the middle and last; the
    total takes the grid-stride loop into a second lap): float32 → bf16 equals torch's
    conversion bit for bit, and every NaN stays a NaN (a payload in the low 16 bits must
    not become ±inf)."""
    from ocm import vae_fused as vf

    assert len(CAST_SIZES) == 32 and CAST_SIZES[0] == CAST_SIZES[15] == CAST_SIZES[-1] == 0
    g = _gen(4)
    spec, nans = _from_bits32(CAST_SPECIALS), _from_bits32(CAST_NANS)
    srcs = []
    for k, n in enumerate(CAST_SIZES):
        # random values over many binades, random bit patterns in every third tensor
        t = torch.randn(n, generator=g) * torch.exp(8.0 * torch.randn(n, generator=g))
        if k % 3 == 2 and n:
            bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
            t = bits.view(torch.float32)
        if n >= len(spec) + len(nans):  # at the start and across the end of the larger tensors
            t[:len(spec)] = spec
            t[n - len(nans):] = nans
        srcs.append(t.contiguous())
    srcs[1] = nans[:1].clone()  # the one-element tensor: 0x7f800001
    dsts = [torch.full((n,), -1.0, dtype=torch.bfloat16, device=DEV) for n in CAST_SIZES]
    vf._cast_multi([s.to(DEV) for s in srcs], dsts, 0, 1, DEV)
    torch.cuda.synchronize()
    n_nan = 0
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        got = _u16(d)
        isnan = torch.isnan(s).numpy()
        n_nan += int(isnan.sum())
        want = _u16(s.to(torch.bfloat16))
        assert np.array_equal(got[~isnan], want[~isnan]), f"tensor {k} (n = {s.numel()})"
        # torch's CPU cast turns a NaN into 0xffff inside a vectorised block and into 0x7fc0 in
        # a scalar tail, so it is no reference for one: the default NaN must keep its bits
        default_nan = _u32(s) == 0x7fc00000
        assert (got[default_nan] == 0x7fc0).all(), f"tensor {k}: the default NaN"
        nan_out = (got & 0x7fff) > 0x7f80
        bad = isnan & ~nan_out
        assert not bad.any(), (f"tensor {k}: NaN inputs {[hex(v) for v in _u32(s)[bad][:4]]} became "
                               f"{[hex(v) for v in got[bad][:4]]}")
    assert n_nan >= 3 * len(CAST_NANS)


def test_cast_multi_bf16_to_f32_bit_exact():
    from ocm import vae_fused as vf

    g = _gen(5)
    srcs = []
    for n in CAST_SIZES:
        bits = torch.randint(0, 2 ** 16, (n,), generator=g, dtype=torch.int64)
        srcs.append((bits - (bits >= 2 ** 15) * 2 ** 16).to(torch.int16).view(torch.bfloat16))
    every = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)  # NaNs included
    srcs[5][:every.numel()] = every
    dsts = [torch.full((n,), -1.0, dtype=torch.float32, device=DEV) for n in CAST_SIZES]
    vf._cast_multi([s.to(DEV) for s in srcs], dsts, 1, 0, DEV)
    torch.cuda.synchronize()
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        assert np.array_equal(_u32(d), _u16(s).astype(np.uint32) << 16), f"tensor {k}"


def test_cast_multi_rejects_33_tensors():
    from ocm import vae_fused as vf

    srcs = [torch.ones(4, device=DEV) for _ in range(33)]
    dsts = [torch.full((4,), -1.0, dtype=torch.bfloat16, device=DEV) for _ in range(33)]
    with pytest.raises(ValueError):
        vf._cast_multi(srcs, dsts, 0, 1, DEV)
    torch.cuda.synchronize()
    assert all(bool((d == -1.0).all()) for d in dsts)


# ---------------------------------------------------------------------------
# 5. act_bias_bwd
# ---------------------------------------------------------------------------
ACT_SHAPES = [(1, 8), (255, 24), (513, 40), (1030, 6144)]


def _act_bias_bwd(act, g, y):
    """ocm_vae_act_bias_bwd on device tensors: (gy, gb); act 0 through _bias_grad."""
    from ocm import _lib
    from ocm import vae_fused as vf

    if not act:
        return None, vf._bias_grad(g)
    B, N = g.shape
    gy = torch.full_like(g, -1.0)
    gb = torch.full((N,), -1.0, dtype=g.dtype, device=g.device)
    _lib.check(_lib.load().ocm_vae_act_bias_bwd(vf._h(g.device), 1, g.data_ptr(), y.data_ptr(), B, N, gy.data_ptr(),
                                                gb.data_ptr(), _lib.stream_handle(g.device)), "ocm_vae_act_bias_bwd")
    return gy, gb


@pytest.mark.parametrize("act", [0, 1], ids=["none", "elu"])
@pytest.mark.parametrize("B,N", ACT_SHAPES)
def test_act_bias_bwd_matches_float64(B, N, act):
    """gy = g·elu'(y) (autograd of torch's ELU in float64 on the bf16 values) rounded to
    bf16, and the bias gradient: the column sums of the rounded gy, rounded to bf16."""
    g0 = _gen(5000 + B + N)
    g = torch.randn(B, N, generator=g0).to(torch.bfloat16)
    y = (2.0 * torch.randn(B, N, generator=g0)).to(torch.bfloat16)
    y[0, :3] = torch.tensor([0.0, -0.0, -90.0]).to(torch.bfloat16)
    gy, gb = _act_bias_bwd(act, g.to(DEV), y.to(DEV))
    tag = f"act_bias_bwd ({B}, {N}) act {act}"
    if act:
        y64 = y.double().requires_grad_(True)
        (ref,) = torch.autograd.grad(torch.nn.functional.elu(y64), y64, g.double())
        _assert_rounds_to_bf16(gy, ref.numpy(), tag + " gy")
        rows = gy.cpu().double().numpy()
    else:
        rows = g.double().numpy()
    # Σ_rows in float32 (any order): ≤ B·2⁻²⁴·Σ|gy| from the exact sum, then one bf16 rounding
    s, sa = rows.sum(0), np.abs(rows).sum(0)
    facc = B * 2.0 ** -24 * sa
    bound = _bf16_half_ulp(np.abs(s) + facc) + facc
    err = np.abs(gb.cpu().double().numpy() - s)
    print(f"{tag} bias: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), tag


# ---------------------------------------------------------------------------
# 6. Adam
# ---------------------------------------------------------------------------
def _adam_reference_step(P, M, V, Mmag, Vmag, G, t, lr, b1, b2, eps, wd):
    """torch.optim.Adam's step in float64 NumPy: L2 weight decay folded into the
    gradient, bias corrections from the Python-double betas.  The moment updates use
    the float32 β and weight decay the kernel reads, widened.  ``t`` is the optimizer's
    step count (FusedAdam keeps one counter for all parameters).  Mmag and Vmag are the
    same recurrences over the magnitude |g| + wd·|p| of the gradient's terms: g + wd·p
    and the sum of exp_avg can cancel, their float32 rounding errors do not."""
    b1k, b2k, wdk = (float(np.float32(v)) for v in (b1, b2, wd))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for i, g in enumerate(G):
        if g is None:
            continue
        gmag = np.abs(g) + wdk * np.abs(P[i])
        g = g + wdk * P[i] if wd != 0 else g
        M[i] = b1k * M[i] + (1.0 - b1k) * g
        Mmag[i] = b1k * Mmag[i] + (1.0 - b1k) * gmag
        V[i] = b2k * V[i] + (1.0 - b2k) * g * g
        Vmag[i] = b2k * Vmag[i] + (1.0 - b2k) * gmag * gmag
        P[i] = P[i] - (lr / bc1) * M[i] / (np.sqrt(V[i]) / np.sqrt(bc2) + eps)


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


ADAM_CYCLE = [1, 3, 255, 256, 257, 1025]


@pytest.mark.parametrize("wd", [1e-3, 0.0])
@pytest.mark.parametrize("table", ["256_tensors", "one_long_tensor"])
def test_fused_adam_matches_float64_adam(table, wd):
    """ocm_adam_step through FusedAdam, three steps: 256 tensors whose boundaries fall
    inside a thread's four strided elements (one of them without a gradient on step 2),
    and one tensor of 4096·1024 + 5 elements (the grid-stride loop's second lap)."""
    from ocm import vae_fused as vf

    sizes = [ADAM_CYCLE[k % 6] for k in range(256)] if table == "256_tensors" else [4096 * 1024 + 5]
    skip = 7 if table == "256_tensors" else None
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    g = _gen(6000 + len(sizes))
    p0 = [torch.randn(n, generator=g) for n in sizes]
    params = [p.clone().to(DEV).requires_grad_(True) for p in p0]
    opt = vf.FusedAdam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    P = [p.double().numpy().copy() for p in p0]
    M, V, Mmag, Vmag = ([np.zeros(n) for n in sizes] for _ in range(4))
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in (1, 2, 3):
        grads = [torch.randn(n, generator=g) for n in sizes]
        G = [gr.double().numpy() for gr in grads]
        if t == 2 and skip is not None:
            G[skip] = None
        for k, (p, gr) in enumerate(zip(params, grads)):
            p.grad = None if G[k] is None else gr.to(DEV)
        if t == 2 and skip is not None:
            before = [x.clone() for x in (params[skip].detach(), opt.exp_avg[skip], opt.exp_avg_sq[skip])]
        opt.step()
        _adam_reference_step(P, M, V, Mmag, Vmag, G, t, lr, b1, b2, eps, wd)
        if t == 2 and skip is not None:  # skipped: parameter and moments untouched
            after = (params[skip].detach(), opt.exp_avg[skip], opt.exp_avg_sq[skip])
            assert all(torch.equal(a, b) for a, b in zip(before, after))
        assert float(opt.step_t) == t
        for k in range(len(sizes)):
            pk = params[k].detach().cpu().double().numpy()
            mk, vk = opt.exp_avg[k].cpu().double().numpy(), opt.exp_avg_sq[k].cpu().double().numpy()
            ep = np.abs(pk - P[k]) / (ADAM_P_REL_LR * lr + ADAM_P_ULPS * _ulp32(P[k]))
            # the moments: ulps of their terms' magnitude (_adam_reference_step), which is the
            # value itself for exp_avg_sq without weight decay
            em = np.abs(mk - M[k]) / (ADAM_M_ULPS * _ulp32(Mmag[k]))
            ev = np.abs(vk - V[k]) / (ADAM_M_ULPS * _ulp32(Vmag[k]))
            worst = dict(p=max(worst["p"], float(ep.max())), m=max(worst["m"], float(em.max())),
                         v=max(worst["v"], float(ev.max())))
            assert (ep <= 1).all(), (t, k, "param")
            assert (em <= 1).all(), (t, k, "exp_avg")
            assert (ev <= 1).all(), (t, k, "exp_avg_sq")
    print(f"adam {table} wd {wd}: worst err / bound: param {worst['p']:.3f}, exp_avg {worst['m']:.3f}, "
          f"exp_avg_sq {worst['v']:.3f}")


def test_fused_adam_rejects_257_tensors():
    from ocm import vae_fused as vf

    params = [torch.ones(3, device=DEV, requires_grad=True) for _ in range(257)]
    for p in params:
        p.grad = torch.ones_like(p)
    opt = vf.FusedAdam(params, lr=1e-2)
    with pytest.raises(ValueError):
        opt.step()
    torch.cuda.synchronize()
    assert all(bool((p == 1.0).all()) for p in params) and float(opt.step_t) == 0.0


# ---------------------------------------------------------------------------
# 7. chan_sum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16_autocast"])
@pytest.mark.parametrize("idx", [3, 4, 8])
def test_chan_sum_bias_gradient(monkeypatch, idx, bf16):
    """ConvTranspose1d's bias gradient through ocm_conv1d_wgrad + ocm_chan_sum
    (ocm.conv.QSUM_FUSED = False) against the fp64 host gradient at
    tests/test_gpu_conv.py's tolerances, and against the fused launch's result."""
    import ocm.conv
    from test_gpu_conv import SHAPES, _mods

    transposed, I, O, K, s, pad, op, L = SHAPES[idx]
    assert transposed
    B = 4 if bf16 else 6
    g = _gen(7000 + idx)
    x = torch.randn(B, I, L, generator=g)
    x = x.bfloat16() if bf16 else x
    got, gy = {}, None
    for fused in (False, True):
        monkeypatch.setattr(ocm.conv, "QSUM_FUSED", fused)
        fast, ref = _mods(transposed, I, O, K, s, pad, op)
        xd = x.to(DEV).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = fast(xd)
        if gy is None:
            gy = torch.randn(y.shape, generator=g)
            gy = gy.bfloat16() if bf16 else gy
        y.backward(gy.to(DEV))
        got[fused] = fast.bias.grad.cpu().numpy().astype(np.float64)
    xr = x.double().requires_grad_(True)
    ref(xr).backward(gy.double())
    want = ref.bias.grad.numpy()
    atol = 1e-5 * np.abs(want).max()
    err = np.abs(got[False] - want) / (atol + 1e-4 * np.abs(want))
    print(f"chan_sum SHAPES[{idx}] {'bf16' if bf16 else 'f32'}: max err / tolerance = {float(err.max()):.3e}")
    np.testing.assert_allclose(got[False], want, rtol=1e-4, atol=atol)
    np.testing.assert_allclose(got[False], got[True], rtol=1e-4, atol=atol)
