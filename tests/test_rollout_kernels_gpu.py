"""vqa_attn_headmean and vqa_rollout_cls (csrc/rollout.hip) against fp64 torch on the same
bf16 q | k.  The inputs are unscaled randn rounded to bf16: unit-variance logits, so the maps
are peaked and differ by layer, and a wrong formula moves the mask by >= 8e-3 of its maximum
(reversed layer order 8e-2, no identity 6e-2, one head instead of the mean 2e-1, a mean over
16 instead of 12 heads 8e-3), while torch fp32 sits at 1e-6 from fp64.

Measured on an MI355X (profiles/vit_rollout_parity.json): vqa_attn_headmean 2.6e-7 max abs at
197 tokens; the chain, relative to the mask's maximum, 2.5e-7 (torch fp32: 8.9e-7) at 12 x 197
and 1.0e-7 (3.1e-7) at 3 x 37; both kernels end to end 4.0e-7 (vqa_attn_probs + torch fp32:
1.1e-6) and 2.6e-7 (3.4e-7)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
FILL = -7.0                                               # pre-fill of the output: pad columns keep it
# (B, n, H, dh, layers): a ragged last query block and key tile at ViT's 197 tokens, more than one
# image, fewer tokens than one tile
SHAPES = ((2, 197, 12, 64, 12), (3, 37, 12, 64, 3), (1, 5, 8, 96, 1))


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ld(n):
    return 200 if n == 197 else 40


def _headmean(pkg, qk, aug, B, n, H, dh):
    """One vqa_attn_headmean launch per layer of qk [layers, B*n, 2*H*dh] into aug [layers, B, n, ld]."""
    L_ = pkg.lib
    D = H * dh
    for i in range(qk.shape[0]):
        d = L_.AttnDesc()
        d.q, d.ldq, d.k, d.ldk = qk[i].data_ptr(), 2 * D, qk[i].data_ptr() + 2 * D, 2 * D
        d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = B, H, n, n, dh, dh ** -0.5
        L_.check(L_.load().vqa_attn_headmean(ctypes.byref(d), aug[i].data_ptr(), aug.shape[-1], L_.stream_handle()),
                 "vqa_attn_headmean")


def _probs64(qk, B, n, H, dh):
    """fp64 softmax(q k^T scale) of the same bf16 values: [layers, B, H, n, n]."""
    x = qk.double().view(qk.shape[0], B, n, 2, H, dh)
    q, k = x[:, :, :, 0].transpose(2, 3), x[:, :, :, 1].transpose(2, 3)
    return torch.softmax(q @ k.transpose(3, 4) * dh ** -0.5, -1)


def _aug(p):
    """(mean over heads + I) / rowsum of [..., H, n, n] maps, in their dtype."""
    n = p.shape[-1]
    a = p.mean(-3) + torch.eye(n, dtype=p.dtype, device=p.device)
    return a / a.sum(-1, keepdim=True)


def _chain(a):
    """The script's chain J_0 = A_0, J_l = A_l J_{l-1} over a [layers, B, n, n]: J_last[:, 0, 1:]."""
    j = a[0]
    for l in range(1, a.shape[0]):
        j = a[l] @ j
    return j[:, 0, 1:]


def _rel(x, ref):
    """Max error relative to each image's mask maximum."""
    return float(((x.double() - ref).abs().amax(1) / ref.amax(1)).max())


def _rollout(pkg, aug, n, unit=True):
    L_ = pkg.lib
    layers, B, _, ld = aug.shape
    mask = torch.full((B, n - 1), FILL, device="cuda")
    mu = torch.full((B, n - 1), FILL, device="cuda") if unit else None
    L_.call("vqa_rollout_cls", aug.data_ptr(), layers, B, n, ld, B * n * ld, mask.data_ptr(),
            mu.data_ptr() if unit else None)
    torch.cuda.synchronize()
    return mask, mu


@pytest.fixture(scope="module")
def maps(cuda, pkg):
    """Per shape: the bf16 q | k of every layer, the kernel's maps (computed once, left unchanged)
    and the fp64 per-head probabilities."""
    out = {}
    for B, n, H, dh, layers in SHAPES:
        g = torch.Generator().manual_seed(1000 + n)
        qk = torch.randn(layers, B * n, 2 * H * dh, generator=g).to(torch.bfloat16).cuda()
        aug = torch.full((layers, B, n, _ld(n)), FILL, device="cuda")
        _headmean(pkg, qk, aug, B, n, H, dh)
        torch.cuda.synchronize()
        out[n] = (qk, aug, _probs64(qk, B, n, H, dh))
    return out


@pytest.mark.parametrize("B,n,H,dh,layers", SHAPES)
def test_headmean_matches_fp64(cuda, pkg, maps, parity_report, B, n, H, dh, layers):
    qk, aug, p64 = maps[n]
    ref = _aug(p64)
    got = aug[..., :n]
    err = float((got.double() - ref).abs().max())
    rows = float((got.sum(-1) - 1).abs().max())
    print(f"headmean {B}x{n}x{H}x{dh}: max abs {err:.3e}, row sums off by {rows:.3e}")
    parity_report.setdefault("attn_headmean_max_abs", {})[f"{B}x{n}x{H}x{dh}"] = err
    # the bound test_attention_probs_match_torch pins for this softmax on such inputs; the mean
    # over the heads and the halving by the row sum (= 2) can only shrink it
    assert err <= 2e-6, err
    assert rows <= 1e-5, rows
    assert bool((aug[..., n:] == FILL).all())               # pad columns untouched
    again = torch.full_like(aug, FILL)
    _headmean(pkg, qk, again, B, n, H, dh)
    torch.cuda.synchronize()
    assert torch.equal(aug.view(torch.int32), again.view(torch.int32))


def test_headmean_refuses_bad_arguments(cuda, pkg):
    L_ = pkg.lib
    qk = torch.zeros(64, 2 * 768, dtype=torch.bfloat16, device="cuda")
    aug = torch.zeros(1, 64, 64, device="cuda")

    def rc(ld=64, lk=64, dh=64, q_off=0):
        d = L_.AttnDesc()
        d.q, d.ldq, d.k, d.ldk = qk.data_ptr() + q_off, 1536, qk.data_ptr() + 1536, 1536
        d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = 1, 12, 64, lk, dh, 0.125
        return L_.load().vqa_attn_headmean(ctypes.byref(d), aug.data_ptr(), ld, L_.stream_handle())
    assert rc() == 0
    for kw in (dict(ld=62), dict(ld=60), dict(lk=32), dict(dh=128), dict(q_off=2)):
        assert rc(**kw) != 0, kw
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [197, 37])
def test_rollout_chain_matches_fp64(cuda, pkg, maps, parity_report, n):
    """The chain alone: the reference is the fp64 chain of the SAME maps, so only the fp32
    summation differs.  Bound: 4 x the error of the same chain done by torch in fp32 on the
    device (a different but equally long summation order: both are fp32 sums of n non-negative
    terms, once per layer)."""
    _, aug, _ = maps[n]
    a32 = aug[..., :n].contiguous()
    ref = _chain(a32.double())
    e_ref = _rel(_chain(a32), ref)
    mask, unit = _rollout(pkg, aug, n)
    err = _rel(mask, ref)
    print(f"rollout chain n={n}: kernel {err:.3e}, torch fp32 {e_ref:.3e}")
    parity_report.setdefault("rollout_chain_rel", {})[f"n{n}"] = {"kernel": err, "torch_fp32": e_ref}
    assert err <= 4 * e_ref, (err, e_ref)
    want = mask / mask.amax(1, keepdim=True)
    assert torch.equal(unit.view(torch.int32), want.view(torch.int32))
    assert float(unit.amax(1).min()) == 1.0 == float(unit.amax(1).max())
    mask2, unit2 = _rollout(pkg, aug, n)
    assert torch.equal(mask.view(torch.int32), mask2.view(torch.int32))
    assert torch.equal(unit.view(torch.int32), unit2.view(torch.int32))
    only, none = _rollout(pkg, aug, n, unit=False)          # mask_unit is optional
    assert none is None and torch.equal(only, mask)


@pytest.mark.parametrize("n", [197, 37])
def test_rollout_end_to_end_matches_fp64(cuda, pkg, maps, parity_report, n):
    """Both kernels against the fp64 rollout of the fp64 softmax; the baseline under the same
    4 x rule is the existing path: vqa_attn_probs per layer, then the rollout by torch in fp32."""
    L_ = pkg.lib
    B, _, H, dh, layers = next(s for s in SHAPES if s[1] == n)
    qk, aug, p64 = maps[n]
    ref = _chain(_aug(p64))
    mask, _ = _rollout(pkg, aug, n)
    p32 = torch.empty(layers, B, H, n, n, device="cuda")
    D = H * dh
    for i in range(layers):
        d = L_.AttnDesc()
        d.q, d.ldq, d.k, d.ldk = qk[i].data_ptr(), 2 * D, qk[i].data_ptr() + 2 * D, 2 * D
        d.p = p32[i].data_ptr()
        d.batch, d.heads, d.lq, d.lk, d.dh, d.scale = B, H, n, n, dh, dh ** -0.5
        L_.check(L_.load().vqa_attn_probs(ctypes.byref(d), L_.stream_handle()), "vqa_attn_probs")
    torch.cuda.synchronize()
    e_ref = _rel(_chain(_aug(p32)), ref)
    err = _rel(mask, ref)
    print(f"rollout end to end n={n}: kernels {err:.3e}, vqa_attn_probs + torch fp32 {e_ref:.3e}")
    parity_report.setdefault("rollout_end_to_end_rel", {})[f"n{n}"] = {"kernels": err, "probs_torch_fp32": e_ref}
    assert err <= 4 * e_ref, (err, e_ref)
