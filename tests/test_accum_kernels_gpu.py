"""The gradient-accumulation kernels alone (csrc/accum.hip): vqa_grad_accumulate against torch's
fp32 adds bit for bit in guarded buffers, its refusals, and the device-counter protocol of
vqa_accum_advance / vqa_accum_finish over k = 3 micro-batches."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 64                                    # canary floats before and after every guarded array
CANARY = 0x5CA1AB1E


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L = pkg.lib
    L.load()
    from __graft_entry__ import ROOT
    inv = int(re.search(r"#define VQA_ERR_INVALID (\d+)",
                        open(os.path.join(ROOT, "include", "vqa_hip.h")).read()).group(1))
    return torch, L, inv


def _rc(L, name, *args):
    return getattr(L.load(), name)(*args, L.stream_handle())


def _guarded(torch, values):
    """values (fp32 cpu tensor) between two canary pads on the device; (whole buffer, the view)."""
    n = values.numel()
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.int32, device="cuda")
    view = buf[PAD:PAD + n].view(torch.float32)
    view.copy_(values)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _pads_intact(buf, n):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all())


def _values(torch, n, seed):
    """Normal values with the special ones spread through them: +-0, denormals, +-inf, NaN."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3.0
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, float("inf"), float("-inf"), float("nan"),
                            3.4e38, -3.4e38, 1.1754944e-38])
    pos = torch.randperm(n, generator=g)[:min(n, 3 * special.numel())]
    x[pos] = special.repeat(3)[:pos.numel()]
    return x


@pytest.mark.parametrize("n", [4, 8, 1020, 1024, 4100, (1 << 20) + 4, (1 << 23) + 1028])
def test_accumulate_bitwise(env, n):
    """acc = g0; acc += g1; acc += g2 in fp32: below, at and across a block (1024 floats), many
    blocks plus one float4 (2^20 + 4), and past the capped grid (2048 blocks x 1024 floats = 2^21
    per sweep): 2^23 + 1028 floats take the four-deep unrolled sweep once and the tail loop."""
    torch, L, _ = env
    gs = [_values(torch, n, 10 * n + j) for j in range(3)]
    want = gs[0].cuda().clone()
    want += gs[1].cuda()
    want += gs[2].cuda()
    abuf, acc = _guarded(torch, torch.full((n,), 123.0))     # dirty: micro == 0 must overwrite it
    micro = torch.zeros(1, dtype=torch.int32, device="cuda")
    for j, g in enumerate(gs):
        gbuf, gv = _guarded(torch, g)
        before = gbuf.clone()
        micro.fill_(j)
        assert _rc(L, "vqa_grad_accumulate", acc.data_ptr(), gv.data_ptr(), n, micro.data_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.equal(gbuf, before), "g (or its guards) was written"
        assert int(micro.item()) == j, "the accumulate wrote the counter"
    assert _pads_intact(abuf, n)
    assert torch.equal(torch.isnan(acc), torch.isnan(want))
    ok = torch.isnan(want) | (acc.view(torch.int32) == want.view(torch.int32))
    assert bool(ok.all()), f"{int((~ok).sum())} of {n} elements differ from torch's fp32 sums"
    assert torch.allclose(acc, want, rtol=0, atol=0, equal_nan=True)


def test_accumulate_refusals(env):
    torch, L, inv = env
    abuf, acc = _guarded(torch, torch.full((16,), 7.0))
    gbuf, g = _guarded(torch, torch.full((16,), 1.0))
    a0, g0 = abuf.clone(), gbuf.clone()
    micro = torch.ones(1, dtype=torch.int32, device="cuda")
    cases = [(acc.data_ptr(), g.data_ptr(), 0), (acc.data_ptr(), g.data_ptr(), 6), (acc.data_ptr(), g.data_ptr(), -4),
             (acc.data_ptr() + 4, g.data_ptr(), 8), (acc.data_ptr(), g.data_ptr() + 4, 8)]
    for a, b, n in cases:
        assert _rc(L, "vqa_grad_accumulate", a, b, n, micro.data_ptr()) == inv, (a % 16, b % 16, n)
    torch.cuda.synchronize()
    assert torch.equal(abuf, a0) and torch.equal(gbuf, g0), "a refused call wrote something"


def test_counter_protocol(env):
    """micro 0 -> 1 -> 2 -> 3, the finish resets it; LOSS = float((double(l0) + l1 + l2) / 3);
    the log-prob rows land at j x B; a second round from a dirty loss sum gives the same."""
    torch, L, _ = env
    k, B, A = 3, 4, 170
    state = torch.zeros(4, dtype=torch.int32, device="cuda")             # {double loss sum, int32 micro}
    loss_sum, micro = state.data_ptr(), state.data_ptr() + 8
    lbuf, logp_all = _guarded(torch, torch.zeros(k * B * A))
    loss = torch.zeros(1, device="cuda")
    losses = [np.float32(1.2345678), np.float32(0.3333333), np.float32(5.4321e-3)]
    want = np.float32((np.float64(losses[0]) + np.float64(losses[1]) + np.float64(losses[2])) / 3.0)
    rows = [torch.randn(B, A, generator=torch.Generator().manual_seed(j)).cuda() for j in range(k)]
    for rnd in range(2):
        logp_all.zero_()
        for j in range(k):
            assert int(state[2].item()) == j
            loss.fill_(float(losses[j]))
            assert _rc(L, "vqa_accum_advance", rows[j].data_ptr(), logp_all.data_ptr(), B, A, k, loss.data_ptr(),
                       loss_sum, micro) == 0
        assert int(state[2].item()) == k
        # a launch past the k-th writes nothing (the counter is outside [0, k))
        assert _rc(L, "vqa_accum_advance", rows[0].data_ptr(), logp_all.data_ptr(), B, A, k, loss.data_ptr(),
                   loss_sum, micro) == 0
        assert int(state[2].item()) == k
        assert _rc(L, "vqa_accum_finish", loss.data_ptr(), loss_sum, micro, k) == 0
        torch.cuda.synchronize()
        assert int(state[2].item()) == 0
        assert np.float32(loss.item()).tobytes() == want.tobytes(), (loss.item(), want)
        got = logp_all.view(k, B, A)
        for j in range(k):
            assert torch.equal(got[j], rows[j]), f"micro-batch {j}'s rows are not at {j} x B"
        assert _pads_intact(lbuf, k * B * A)
        # the loss sum stays dirty for the second round: micro == 0 restarts it
        assert state[:2].view(torch.float64).item() != 0.0
