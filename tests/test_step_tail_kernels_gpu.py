"""The step-tail exports of ABI 21 against the calls they specialise, bit for bit:
vqa_embedding_sort + vqa_embedding_bwd_sorted == vqa_embedding_bwd; vqa_grad_sqnorm_final ==
vqa_grad_sqnorm x2 + vqa_optim_finalize (dense, and with the table rows known untouched not
loaded); vqa_copy_multi == one copy per segment."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def k(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    return pkg


def run(pkg, name, *args):
    pkg.ops.Call(name, *[pkg.ops.addr(a) if isinstance(a, torch.Tensor) else a for a in args])(
        pkg.lib.stream_handle())


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g) * scale


def bits(t):
    return t.contiguous().view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ the embedding scatter's two halves
@pytest.mark.parametrize("ids_kind", ["equal", "distinct", "repeats"])
@pytest.mark.parametrize("T", [1, 33, 2048])
def test_sort_then_sorted_scatter_equals_embedding_bwd(k, T, ids_kind):
    """`distinct`: every id differs while the vocabulary allows it (T <= 97), else each id of the
    vocabulary in turn -- 2048 tokens cannot differ in a vocabulary of 97."""
    V, D = 97, 256
    if ids_kind == "equal":
        ids = torch.full((T,), 5, device="cuda", dtype=torch.int64)
    elif ids_kind == "distinct":
        ids = (torch.arange(T, device="cuda", dtype=torch.int64) * 7) % V
    else:
        g = torch.Generator(device="cuda").manual_seed(T)
        ids = torch.randint(0, V, (T,), device="cuda", generator=g)
        ids[: T // 3] = 11
    dh = rnd((T, D), 40 + T)
    ws1 = torch.full((3 * T,), -7, device="cuda", dtype=torch.int32)
    ws2 = torch.full((3 * T,), -9, device="cuda", dtype=torch.int32)
    base = rnd((V, D), 41)                                   # the scatter ADDS into the rows
    one, two = base.clone(), base.clone()
    run(k, "vqa_embedding_bwd", ids, dh, one, T, D, V, ws1)
    run(k, "vqa_embedding_sort", ids, T, V, ws2)
    junk = rnd((V, D), 42)                                   # unrelated work between the halves
    junk.mul_(2.0)
    run(k, "vqa_embedding_bwd_sorted", dh, two, T, D, V, ws2)
    torch.cuda.synchronize()
    assert same_bits(one, two)
    assert not same_bits(one, base)
    assert torch.equal(ws1[: 2 * T], ws2[: 2 * T])           # positions and ids (run ends: at run starts only)


def test_split_exports_refuse_more_than_one_slice(k):
    lib = k.lib.load()
    ws = torch.zeros(8, device="cuda", dtype=torch.int32)
    ids = torch.zeros(8, device="cuda", dtype=torch.int64)
    s = k.lib.stream_handle()
    assert lib.vqa_embedding_sort(ctypes.c_void_p(ids.data_ptr()), 16385, 97, ctypes.c_void_p(ws.data_ptr()), s) == 1000
    assert lib.vqa_embedding_sort(ctypes.c_void_p(ids.data_ptr()), 0, 97, ctypes.c_void_p(ws.data_ptr()), s) == 1000


# ------------------------------------------------------------------ the fused last squared-norm + finalize
FIN = (1.0, 1.0, 2, 10, 0.9, 0.999)                         # grad_scale, max_norm, warmup, total, betas


def _state(step=3.0):
    st = torch.zeros(16, device="cuda")
    st[0] = step
    return st


def _three_calls(k, pre, g0, g1, ws, K, st):
    run(k, "vqa_grad_sqnorm", pre, pre.numel(), ws, K)
    run(k, "vqa_grad_sqnorm", g0, g0.numel(), k.ops.addr(ws, K), K)
    run(k, "vqa_grad_sqnorm", g1, g1.numel(), k.ops.addr(ws, 2 * K), K)
    run(k, "vqa_optim_finalize", ws, 3 * K, *FIN, st)


def _fused(k, pre, g0, g1, ws, K, st, cnt, mark=None, lead=0, cols=0):
    run(k, "vqa_grad_sqnorm", pre, pre.numel(), ws, K)
    run(k, "vqa_grad_sqnorm_final", g0, g0.numel(), g1, g1.numel(), ws, K, 3 * K, mark, lead, cols, cnt, *FIN, st)


@pytest.mark.parametrize("case", ["below", "above", "inf"])
@pytest.mark.parametrize("K", [1, 3, 1024])
@pytest.mark.parametrize("big", [False, True])
def test_sqnorm_final_equals_sqnorm_sqnorm_finalize(k, big, K, case):
    """n = 4 and n = 4 (256 K + 1) per range; a clip norm below and above max_norm = 1 and one
    inf gradient; partials of an earlier launch in the first K slots.  Run twice on the same
    workspace and counter: the second run starts from the counter the first left."""
    n = 4 * (256 * K + 1) if big else 4
    scale = {"below": 1e-3 / (n ** 0.5), "above": 10.0, "inf": 1.0}[case]
    g = rnd(3 * n, 50 + K, scale)
    if case == "inf":
        g[n + n // 2] = float("inf")
    pre, g0, g1 = g[:n], g[n:2 * n], g[2 * n:]
    ws_a = torch.full((3 * K,), NAN, device="cuda", dtype=torch.float64)
    ws_b = ws_a.clone()
    st_a, st_b = _state(), _state()
    cnt = torch.zeros(k.lib.SQNORM_FINAL_COUNTER_WORDS, device="cuda", dtype=torch.int32)
    for rep in range(2):
        _three_calls(k, pre, g0, g1, ws_a, K, st_a)
        _fused(k, pre, g0, g1, ws_b, K, st_b, cnt)
        torch.cuda.synchronize()
        assert same_bits(ws_a, ws_b), rep
        assert same_bits(st_a, st_b), (rep, st_a.tolist(), st_b.tolist())
        assert not bool(cnt.any()), rep
        assert float(st_b[0]) == 4.0 + rep and float(st_b[8]) == 1.0
        g.mul_(0.5)                                          # other partials in the second run
        g0, g1 = g[n:2 * n], g[2 * n:]
    coef = float(st_b[2])
    assert {"below": coef == 1.0, "above": 0.0 < coef < 1.0, "inf": coef == 0.0}[case], coef


@pytest.mark.parametrize("touched", ["none", "all", "first", "last", "repeats"])
def test_sqnorm_final_skips_unmarked_rows_with_the_same_partials(k, touched):
    """37 rows x 256 behind 8 densely read floats; rows not marked with the step counter hold
    exact zeros and are not loaded: every partial equals the dense kernel's.  Stale marks of
    another step count as untouched."""
    R, C, lead, K = 37, 256, 8, 3
    ids = {"none": [], "all": list(range(R)), "first": [0], "last": [36], "repeats": [3, 3, 17, 3, 36, 17]}[touched]
    st_a, st_b = _state(5.0), _state(5.0)
    mark = torch.full((R,), -1, device="cuda", dtype=torch.int32)
    mark[::2] = 4                                            # an earlier step's marks
    if ids:
        idt = torch.tensor(ids, device="cuda", dtype=torch.int64)
        run(k, "vqa_embed_mark", idt, len(ids), R, mark, st_b)
    g1 = torch.zeros(lead + R * C, device="cuda")
    g1[:lead] = rnd(lead, 60)
    rows = g1[lead:].view(R, C)
    for r in set(ids):
        rows[r] = rnd(C, 61 + r)
    pre, g0 = rnd(16, 62), rnd(4 * 300, 63)
    ws_a = torch.full((3 * K,), NAN, device="cuda", dtype=torch.float64)
    ws_b = ws_a.clone()
    cnt = torch.zeros(k.lib.SQNORM_FINAL_COUNTER_WORDS, device="cuda", dtype=torch.int32)
    _three_calls(k, pre, g0, g1, ws_a, K, st_a)
    _fused(k, pre, g0, g1, ws_b, K, st_b, cnt, mark=mark, lead=lead, cols=C)
    torch.cuda.synchronize()
    assert same_bits(ws_a, ws_b)
    assert same_bits(st_a, st_b)
    assert not bool(cnt.any())
    # the rows really are skipped: poison an unmarked row -- the dense sum sees it, this one does not
    free = [r for r in range(R) if r not in ids]
    if free:
        rows[free[-1]] = 1e6
        st_c = _state(5.0)
        ws_c = ws_a.clone()
        _fused(k, pre, g0, g1, ws_c, K, st_c, cnt, mark=mark, lead=lead, cols=C)
        torch.cuda.synchronize()
        assert same_bits(ws_c, ws_b)


def test_sqnorm_final_refuses_bad_ranges(k):
    lib, P = k.lib.load(), ctypes.c_void_p
    g = torch.zeros(64, device="cuda")
    ws = torch.zeros(8, device="cuda", dtype=torch.float64)
    cnt = torch.zeros(k.lib.SQNORM_FINAL_COUNTER_WORDS, device="cuda", dtype=torch.int32)
    st, mark = _state(), torch.zeros(4, device="cuda", dtype=torch.int32)
    f = (ctypes.c_float(1.0), ctypes.c_float(1.0), 2, 10, ctypes.c_float(0.9), ctypes.c_float(0.999))

    def rc(n0, n1, parts, fin, mk, lead, cols):
        return lib.vqa_grad_sqnorm_final(P(g.data_ptr()), n0, P(g.data_ptr()), n1, P(ws.data_ptr()), parts, fin,
                                         P(mk.data_ptr()) if mk is not None else None, lead, cols,
                                         P(cnt.data_ptr()), *f, P(st.data_ptr()), k.lib.stream_handle())
    assert rc(6, 8, 2, 4, None, 0, 0) == 1000                # n % 4
    assert rc(8, 8, 2, 3, None, 0, 0) == 1000                # fin_parts < 2 parts
    assert rc(8, 40, 2, 4, mark, 8, 12) == 1000              # 32 floats are not whole rows of 12
    assert rc(8, 40, 2, 4, mark, 8, 8) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ several copies in one launch
def test_copy_multi_eight_segments(k):
    sizes = [0, 16, 48, 4096, 16 * 257, (1 << 20) + 16, 16 * (256 * 4096 + 3), 256]
    pad = 4                                                  # int32 guard words on both sides
    srcs = [torch.randint(-2 ** 31, 2 ** 31 - 1, (s // 4,), device="cuda", dtype=torch.int32) for s in sizes]
    dsts = [torch.full((s // 4 + 2 * pad,), 0x5A5A5A5A, device="cuda", dtype=torch.int32) for s in sizes]
    jobs = (k.lib.CopyJob * 8)(*[k.lib.CopyJob(d.data_ptr() + 4 * pad, s.data_ptr(), n)
                                 for d, s, n in zip(dsts, srcs, sizes)])
    k.lib.call("vqa_copy_multi", jobs, 8)
    torch.cuda.synchronize()
    for d, s, n in zip(dsts, srcs, sizes):
        assert torch.equal(d[pad:pad + n // 4], s), n
        assert bool((d[:pad] == 0x5A5A5A5A).all()) and bool((d[pad + n // 4:] == 0x5A5A5A5A).all()), n


def test_copy_multi_refuses_misaligned_and_too_many(k):
    lib = k.lib.load()
    a, b = torch.zeros(64, device="cuda", dtype=torch.int32), torch.ones(64, device="cuda", dtype=torch.int32)
    s = k.lib.stream_handle()
    ok = k.lib.CopyJob(a.data_ptr(), b.data_ptr(), 64)
    for bad in (k.lib.CopyJob(a.data_ptr() + 4, b.data_ptr(), 64), k.lib.CopyJob(a.data_ptr(), b.data_ptr() + 8, 64),
                k.lib.CopyJob(a.data_ptr(), b.data_ptr(), 24)):
        jobs = (k.lib.CopyJob * 2)(ok, bad)
        assert lib.vqa_copy_multi(jobs, 2, s) == 1000
    jobs = (k.lib.CopyJob * 9)(*([ok] * 9))
    assert lib.vqa_copy_multi(jobs, 9, s) == 1000
    torch.cuda.synchronize()
    assert not bool(a.any())                                 # a refused call copies nothing
