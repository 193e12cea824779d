"""vqa_eval_rows (include/vqa_hip.h "evaluation"): per-row top-k of log-probs and the epoch's
metric accumulators, against numpy on the host.

Everything is exact: the top-k is numpy's stable argsort of -x (equal values by ascending
index) with the values' bits, and the fp64 sums are the same sequential adds in the same order,
compared as int64 views.  Inputs are log-probs made on the CPU (seeded normal, log_softmax,
fp32)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACC_INTS = ("steps", "rows", "top1", "topk", "cursor")
ACC_F64 = ("loss_sum", "nll_sum", "sim_sum")


@pytest.fixture(scope="module")
def k(pkg):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    pkg.lib.load()
    return pkg


@functools.lru_cache(maxsize=None)
def logprobs(batch, answers, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(batch, answers, generator=g), -1).float().numpy()
    x.setflags(write=False)
    return x


def expected_topk(x, kk):
    """numpy's stable descending order; slots past the answers: index -1, value -inf."""
    B, A = x.shape
    order = np.argsort(-x, kind="stable")[:, :kk].astype(np.int32)
    vals = np.take_along_axis(x, order, 1)
    if kk > A:
        order = np.concatenate([order, np.full((B, kk - A), -1, np.int32)], 1)
        vals = np.concatenate([vals, np.full((B, kk - A), -np.inf, np.float32)], 1)
    return order, vals


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.array(a), dtype=dtype).cuda()     # (a copy: inputs are read-only)


class Run:
    """One vqa_eval_rows call; outputs start from sentinels so an unwritten slot shows."""

    def __init__(self, pkg, x, kk, tgt=None, nll=None, loss=None, sim=None, acc=None, plog=None, tlog=None,
                 capacity=0, answers=None, null_logp=False):
        B, A = x.shape
        self.idx = torch.full((B, max(kk, 1)), -7, dtype=torch.int32, device="cuda")
        self.val = torch.full((B, max(kk, 1)), 123.0, device="cuda")
        self.keep = [dev(x), dev(tgt, torch.int64), dev(nll), dev(loss), dev(sim)]
        d = pkg.lib.EvalDesc()
        d.logp, d.targets, d.nll, d.loss, d.similarity = (pkg.ops.addr(t) for t in self.keep)
        if null_logp:
            d.logp = None
        d.batch, d.answers, d.k = B, (A if answers is None else answers), kk
        d.topk_idx, d.topk_logp = self.idx.data_ptr(), self.val.data_ptr()
        d.acc, d.pred_log, d.tgt_log = pkg.ops.addr(acc), pkg.ops.addr(plog), pkg.ops.addr(tlog)
        d.capacity = capacity
        pkg.lib.call("vqa_eval_rows", ctypes.byref(d))
        torch.cuda.synchronize()

    def topk(self):
        return self.idx.cpu().numpy(), self.val.cpu().numpy()


def assert_topk(run, x, kk):
    idx, val = run.topk()
    eidx, eval_ = expected_topk(x, kk)
    np.testing.assert_array_equal(idx, eidx)
    np.testing.assert_array_equal(val.view(np.uint32), eval_.view(np.uint32))


# answers below 64, a partial last lane group, more than 256 answers (the other lanes-per-row
# kernel), more than 4 rows (one workgroup) and more than 64, k > answers
@pytest.mark.parametrize("batch,answers,kk", [(1, 1, 1), (1, 1, 4), (5, 170, 5), (4, 64, 16), (3, 65, 8),
                                             (65, 170, 5), (7, 1024, 16), (1024, 170, 1)])
def test_topk_matches_stable_argsort(k, batch, answers, kk):
    x = logprobs(batch, answers, 100 + batch + answers)
    assert_topk(Run(k, x, kk), x, kk)


def test_topk_ties_and_infinities(k):
    A = 170
    x = logprobs(6, A, 7).copy()
    x[0, :] = np.float32(-np.log(A))                     # all equal: indices 0..k-1
    m = x[1].max()
    x[1, 150], x[1, 3], x[1, 64] = m, m, m               # duplicated maxima (and the true one)
    x[2, 169] = x[2, 0] = x[2].max() + 1                 # first and last entry tie
    x[3, 5:] = -np.inf                                   # five finite entries, then -inf ties
    r = Run(k, x, 8)
    assert_topk(r, x, 8)
    idx, _ = r.topk()
    assert idx[0].tolist() == list(range(8))
    assert idx[2, :2].tolist() == [0, 169]
    assert sorted(idx[3].tolist()) == list(range(8))     # each index once
    y = np.array([[0.0, -np.inf, -np.inf, -np.inf]], np.float32)
    r = Run(k, y, 4)
    assert r.topk()[0].tolist() == [[0, 1, 2, 3]]
    assert_topk(r, y, 4)
    big = logprobs(3, 700, 9).copy()                     # the 16-answers-per-lane kernel
    big[0, 300:] = -np.inf
    big[1, 699] = big[1, 64] = big[1].max()
    assert_topk(Run(k, big, 16), big, 16)


# ---------------------------------------------------------------- accumulators
B, A, K = 37, 170, 5


@functools.lru_cache(maxsize=None)
def call_inputs(i):
    """Inputs of accumulator call i: log-probs, targets (valid rows, -100, one >= answers, one
    whose low 32 bits alone would be a valid answer), per-row nll, batch loss."""
    rs = np.random.RandomState(40 + i)
    x = logprobs(B, A, 50 + i)
    tgt = rs.randint(0, A, B).astype(np.int64)
    tgt[rs.choice(B, 9, replace=False)] = -100
    tgt[4 + i] = A
    tgt[20 + i] = (1 << 33) + 3
    top = np.argsort(-x, kind="stable")
    tgt[1], tgt[2] = top[1, 0], top[2, 3]                # a top-1 hit and a top-k-only hit
    nll = rs.rand(B).astype(np.float32) * 7
    loss = rs.rand(1).astype(np.float32) * 5
    return x, tgt, nll, loss


@functools.lru_cache(maxsize=None)
def sim_table():
    t = np.random.RandomState(3).rand(A, A).astype(np.float32)
    t.setflags(write=False)
    return t


def new_state():
    st = {n: 0 for n in ACC_INTS}
    st.update({n: np.float64(0.0) for n in ACC_F64})
    return st


def ref_accumulate(st, x, tgt, nll, loss, sim, kk, cap, plog, tlog):
    """The contract's sequential adds, on the host."""
    order = np.argsort(-x, kind="stable")[:, :kk]
    valid = [b for b in range(len(tgt)) if 0 <= tgt[b] < x.shape[1]]
    if not valid:
        return
    st["steps"] += 1
    st["loss_sum"] = st["loss_sum"] + np.float64(loss[0])
    st["rows"] += len(valid)
    for b in valid:
        p, t = int(order[b, 0]), int(tgt[b])
        st["nll_sum"] = st["nll_sum"] + np.float64(nll[b])
        st["sim_sum"] = st["sim_sum"] + np.float64(sim[p, t])
        st["top1"] += int(p == t)
        st["topk"] += int(t in order[b].tolist())
        if st["cursor"] < cap:
            plog[st["cursor"]], tlog[st["cursor"]] = p, t
        st["cursor"] += 1


def read_acc(acc):
    h = acc.cpu().numpy()
    return h[:5].tolist(), h[5:].copy()                  # int64 words; fp64 words as int64 bits


def bits(st):
    return np.array([st[n] for n in ACC_F64], np.float64).view(np.int64)


def three_calls(pkg, cap=64):
    acc = torch.zeros(8, dtype=torch.int64, device="cuda")
    plog = torch.full((cap + 8,), -99, dtype=torch.int32, device="cuda")
    tlog = torch.full((cap + 8,), -99, dtype=torch.int32, device="cuda")
    outs = []
    for i in range(3):
        x, tgt, nll, loss = call_inputs(i)
        r = Run(pkg, x, K, tgt, nll, loss, sim_table(), acc, plog, tlog, cap)
        outs.append(r.topk())
    return acc, plog, tlog, outs


def test_accumulators_match_sequential_numpy(k):
    cap = 128
    acc, plog, tlog, outs = three_calls(k, cap)
    st, ep, et = new_state(), np.full(cap + 8, -99, np.int32), np.full(cap + 8, -99, np.int32)
    for i in range(3):
        x, tgt, nll, loss = call_inputs(i)
        ref_accumulate(st, x, tgt, nll, loss, sim_table(), K, cap, ep, et)
        eidx, _ = expected_topk(x, K)
        np.testing.assert_array_equal(outs[i][0], eidx)
    ints, fbits = read_acc(acc)
    assert ints == [st[n] for n in ACC_INTS]
    assert st["steps"] == 3 and 0 < st["top1"] < st["topk"] < st["rows"] == st["cursor"]
    np.testing.assert_array_equal(fbits, bits(st))
    np.testing.assert_array_equal(plog.cpu().numpy(), ep)   # equal up to the cursor, sentinel after it
    np.testing.assert_array_equal(tlog.cpu().numpy(), et)


def test_ignored_rows_change_only_the_row_outputs(k):
    acc, plog, tlog, _ = three_calls(k)
    before = [t.clone() for t in (acc, plog, tlog)]
    x, _, nll, loss = call_inputs(0)
    ign = np.full(B, -100, np.int64)
    ign[3], ign[5] = A, -1
    for tgt in (ign, None):                                 # all ignored; targets == NULL
        r = Run(k, x, K, tgt, nll, loss, sim_table(), acc, plog, tlog, 64)
        assert_topk(r, x, K)
        for was, now in zip(before, (acc, plog, tlog)):
            assert torch.equal(was, now)


def test_capacity_bounds_the_log(k):
    cap = 10
    acc, plog, tlog, _ = three_calls(k, cap)
    st, ep, et = new_state(), np.full(cap + 8, -99, np.int32), np.full(cap + 8, -99, np.int32)
    for i in range(3):
        ref_accumulate(st, *call_inputs(i), sim_table(), K, cap, ep, et)
    ints, fbits = read_acc(acc)
    assert ints == [st[n] for n in ACC_INTS]
    assert ints[4] == st["rows"] > cap                      # cursor = the valid rows, past the capacity
    np.testing.assert_array_equal(fbits, bits(st))
    p, t = plog.cpu().numpy(), tlog.cpu().numpy()
    np.testing.assert_array_equal(p, ep)
    np.testing.assert_array_equal(t, et)
    assert (p[cap:] == -99).all() and (t[cap:] == -99).all() and (p[:cap] >= 0).all()


def test_same_calls_same_bytes(k):
    a = three_calls(k)
    b = three_calls(k)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)
    for (i1, v1), (i2, v2) in zip(a[3], b[3]):
        assert i1.tobytes() == i2.tobytes() and v1.tobytes() == v2.tobytes()


@pytest.mark.parametrize("bad", [dict(kk=0), dict(kk=17), dict(answers=1025), dict(null_logp=True)])
def test_argument_errors(k, bad):
    x = logprobs(4, 64, 1)
    kw = dict(kk=4)
    kw.update(bad)
    acc = torch.zeros(8, dtype=torch.int64, device="cuda")
    tgt = np.zeros(4, np.int64)
    with pytest.raises(RuntimeError, match="vqa_eval_rows"):
        Run(k, x, kw.pop("kk"), tgt, acc=acc, **kw)
    torch.cuda.synchronize()
    assert not acc.any()                                    # nothing launched
