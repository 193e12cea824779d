"""Host side of the evaluation path: the similarity (WUPS) table helper and the validation of
`similarity=` in VQATrainer.evaluate, which happens before any device work (no GPU here)."""
import numpy as np
import pytest


def test_similarity_table_orientation(pkg):
    answers = ["chair", "table", "lamp"]
    calls = []

    def fn(pred, target):                                # asymmetric: tells [prediction, target] apart
        calls.append((pred, target))
        return 10 * answers.index(pred) + answers.index(target)

    tab = pkg.metrics.similarity_table(answers, fn)
    assert tab.dtype == np.float32 and tab.shape == (3, 3)
    np.testing.assert_array_equal(tab, np.array([[0, 1, 2], [10, 11, 12], [20, 21, 22]], np.float32))
    assert tab[2, 0] == fn("lamp", "chair") and tab[0, 2] == fn("chair", "lamp")
    assert len(calls) == 9 + 2
    assert pkg.trainer.similarity_table is pkg.metrics.similarity_table


def test_similarity_table_symmetric_toy(pkg):
    tab = pkg.metrics.similarity_table(range(4), lambda p, t: 1.0 if p == t else 0.25)
    np.testing.assert_array_equal(tab, np.where(np.eye(4) > 0, 1.0, 0.25).astype(np.float32))


class _NoDevice:
    """A model whose engine must never be reached."""
    answer_spaces = 5
    training = True

    @property
    def engine(self):
        raise AssertionError("evaluate touched the engine before validating `similarity`")

    def eval(self):
        raise AssertionError("evaluate changed the mode before validating `similarity`")


@pytest.mark.parametrize("bad", [np.zeros((4, 5), np.float32), np.zeros((5, 5, 1)), np.zeros(25), [[1.0, 2.0]],
                                 np.array([["a"] * 5] * 5)])
def test_evaluate_validates_similarity_first(pkg, bad):
    tr = object.__new__(pkg.trainer.VQATrainer)
    tr.model, tr.logger = _NoDevice(), None
    with pytest.raises(ValueError, match="similarity"):
        tr.evaluate([], similarity=bad)


def test_check_similarity_accepts_convertible(pkg):
    import torch
    chk = pkg.metrics.check_similarity
    assert chk(None, 5) is None
    for good in (np.ones((5, 5), np.float64), torch.ones(5, 5), [[1] * 5] * 5):
        out = chk(good, 5)
        assert out.dtype == np.float32 and out.shape == (5, 5) and out.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        chk(np.ones((5, 5)), 6)
