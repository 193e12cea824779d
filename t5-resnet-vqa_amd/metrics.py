"""Host helpers of the evaluation path (no device work here).

The reference selects its best model by average WUPS between the predicted and the target
answer (trainer/faster_rcnn_vqa_trainer.py:440-480, utils `wup_measure` over nltk's WordNet).
Between two answers of a fixed answer space that is a fixed [answers, answers] table: it is
computed once, where nltk exists, and the evaluation kernel (vqa_eval_rows) gathers from it.
"""
from __future__ import annotations

import numpy as np


def similarity_table(answers, fn):
    """The [A, A] fp32 table `fn(answers[p], answers[t])` at [p, t]: row = the PREDICTED
    answer, column = the TARGET answer (the orientation vqa_eval_rows reads it in; `fn` need
    not be symmetric).  `fn` is e.g. the reference's wup_measure on a machine with nltk."""
    answers = list(answers)
    a = len(answers)
    tab = np.empty((a, a), np.float32)
    for p, ap in enumerate(answers):
        for t, at in enumerate(answers):
            tab[p, t] = fn(ap, at)
    return tab


def check_similarity(similarity, answers):
    """`similarity` as a contiguous [answers, answers] fp32 numpy array (None stays None);
    ValueError for anything that is not convertible to that shape."""
    if similarity is None:
        return None
    if hasattr(similarity, "detach"):                   # a torch tensor, host or device
        similarity = similarity.detach().cpu().numpy()
    try:
        tab = np.ascontiguousarray(similarity, dtype=np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(f"similarity: not convertible to a float32 array ({e})") from None
    if tab.shape != (answers, answers):
        raise ValueError(f"similarity: shape {tab.shape}, expected ({answers}, {answers}) = [prediction, target]")
    return tab
