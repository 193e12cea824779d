"""Gradient accumulation without a GPU: the new exports are declared and registered (the ABI
version stays 22: new symbols only), and the row split of a global batch into micro-batches is a
pure function."""
import pytest

EXPORTS = ("vqa_grad_accumulate", "vqa_accum_advance", "vqa_accum_finish")


def test_exports_declared_and_registered(pkg):
    declared = pkg.lib.header_symbols()
    for name in EXPORTS:
        assert name in declared, f"{name} is not declared in include/vqa_hip.h"
        assert name in pkg.lib._SIGS, f"{name} is not registered in lib.py"
    assert pkg.lib.abi_version() == 22


def test_row_split(pkg):
    spans = pkg.engine.accum_spans
    assert spans(8, 4, 2) == [(0, 4), (4, 8)]
    assert spans(5, 4, 2) == [(0, 4), (4, 5)]
    assert spans(4, 4, 2) == [(0, 4), (4, 4)]                 # an empty micro-batch
    assert spans(1, 4, 4) == [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert spans(16, 4, 4) == [(0, 4), (4, 8), (8, 12), (12, 16)]
    for rows in (9, 0, -1):
        with pytest.raises(ValueError):
            spans(rows, 4, 2)
