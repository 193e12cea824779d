"""Argument validation of the reference-interface mirror (no GPU needed: it fails before any allocation)."""
import pytest


def test_model_rejects_unsupported_configs(pkg):
    with pytest.raises(ValueError):
        pkg.model.ResnetVQAModel("faster-rcnn", "t5-base", 170)
    with pytest.raises(ValueError):
        pkg.model.ResnetVQAModel("resnet50", "t5-3b", 170)
    with pytest.raises(ValueError):
        pkg.model.ResnetVQAModel("resnet50", "t5-base", 170, num_attention_blocks=0)


def test_trainer_signature_mirrors_reference(pkg):
    import inspect
    sig = inspect.signature(pkg.trainer.VQATrainer.train_one_step)
    assert list(sig.parameters)[:2] == ["self", "data_items"]
    fwd = inspect.signature(pkg.model.ResnetVQAModel.forward)
    # resnet_vqa_model.py:101-112 keyword set
    assert list(fwd.parameters)[1:] == ["question_input_ids", "decoder_question_input_ids",
                                        "question_attention_masks", "decoder_question_attention_masks",
                                        "annotation_ids", "image_tensors", "answer_input_ids", "pixel_values",
                                        "answer_attention_masks", "question_type_ids"]


def test_collate_refuses_interpolations_without_a_kernel(pkg):
    """resnet_vqa_daquar_dataset.py:156-164 accepts LINEAR / LANCZOS4 / CUBIC; the GPU collate
    has the INTER_LINEAR kernel only and says so instead of training on other pixels."""
    for strategy in ("LANCZOS4", "CUBIC", 4):
        with pytest.raises(NotImplementedError):
            pkg.data.DaquarCollate(interpolation_strategy=strategy, device="cpu")


def test_short_batch_rows_are_padded_with_real_rows_and_ignored_targets(pkg):
    """A loader's short last batch (no drop_last in the reference, faster_rcnn_vqa_trainer.py:172-197)
    on a planned-B engine: rows past B' are copies of rows 0..B'-1 (every activation stays a real
    sample's) and their targets NLLLoss's ignore_index, so the head's mean runs over B' rows."""
    import torch
    E = pkg.engine
    dst = torch.full((7, 3), -1.0)
    src = torch.arange(9.0).reshape(3, 3)
    E.load_rows(dst, src, 3)
    assert torch.equal(dst, src[torch.tensor([0, 1, 2, 0, 1, 2, 0])])
    tgt = torch.zeros(7, dtype=torch.int64)
    E.load_rows(tgt, torch.tensor([5, 6, 7]), 3, fill=E.IGNORE_INDEX)
    assert tgt.tolist() == [5, 6, 7, -100, -100, -100, -100]
    full = torch.zeros(7, dtype=torch.int64)
    E.load_rows(full, torch.arange(7), 7, fill=E.IGNORE_INDEX)
    assert full.tolist() == list(range(7))
    assert E.batch_rows({"q": torch.zeros(5, 2)}, "q", 7) == 5
    for bad in (0, 8):
        with pytest.raises(ValueError):
            E.batch_rows({"q": torch.zeros(bad, 2)}, "q", 7)


def test_empty_data_parallel_rank_rows(pkg):
    """A data-parallel rank whose share of the global batch is empty (engine.use_global_rows):
    batch_rows accepts 0 rows only with allow_empty, and load_rows fills every row -- targets with
    ignore_index (the rank's gradient is exactly zero), inputs with a finite constant (masks 1)."""
    import torch
    E = pkg.engine
    assert E.batch_rows({"q": torch.zeros(0, 2)}, "q", 7, allow_empty=True) == 0
    with pytest.raises(ValueError):
        E.batch_rows({"q": torch.zeros(8, 2)}, "q", 7, allow_empty=True)
    img = torch.full((4, 3), float("nan"))
    E.load_rows(img, torch.zeros(0, 3), 0)
    assert torch.equal(img, torch.zeros(4, 3))
    mask = torch.zeros(4, 5, dtype=torch.int64)
    E.load_rows(mask, torch.zeros(0, 5, dtype=torch.int64), 0, empty_fill=1)
    assert bool((mask == 1).all())
    tgt = torch.zeros(4, dtype=torch.int64)
    E.load_rows(tgt, torch.zeros(0, dtype=torch.int64), 0, fill=E.IGNORE_INDEX)
    assert tgt.tolist() == [-100] * 4


def test_adam_range_desc_rebases_pointers_count_and_group_ends(pkg):
    """EngineBase._adam_range_desc(lo, hi): the full AdamW descriptor restricted to flat elements
    [lo, hi) -- the six arena pointers moved by `lo` elements, n = hi - lo, the group ends relative
    to `lo`, every other byte the full descriptor's.  Every sub-range update (the deferred cuts,
    the embedding rows, DP's sharded optimizer) is made by this one function."""
    import ctypes
    import types
    import torch
    L = pkg.lib
    n, ends = 20, (8, 14, 20)
    eng = types.SimpleNamespace(**{k: torch.zeros(n) for k in ("P32", "G32", "M", "V", "VMAX")},
                                P16=torch.zeros(n, dtype=torch.bfloat16))
    full = L.AdamWDesc()
    ptrs = {"param": eng.P32, "grad": eng.G32, "exp_avg": eng.M, "exp_avg_sq": eng.V, "max_exp_avg_sq": eng.VMAX,
            "param16": eng.P16}
    for f, t in ptrs.items():
        setattr(full, f, t.data_ptr())
    full.n, full.ngroups = n, len(ends)
    for i, e in enumerate(ends):
        full.group_end[i], full.group_lr[i] = e, 1e-4 * (i + 1)
    full.beta1, full.beta2, full.eps, full.weight_decay, full.grad_scale = 0.9, 0.999, 1e-8, 0.1, 0.5
    full.state = 0x1234560
    eng._adam_desc = full
    before = bytes(full)
    moved = set(ptrs) | {"n", "group_end"}
    for lo, hi in ((0, n), (4, 12), (12, n)):
        d = pkg.engine_base.EngineBase._adam_range_desc(eng, lo, hi)
        for f, t in ptrs.items():
            assert getattr(d, f) == t.data_ptr() + t.element_size() * lo, (lo, hi, f)
            assert t.element_size() == (2 if f == "param16" else 4)
        assert d.n == hi - lo
        assert [d.group_end[i] for i in range(len(ends))] == [e - lo for e in ends]
        for name, _ in L.AdamWDesc._fields_:
            fd = getattr(L.AdamWDesc, name)
            if name == "group_end":                         # the entries past ngroups stay untouched
                a, b = fd.offset + 8 * len(ends), fd.offset + fd.size
            elif name in moved:
                continue
            else:
                a, b = fd.offset, fd.offset + fd.size
            assert bytes(d)[a:b] == before[a:b], (lo, hi, name)
        assert ctypes.sizeof(d) == len(before)
    assert bytes(full) == before                            # the full descriptor is only read


def test_both_engines_share_one_base_and_engine_keeps_its_exports(pkg):
    """VQAEngine and VitVQAEngine inherit EngineBase (no method of one assigned into the other),
    and the helpers that moved into engine_base still resolve through `engine`."""
    import types
    base, V, T = pkg.engine_base.EngineBase, pkg.engine.VQAEngine, pkg.vit_engine.VitVQAEngine
    assert issubclass(V, base) and issubclass(T, base) and not issubclass(T, V)
    own = {f for f in vars(V).values() if isinstance(f, types.FunctionType)}
    own |= {p.fget for p in vars(V).values() if isinstance(p, property)}
    for name, v in vars(T).items():
        f = v.fget if isinstance(v, property) else v
        assert not any(f is g for g in own), name
        if isinstance(f, types.FunctionType):
            assert f.__qualname__.startswith("VitVQAEngine."), name
    for name in ("BF16", "F32", "I64", "IGNORE_INDEX", "SITE_EMBED", "SITE_FINAL", "t5_site", "_Seq", "no_gc_capture",
                 "_check_attn_path", "_h2d", "batch_rows", "load_rows", "_after"):
        assert getattr(pkg.engine, name) is getattr(pkg.engine_base, name), name
    assert callable(pkg.engine.stem_s2d_weight) and callable(pkg.engine.sga_site)      # these stayed
    assert pkg.dp._after is pkg.engine_base._after
