"""The evaluation interface of both engines lives in EngineBase, VitVQAModel has the top-k
`predict` of ResnetVQAModel plus the attention rollout, and the library's ABI moved with the
two rollout exports (no GPU needed: classes, signatures and the header only)."""
import inspect

EVAL_METHODS = ("eval_plan", "eval_prepare", "eval_capture", "eval_capture_graph", "eval_step", "eval_reset",
                "eval_result")


def test_both_engines_evaluate_through_the_base(pkg):
    base, V, T = pkg.engine_base.EngineBase, pkg.engine.VQAEngine, pkg.vit_engine.VitVQAEngine
    for name in EVAL_METHODS:
        assert getattr(T, name) is getattr(base, name), name
        assert getattr(V, name) is getattr(base, name), name
    assert V.eval_step is base.eval_step
    assert V.EVAL_CAPACITY == T.EVAL_CAPACITY == base.EVAL_CAPACITY == 1 << 16
    # the two hooks stay per engine
    for cls in (V, T):
        assert "_run_eval_streams" in vars(cls) and "_eval_setup" in vars(cls), cls
    assert "rollout" in inspect.signature(base.eval_plan).parameters
    assert callable(T.attention_rollout)


def test_vit_model_predict_signature(pkg):
    sig = inspect.signature(pkg.model.VitVQAModel.predict)
    assert list(sig.parameters)[1:] == ["question_input_ids", "decoder_question_input_ids",
                                        "question_attention_masks", "decoder_question_attention_masks",
                                        "pixel_values", "annotation_ids", "topk", "rollout"]
    assert sig.parameters["annotation_ids"].default is None
    assert sig.parameters["topk"].default == 5 and sig.parameters["rollout"].default is False
    roll = inspect.signature(pkg.model.VitVQAModel.attention_rollout)
    assert roll.parameters["normalize"].default is False
    # forward(**batch)'s keyword set is accepted
    fwd = inspect.signature(pkg.model.VitVQAModel.forward)
    assert set(fwd.parameters) <= set(roll.parameters)


def test_abi_and_exports(pkg):
    assert pkg.lib.abi_version() == 22
    syms = pkg.lib.header_symbols()
    assert "vqa_attn_headmean" in syms and "vqa_rollout_cls" in syms
