"""The engine's plan depends on its arguments and shapes alone: the retired A/B switches
(VQA_STEM, VQA_RES_FUSE_DS, VQA_EMBED_SPLIT, VQA_EMB_GRID) no longer select anything.  Engines
are only built here; no step runs."""
import pytest

RETIRED = {"VQA_STEM": "gemm", "VQA_RES_FUSE_DS": "0", "VQA_EMBED_SPLIT": "0", "VQA_EMB_GRID": "32"}


def _engine(pkg, image):
    sd = _engine.sd = getattr(_engine, "sd", None) or pkg.synthetic.make_state_dict("resnet50", seed=0)
    return pkg.engine.VQAEngine(sd, vision="resnet50", batch=2, seq_len=16, image_size=image)


@pytest.mark.gpu
def test_t5_dw_group_int_is_its_list(pkg):
    """A group size is kept as the list of group sizes it stands for, and plans what that list
    plans; 1 is the paired per-layer form, with one mark per T5 layer."""
    sd = pkg.synthetic.make_state_dict("resnet50", seed=0)

    def build(g):
        return pkg.engine.VQAEngine(sd, vision="resnet50", batch=2, seq_len=16, image_size=64, t5_dw_group=g)

    def plan(eng):
        return [(c.name, c.side) for c in eng.bwd_calls]
    by_size, by_list = build(4), build((4, 4, 4))
    assert by_size.t5_dw_groups == [4, 4, 4] == by_list.t5_dw_groups
    assert plan(by_size) == plan(by_list) and by_size.ready_marks == by_list.ready_marks
    paired = build(1)
    assert paired.t5_dw_groups is None
    ends = {sg.offset + (sg.numel + 63) // 64 * 64 for sg in (paired.lay[f"t5.{i}.ln1"] for i in range(paired.nl))}
    assert len(ends) == paired.nl and ends <= {end for _, end in paired.ready_marks}


def _names(eng):
    return {k: [c.name for c in getattr(eng, k)] for k in ("res_calls", "opt_calls", "tail_calls", "emb_pre")}


@pytest.mark.gpu
def test_plan_ignores_retired_switches_and_stem_follows_the_image_size(pkg, monkeypatch):
    for k in RETIRED:
        monkeypatch.delenv(k, raising=False)
    plain = _names(_engine(pkg, 64))
    for k, v in RETIRED.items():
        monkeypatch.setenv(k, v)
    eng = _engine(pkg, 64)
    assert _names(eng) == plain
    # H % 32 == 0: the fused image -> pooled-map stem; the split embedding update with its 256-block grid
    assert eng.res_calls[0].name == "vqa_stem_pool_img" and eng.IMG8 is None
    assert eng.embed_split and [c.name for c in eng.emb_pre] == ["vqa_embed_mark", "vqa_adamw_rows"]
    assert eng.emb_pre[1].args[4] == 256
    # any other even H (80: a 40 x 40 stem map pooled to 20 x 20): space-to-depth image,
    # implicit-GEMM stem, max-pool
    eng = _engine(pkg, 80)
    assert [c.name for c in eng.res_calls[:3]] == ["vqa_image_to_s2d16", "vqa_gemm", "vqa_maxpool3x3s2_nhwc"]
    assert tuple(eng.IMG8.shape) == (2, 41, 41, 16)


@pytest.mark.gpu
def test_tail_lists_are_the_named_compositions(pkg):
    """opt_calls, tail_calls_unfused, tail_calls and emb_pre are the tail's named calls
    (engine.StepTail) in the documented order, the very objects: with the deferred update the row
    split and the fused tail, without it the whole AdamW pass after finalize and nothing split."""
    sd = pkg.synthetic.make_state_dict("resnet50", seed=0)

    def build(**kw):
        eng = pkg.engine.VQAEngine(sd, vision="resnet50", batch=2, seq_len=16, image_size=64, **kw)
        t = eng.tail
        assert [c.name for c in (t.sq_a, t.sq_b, t.sq_c, t.finalize)] == ["vqa_grad_sqnorm"] * 3 + ["vqa_optim_finalize"]
        assert eng.opt_calls == t.dense and eng.tail_calls_unfused == t.split and eng.tail_calls == t.short
        return eng, t
    eng, t = build()
    assert eng.embed_split and eng.fused_tail
    assert eng.opt_calls == [t.sq_a, t.sq_b, t.sq_c, t.finalize, eng.adam_embed]
    assert eng.tail_calls_unfused == [t.sq_c, t.finalize, t.relbias, t.rows_touched]
    assert eng.tail_calls == [t.sq_final, t.relbias, t.rows_touched]
    assert eng.emb_pre == [t.mark, t.rows_rest] and (eng.emb_sort_call, eng.emb_scatter_call) == (t.sort, t.scatter)
    assert [c.name for c in eng.tail_calls + eng.emb_pre + [t.sort, t.scatter]] == [
        "vqa_grad_sqnorm_final", "vqa_adamw_amsgrad", "vqa_adamw_rows", "vqa_embed_mark", "vqa_adamw_rows",
        "vqa_embedding_sort", "vqa_embedding_bwd_sorted"]
    assert (t.rows_rest.args[4], t.rows_touched.args[4]) == (256, 1)
    eng, t = build(defer_optimizer=False)
    assert not eng.embed_split and not eng.fused_tail
    assert eng.opt_calls == [t.sq_a, t.sq_b, t.sq_c, t.finalize, eng.adam_full] + eng.quant_all
    assert eng.tail_calls == eng.tail_calls_unfused == [t.sq_c, t.finalize, eng.adam_full] + eng.quant_all
    assert eng.emb_pre == [] and eng.emb_sort_call is None and eng.emb_scatter_call is None
    assert (t.mark, t.rows_rest, t.relbias, t.rows_touched, t.sort, t.scatter, t.sq_final) == (None,) * 7


PLANS = {"defaults": {}, "fuse_norm": dict(fuse_norm=True), "fp8": dict(fp8=True),
         "fp8_fuse_norm": dict(fp8=True, fuse_norm=True), "paired_dw": dict(t5_dw_group=1, sga_dw_batch=False),
         "sga_attn_group_off": dict(sga_attn_group=False), "blocks_1": dict(num_blocks=1),
         "blocks_2": dict(num_blocks=2)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANS))
def test_planned_calls_keep_their_buffers_and_fp8_sites(pkg, name):
    """Every forward / backward call of every plan variant owns (through `keep`) each address it
    passes, and with fp8 exactly the weight GEMMs meant to run on e4m3 operands do: the T5 q|k|v,
    o, wi, wo per layer, the three batched SGA GEMMs (q|k|v, merge, q2), and kv2, m2, fc1, fc2 per
    block."""
    kw = PLANS[name]
    nb = kw.get("num_blocks", 3)
    sd = pkg.synthetic.make_state_dict("resnet50", seed=0, num_attention_blocks=nb)
    eng = pkg.engine.VQAEngine(sd, vision="resnet50", batch=2, seq_len=16, image_size=64, **kw)
    assert eng.NB == nb == len(eng.sga)
    for c in eng.fwd_calls + eng.bwd_calls:
        assert not pkg.ops.uncovered_pointers(c), (c.name, pkg.ops.uncovered_pointers(c))
    fp8 = [c for c in eng.fwd_calls if c.name == "vqa_gemm" and c.desc.fp8]
    assert len(fp8) == ((4 * eng.nl + 3 + 4 * nb) if kw.get("fp8") else 0)
