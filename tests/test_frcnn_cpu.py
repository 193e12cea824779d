"""FasterRcnnVQAModel on the CPU: specs, layout and the oracle restatement (tests/frcnn_oracle.py)
against the fixture the reference's own class produced (tests/golden/make_golden_frcnn.py)."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import vqa_oracle as orc

import frcnn_oracle as fo

torch.set_num_threads(8)
V = "faster-rcnn"


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], dtype=np.uint64)[0]


def test_specs_match_reference_state_dict(pkg, golden):
    g = golden("model_frcnn_256_l16")
    specs = pkg.synthetic.model_specs(V)
    assert list(specs) == [str(k) for k in g["sd_keys"]]
    assert ["x".join(map(str, s)) for s in specs.values()] == [str(s) for s in g["sd_shapes"]]
    nvis = sum(pkg.synthetic.is_parameter(k, s, V) for k, s in specs.items() if k.startswith("vision_model."))
    assert nvis == int(g["vision_param_count"]) == 53 + 16
    assert "downscale_layer.weight" not in specs and specs["upscale_layer.weight"] == (256, 768, 3, 3)
    assert list(pkg.synthetic.make_state_dict(V)) == list(specs)
    with pytest.raises(ValueError):
        pkg.synthetic.model_specs("faster-rcnn-v2")


def test_existing_keys_keep_their_values(pkg):
    """The generator is keyed by key string: the new vision name moves no existing value."""
    a = pkg.synthetic.make_state_dict("resnet18", keys={"upscale_layer.weight", "lang_model.final_layer_norm.weight"})
    b = pkg.synthetic.make_state_dict(V, keys={"lang_model.final_layer_norm.weight"})
    np.testing.assert_array_equal(a["lang_model.final_layer_norm.weight"], b["lang_model.final_layer_norm.weight"])
    w = pkg.synthetic.init_param("vision_model.fpn.inner_blocks.3.0.weight", (256, 2048, 1, 1))
    assert abs(float(np.abs(w).max()) - np.sqrt(3.0 / 2048)) < 1e-4        # kaiming_uniform_(a=1)
    assert float(np.abs(pkg.synthetic.init_param("vision_model.fpn.layer_blocks.3.0.bias", (256,))).min()) > 0.0


def _trainable(pkg, lay):
    keys = set(lay.trainable_keys)
    return pkg.synthetic.make_state_dict(V, seed=3, keys=keys)


def test_layout_roundtrip_is_bit_exact(pkg):
    lay = pkg.layout.ParamLayout(V)
    assert lay.scaler == "upscale_layer" and lay.scaler_cin == 256 and lay["scaler_w"].shape == (768, 3, 3, 256)
    assert not any(k.startswith("vision_model.") for k in lay.trainable_keys)
    sd = _trainable(pkg, lay)
    flat = lay.pack(sd)
    back = lay.unpack(flat)
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert back[k].shape == v.shape
        np.testing.assert_array_equal(back[k], v)
    # the ConvTranspose2d flip: Wc[o, kh, kw, c] = W[c, o, 2 - kh, 2 - kw]
    w = sd["upscale_layer.weight"]
    sg = lay["scaler_w"]
    wc = flat[sg.offset:sg.offset + sg.numel].reshape(sg.shape)
    assert wc[5, 0, 2, 7] == w[7, 5, 2, 0] and wc[700, 1, 1, 255] == w[255, 700, 1, 1]


def test_old_fpn_key_form_is_upgraded(pkg):
    S = pkg.synthetic
    lay = pkg.layout.ParamLayout(V)
    sd = S.make_state_dict(V, seed=3, keys=set(lay.trainable_keys) | {k for k in S.model_specs(V) if ".fpn." in k})
    old = {k.replace(".0.weight", ".weight").replace(".0.bias", ".bias") if ".fpn." in k else k: v
           for k, v in sd.items()}
    assert not any(".fpn." in k and k.split(".")[4] == "0" for k in old)
    up = S.upgrade_fpn_keys(old)
    assert list(up) == list(sd)
    for k in sd:
        np.testing.assert_array_equal(up[k], sd[k])
    assert list(S.upgrade_fpn_keys(sd)) == list(sd)                       # the new form passes through
    np.testing.assert_array_equal(lay.pack(up), lay.pack(sd))


@pytest.mark.parametrize("H", [96, 224])
def test_pool_is_the_stride2_conv(pkg, H):
    """max_pool2d(P5, 1, 2) == layer_blocks.3 at stride 2 over the lateral map, at odd h (3 and 7)."""
    S = pkg.synthetic
    sd = {k: torch.as_tensor(v) for k, v in S.make_state_dict(
        V, keys={k for k in S.model_specs(V) if k.startswith("vision_model.")}).items()}
    img = torch.as_tensor(S.make_batch(2, 16, H, seed=1)["image_tensors"])
    maps = fo.fpn_maps(sd, img)
    h = maps["3"].shape[-1]
    assert h % 2 == 1 and maps["pool"].shape[-1] == (h - 1) // 2 + 1
    assert tuple(maps["0"].shape[1:]) == (256, H // 4, H // 4)
    assert float((maps["pool"] - fo.pool_stride2(sd, img)).abs().max()) <= 1e-6
    c = fo.body_features(sd, img)
    assert torch.equal(c[3], orc.resnet_features(sd, img, "resnet50", prefix=fo.BODY))


def test_oracle_matches_reference_fixture(pkg, golden):
    """tests/test_oracle_golden.py's tolerances for the ResNet cases, plus the FPN levels."""
    g = golden("model_frcnn_256_l16")
    B, L, H = int(g["B"]), int(g["L"]), int(g["H"])
    nb = pkg.synthetic.make_batch(B, L, H, seed=1)
    assert _sha(nb["image_tensors"]) == g["image_sha"], "synthetic image generator drifted"
    np.testing.assert_array_equal(nb["question_input_ids"], g["ids"])
    np.testing.assert_array_equal(nb["annotation_ids"], g["targets"])
    sd = pkg.synthetic.make_state_dict(V, seed=0)
    tr = fo.FrcnnOracleTrainer(sd, warmup=int(g["warmup"]), total=int(g["total"]))
    batch = orc.to_torch_batch(nb)
    maps = fo.fpn_maps(tr.sd, batch["image_tensors"])
    f = maps["pool"].numpy()
    np.testing.assert_allclose(f[:, :8], g["feat_slice"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose([f.sum(), np.abs(f).sum(), (f * f).sum()], g["feat_sum"], rtol=1e-4)
    for k in "0123":
        np.testing.assert_allclose(maps[k].numpy()[:, :8], g[f"pyr_slice_{k}"], atol=1e-4, rtol=1e-4)
    losses, norms, gnorms = [], [], []
    for s in range(len(g["losses"])):
        lp, loss = tr.forward_backward(batch)
        if s == 0:
            np.testing.assert_allclose(lp.numpy(), g["log_probs"], atol=2e-4)
        gn = tr.group_grad_norms()
        gnorms.append([gn[k] for k in ("lang_model", "scaler", "sga_modules", "attention_pooler",
                                       "classification_layer")])
        norms.append(float(tr.clip_and_step()))
        losses.append(float(loss))
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-5)
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=2e-4)
    np.testing.assert_allclose(np.array(gnorms), g["group_grad_norms"], rtol=5e-4)
    np.testing.assert_allclose(tr.sd["lang_model.block.0.layer.0.SelfAttention.q.weight"][:4, :16].detach().numpy(),
                               g["post_t5_q0"], atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(tr.sd["classification_layer.weight"][:4, :16].detach().numpy(), g["post_cls_w"],
                               atol=1e-7, rtol=1e-5)
    np.testing.assert_allclose(tr.sd["sga_modules.2.ffn.mlp.fc1.weight"][:4, :16].detach().numpy(),
                               g["post_sga_fc1"], atol=1e-5, rtol=1e-4)
