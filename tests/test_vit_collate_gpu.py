"""The ViT collate's image path on the GPU (vqa_resize_pil_bilinear_u8 through
data.VitImageBatcher / data.DaquarVitCollate) against Pillow itself: bit-exact fp32 output for
variable-size images (down- and up-scaling, one axis each way, identity passes, 1-pixel sides),
the ToTensor look-up, reused staging buffers, a training step fed straight from it
(dataset_utils/vit_vqa_daquar_dataset.py:127-198) and the export's argument checks."""
import numpy as np
import pytest
import torch

import pil_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def sources():
    """The ten sources of the CPU test and a 900 x 1200 one (ksize 13 to 224)."""
    return po.source_images() + [np.random.default_rng(1).integers(0, 256, (900, 1200, 3), dtype=np.uint8)]


def _pillow(images, oh, ow, **kw):
    return po.pixel_values(images, oh, ow, resize=po.pillow_resize, **kw)


def _assert_bits(got, ref):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (len(bad), bad[:5])


@pytest.mark.parametrize("oh,ow", [(224, 224), (5, 9), (37, 300)])
def test_batch_equals_pillow_bit_exact(cuda, pkg, sources, oh, ow):
    _assert_bits(pkg.data.VitImageBatcher(oh, ow)(sources), _pillow(sources, oh, ow))


def test_to_tensor_lut(cuda, pkg, sources):
    imgs = sources[:1] + sources[5:7]
    got = pkg.data.VitImageBatcher(224, 224, mean=(0, 0, 0), std=(1, 1, 1))(imgs)
    ref = np.stack([po.pillow_resize(im, 224, 224).astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
                    for im in imgs])
    _assert_bits(got, ref)


def test_reuse_and_growth(cuda, pkg, sources):
    """3, then 9, then 2 images through one batcher: the staging buffers, the metadata block and the
    workspace grow and are reused; the same input twice gives the same bits."""
    vb = pkg.data.VitImageBatcher(37, 300)
    order = [sources[5:8], sources[1:10], [sources[0], sources[10]]]
    ref = {i: _pillow(b, 37, 300) for i, b in enumerate(order)}
    for i, b in enumerate(order):
        _assert_bits(vb(b), ref[i])
    first = vb(order[1]).clone()
    again = vb(order[1])
    assert torch.equal(first, again)
    _assert_bits(again, ref[1])


def test_collate_into_engine_and_step(cuda, pkg, tmp_path):
    """PNGs (lossless) decoded on the host and resampled straight into the ViT engine's pixel
    buffer; a training step and predict take the collate's dict."""
    from PIL import Image
    B, L, H, A = 4, 16, 224, 170
    Q, ANS, EOS = 32100, 32101, 1
    imgs = pkg.data.synthetic_images(B, seed=11, min_side=40, max_side=120)
    pts = []
    for i, a in enumerate(imgs):
        p = tmp_path / f"im{i}.png"
        Image.fromarray(a).save(p)
        t = list(range(5, 5 + 3 * i))
        pts.append({"image_path": str(p), "question_ids": [Q] + t + [EOS],
                    "decoder_question_ids": [Q] + t + [ANS, EOS], "annotation_id": 7 * i})
    sd = pkg.vit_model.make_state_dict(seed=0)
    m = pkg.model.VitVQAModel(answer_spaces=A, batch_size=B, seq_len=L, image_size=H, state_dict=sd, dropout=0.1)
    eng = m.engine
    col = pkg.data.DaquarVitCollate(L, image_size=H)
    batch = col(pts, out=eng.PIX)                      # resampled straight into the engine's buffer
    assert batch["pixel_values"].data_ptr() == eng.PIX.data_ptr()
    assert batch["image_tensors"] is None and batch["question_type_ids"] is None and "image_fns" not in batch
    ref = _pillow(imgs, H, H)
    _assert_bits(eng.PIX, ref)
    assert batch["question_input_ids"].shape == (B, L) and int(batch["question_attention_masks"][3].sum()) == 11
    assert batch["decoder_question_input_ids"].shape == batch["answer_input_ids"].shape == (B, 20)
    lp, loss = eng.forward_backward(batch)
    assert np.isfinite(loss) and lp.shape == (B, A)
    _assert_bits(eng.PIX, ref)                         # loading its own buffer left it as it was
    idx, top = m.predict(batch["question_input_ids"], batch["decoder_question_input_ids"],
                         batch["question_attention_masks"], batch["decoder_question_attention_masks"],
                         batch["pixel_values"], batch["annotation_ids"])
    assert idx.shape == (B, 5) and top.shape == (B, 5) and bool(torch.isfinite(top).all())
    lp2, loss2 = m(**batch)                            # forward(**batch) takes every key
    assert lp2.shape == (B, A) and bool(torch.isfinite(loss2))
    ev = pkg.data.DaquarVitCollate(L, image_size=H, eval_mode=True)(pts)
    assert ev["image_fns"] == [p["image_path"] for p in pts]
    assert ev["pixel_values"].data_ptr() != eng.PIX.data_ptr()
    _assert_bits(ev["pixel_values"], ref)


def test_export_argument_checks(cuda, pkg):
    """Refused before any launch: a source side of 8193, a null workspace, null tables, a workspace
    stride below max_h * ow * 3.  The pointers passed are real (small) buffers; `out` stays as it was."""
    L_ = pkg.lib
    lib = L_.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 4, 4), 7.0, device="cuda")
    p, s = buf.data_ptr(), L_.stream_handle()

    def call(max_h=8, max_w=8, tables=p, lut=p, work=p, stride=8 * 4 * 3):
        return lib.vqa_resize_pil_bilinear_u8(p, p, 1, max_h, max_w, 4, 4, tables, lut, work, stride, out.data_ptr(), s)
    for kw, word in [({"max_w": 8193}, "8192"), ({"max_h": 8193, "stride": 8193 * 12}, "8192"),
                     ({"work": None}, "workspace"), ({"tables": None}, "tables"), ({"lut": None}, "look-up"),
                     ({"stride": 8 * 4 * 3 - 1}, "stride")]:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(RuntimeError, match=word):
            L_.check(rc, "vqa_resize_pil_bilinear_u8")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="8192"):
        pkg.data.VitImageBatcher(4, 4)([np.zeros((2, 8193, 3), np.uint8)])
