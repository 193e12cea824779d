"""The ViT collate (dataset_utils/vit_vqa_daquar_dataset.py:127-198) on the CPU: the restatement
of Pillow's BILINEAR resample (tests/pil_oracle.py) against Pillow itself, the host coefficient
tables and look-up table of data.VitImageBatcher against the restatement and ViTImageProcessor,
the token side, and the input checks that need no device."""
import numpy as np
import pytest

import pil_oracle as po

OUTPUTS = [(224, 224), (5, 9)]


@pytest.fixture(scope="module")
def sources():
    return po.source_images()


@pytest.mark.parametrize("oh,ow", OUTPUTS)
def test_oracle_equals_pillow(sources, oh, ow):
    for im in sources:
        ref = po.pillow_resize(im, oh, ow)
        got = po.resize_bilinear_u8(im, oh, ow)
        assert got.shape == ref.shape == (oh, ow, 3)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (im.shape[:2], len(bad), bad[:5])


@pytest.mark.parametrize("n_in,n_out", [(640, 224), (480, 224), (3, 224), (224, 224), (1536, 224)])
def test_coeff_tables_equal_oracle(pkg, n_in, n_out):
    bounds, coefs = pkg.data.pil_bilinear_coeffs(n_in, n_out)
    rb, rk = po.coeffs(n_in, n_out)
    assert bounds.dtype == np.int32 and coefs.dtype == np.int32
    assert bounds.shape == (n_out, 2) and coefs.shape == rk.shape
    assert np.array_equal(bounds, rb) and np.array_equal(coefs, rk)
    ksize = coefs.shape[1]
    assert ksize == int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
    assert (np.abs(coefs.sum(1).astype(np.int64) - (1 << 22)) <= ksize).all()
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all()
    assert (bounds[:, 1] <= ksize).all()
    for o in range(n_out):                                 # nothing past the taps
        assert not coefs[o, bounds[o, 1]:].any()
    assert pkg.data.pil_bilinear_coeffs(n_in, n_out)[1] is coefs          # one table per pair


def test_identity_pass_copies(pkg):
    """in == out: every output takes its own source pixel with the weight 2^22, so running the pass
    gives the bytes that skipping it (as Pillow does) gives."""
    bounds, coefs = pkg.data.pil_bilinear_coeffs(224, 224)
    assert np.array_equal(bounds[:, 0], np.arange(224))
    assert (coefs[:, 0] == 1 << 22).all() and not coefs[:, 1:].any()


def _ramps():
    """Two 224 x 224 images that hold every level in every channel."""
    i = np.arange(224 * 224).reshape(224, 224)
    a = np.stack([i % 256, (i // 3) % 256, (i * 7 + 5) % 256], -1).astype(np.uint8)
    return [a, np.ascontiguousarray(255 - a.transpose(1, 0, 2))]


def test_lut_is_the_processor_formula(pkg):
    """The look-up table is (v / 255 - mean) / std in fp32 with true division, applied per pixel."""
    lut = pkg.data.normalize_lut()
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    assert np.array_equal(lut, po.lut())
    for a in _ramps():
        assert all(len(np.unique(a[:, :, c])) == 256 for c in range(3))
        ref = ((a.astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)
        got = np.stack([lut[c][a[:, :, c]] for c in range(3)], -1)
        assert np.array_equal(got, ref)
    tt = pkg.data.normalize_lut((0, 0, 0), (1, 1, 1))                    # ToTensor
    assert np.array_equal(tt[1], np.arange(256, dtype=np.float32) / np.float32(255.0))


def test_lut_equals_vit_image_processor(pkg):
    transformers = pytest.importorskip("transformers")
    proc = transformers.ViTImageProcessor()
    ramps = _ramps()
    ref = np.asarray(proc(images=ramps, return_tensors="np")["pixel_values"])
    assert ref.shape == (2, 3, 224, 224) and ref.dtype == np.float32
    lut = pkg.data.normalize_lut()
    for b, a in enumerate(ramps):                          # 224 x 224: the resize is the identity
        got = np.stack([lut[c][a[:, :, c]] for c in range(3)])
        assert np.array_equal(got, ref[b])


def test_vit_text_batch_layout(pkg):
    Q, A, EOS = 32100, 32101, 1
    texts = [[5, 6, 7], list(range(10, 19)), list(range(100, 130))]
    pts = [{"question_ids": [Q] + t + [EOS], "decoder_question_ids": [Q] + t + [A, EOS], "annotation_id": 3 * i}
           for i, t in enumerate(texts)]
    pts[1]["answer_ids"] = [77, 78, EOS]
    out = pkg.data.vit_text_batch(pts, 40)
    for k in ("question_input_ids", "question_attention_masks", "decoder_question_input_ids",
              "decoder_question_attention_masks", "answer_input_ids", "answer_attention_masks", "annotation_ids"):
        assert out[k].dtype == np.int64, k
    q, qm = out["question_input_ids"], out["question_attention_masks"]
    assert q.shape == qm.shape == (3, 40)
    for b, t in enumerate(texts):
        n = len(t) + 2
        assert q[b, :n].tolist() == [Q] + t + [EOS] and not q[b, n:].any()
        assert qm[b].tolist() == [1] * n + [0] * (40 - n)
    d, dm = out["decoder_question_input_ids"], out["decoder_question_attention_masks"]
    assert d.shape == dm.shape == (3, 20)
    assert d[0].tolist() == [Q, 5, 6, 7, A, EOS] + [0] * 14 and dm[0].tolist() == [1] * 6 + [0] * 14
    assert d[1, :12].tolist() == [Q] + texts[1] + [A, EOS] and int(dm[1].sum()) == 12
    # 33 tokens: truncated to 20 with the final EOS kept (truncation=True, max_length=20)
    assert d[2].tolist() == [Q] + texts[2][:18] + [EOS] and dm[2].all()
    a, am = out["answer_input_ids"], out["answer_attention_masks"]
    assert a.shape == am.shape == (3, 20)
    assert not a[0].any() and not am[0].any() and not a[2].any() and not am[2].any()      # no answer_ids
    assert a[1].tolist() == [77, 78, EOS] + [0] * 17 and am[1].tolist() == [1] * 3 + [0] * 17
    assert out["annotation_ids"].tolist() == [0, 3, 6]
    d8 = pkg.data.vit_text_batch(pts, 40, dec_len=8)["decoder_question_input_ids"]
    assert d8.shape == (3, 8) and d8[1].tolist() == [Q] + texts[1][:6] + [EOS]


def test_vit_text_batch_rejects_long_question(pkg):
    pts = [{"question_ids": list(range(2, 19)) + [1], "decoder_question_ids": [2, 1], "annotation_id": 0}]
    with pytest.raises(ValueError, match=r"18.*16"):
        pkg.data.vit_text_batch(pts, 16)
    assert pkg.data.vit_text_batch(pts, 18)["question_attention_masks"].all()


def test_batcher_input_checks_need_no_device(pkg):
    """Raised before any GPU call: the device named here does not exist."""
    vb = pkg.data.VitImageBatcher(224, 224, device="cuda:63")
    ok = np.zeros((8, 8, 3), np.uint8)
    for bad in (np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.int16), np.zeros((8, 8), np.uint8),
                np.zeros((8, 8, 4), np.uint8), np.zeros((3, 8, 8, 3), np.uint8), np.zeros((0, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            vb([ok, bad])
    with pytest.raises(ValueError, match="empty"):
        vb([])
    with pytest.raises(ValueError, match="8192"):
        vb([np.zeros((8193, 1, 3), np.uint8)])             # (also 100:1: the size is named first)
    with pytest.raises(ValueError, match="8192"):
        vb([np.zeros((2, 8193, 3), np.uint8)])
    with pytest.raises(ValueError, match="vertical"):
        vb([ok, np.zeros((333, 2, 3), np.uint8)])          # h > 100 w, shrunk: Pillow goes vertical-first
    # ... and those just inside the rule pass the checks: h = 100 w, and a tall image that is not shrunk
    assert len(vb.check([np.zeros((300, 3, 3), np.uint8)])) == 1
    tall = pkg.data.VitImageBatcher(400, 9, device="cuda:63")
    assert len(tall.check([np.zeros((333, 2, 3), np.uint8)])) == 1


def test_tall_image_rule_is_pillows():
    """Why the rule: for 333 x 2 Pillow's bytes are the vertical-first order's, and the
    horizontal-first order differs from them."""
    im = np.random.default_rng(9).integers(0, 256, (333, 2, 3), dtype=np.uint8)
    for oh, ow in OUTPUTS:
        ref = po.pillow_resize(im, oh, ow)
        assert np.array_equal(po.resize_bilinear_u8(im, oh, ow, vertical_first=True), ref)
