"""CPU restatement of Pillow's 8-bit BILINEAR resample (src/libImaging/Resample.c:
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) and of
ViTImageProcessor's rescale + normalise, which vqa_resize_pil_bilinear_u8 and data.VitImageBatcher
are held to.  Pillow itself defines the expected bytes (tests/test_vit_collate_cpu.py checks this
file against it); the restatement is what states the tables the kernel reads.

Scalar Python floats are IEEE doubles, Resample.c's type, and the statements keep its order."""
import math

import numpy as np

PRECISION_BITS = 22          # 32 - 8 - 2


def triangle(a):
    a = abs(a)
    return 1.0 - a if a < 1.0 else 0.0


def coeffs(in_size, out_size):
    """(bounds [out, 2] int32 = {xmin, taps}, k [out, ksize] int32) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [triangle((x + xmin - center + 0.5) / filterscale) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            kk[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return bounds, kk


def _pass(img, out_size):
    """One pass along axis 0 of img [n, m, 3] uint8 -> [out_size, m, 3] uint8."""
    bounds, kk = coeffs(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], 1)
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resize_bilinear_u8(img, oh, ow, vertical_first=False):
    """PIL.Image.fromarray(img).resize((ow, oh), Image.BILINEAR) of a uint8 [H, W, 3] array: the
    horizontal pass, then the vertical one, each through an 8-bit image; a pass whose size does
    not change is skipped.  vertical_first: the order Pillow takes for h > 100 * w, oh < h."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]

    def horizontal(a):
        return a if a.shape[1] == ow else _pass(a.transpose(1, 0, 2), ow).transpose(1, 0, 2)

    def vertical(a):
        return a if a.shape[0] == oh else _pass(a, oh)
    out = horizontal(vertical(img)) if vertical_first else vertical(horizontal(img))
    return np.ascontiguousarray(out)


def lut(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """[3, 256] fp32: ViTImageProcessor's rescale (v / 255, fp32 true division) and normalise."""
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.stack([(v - np.float32(m)) / np.float32(s) for m, s in zip(mean, std)])


def pixel_values(images, oh, ow, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resize=resize_bilinear_u8):
    """[B, 3, oh, ow] fp32 batch: lut[c][resize(image)] in CHW."""
    t = lut(mean, std)
    out = np.empty((len(images), 3, oh, ow), np.float32)
    for b, im in enumerate(images):
        r = resize(im, oh, ow)
        for c in range(3):
            out[b, c] = t[c][r[:, :, c]]
    return out


SOURCE_SHAPES = [(480, 640), (1, 1), (224, 224), (224, 500), (500, 224), (7, 3), (223, 225), (448, 448), (1, 700)]


def source_images(seed=3):
    """The sources the restatement was verified on against Pillow (H x W): SOURCE_SHAPES of
    uniform noise, and 100 x 1000 of 0 / 255 noise (every sum at an extreme of the range)."""
    g = np.random.default_rng(seed)
    imgs = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCE_SHAPES]
    imgs.append((g.integers(0, 2, (100, 1000, 3)) * 255).astype(np.uint8))
    return imgs


def pillow_resize(img, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
