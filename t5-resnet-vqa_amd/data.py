"""Input pipeline of the reference collate on the GPU.

`DaquarFasterRcnnT5CollateFn.collect_preprocessed_data`
(dataset_utils/resnet_vqa_daquar_dataset.py:145-231) decodes, converts,
resizes and ToTensor's every image on the host, one at a time, then tokenizes
the questions.  Here:

* decode stays on the host (JPEG entropy decoding is serial): `decode_image`
  returns the RGB uint8 HWC array cv2.imread + cvtColor(BGR2RGB) gives (PIL is
  the decoder available offline);
* `ImageBatcher` packs a batch of variable-size uint8 images into one pinned
  buffer, copies it to HBM in one async transfer (uint8: 4x fewer PCIe bytes
  than the fp32 tensors the reference moves, `:327-329` of the trainer) and one
  `vqa_resize_linear_u8` launch writes the resized ToTensor batch straight into
  the destination (e.g. the engine's static image buffer);
* questions arrive pre-tokenized (the t5-base tokenizer files cannot be fetched
  offline): `DaquarCollate` pads / truncates them exactly as
  `tokenizer(..., padding="max_length", max_length=16, truncation=True)` lays
  out ids and masks, and returns the reference batch dict.

The ViT model's collate (`DaquarVitT5CollateFn`, dataset_utils/vit_vqa_daquar_dataset.py:
127-198) is another image path: `ViTImageProcessor` = PIL BILINEAR resize to 224 x 224 (an
antialiased resample when it shrinks), rescale 1/255, normalise.  `VitImageBatcher` does it
with one `vqa_resize_pil_bilinear_u8` call, bit-equal to Pillow, from coefficient tables made
on the host (`pil_bilinear_coeffs`); `vit_text_batch` lays out the token side and
`DaquarVitCollate` returns the reference's batch dict.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import lib as L


def decode_image(path):
    """cv2.imread(path) + cv2.cvtColor(BGR2RGB): an RGB uint8 [H, W, 3] array."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class ImageBatcher:
    """Resize + ToTensor of a batch of uint8 RGB images on the GPU (cv2 INTER_LINEAR numerics).

    Buffers grow on demand and are reused; `__call__` is asynchronous on the current
    stream (the pinned staging buffer is not rewritten before the previous copy ended)."""

    def __init__(self, out_h=256, out_w=256, device="cuda"):
        self.oh, self.ow = int(out_h), int(out_w)
        self.dev = torch.device(device)
        self._host = self._dev_src = None
        self._hdesc = self._ddesc = None
        self._done = None
        L.load()

    def _ensure(self, nbytes, batch):
        if self._host is None or self._host.numel() < nbytes:
            cap = max(nbytes, 1 << 20)
            self._host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._dev_src = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        if self._hdesc is None or self._hdesc.numel() < batch * 16:
            self._hdesc = torch.empty(batch * 16, dtype=torch.uint8).pin_memory()
            self._ddesc = torch.empty(batch * 16, dtype=torch.uint8, device=self.dev)

    def __call__(self, images, out=None):
        """images: list of [H_i, W_i, 3] uint8 arrays; out: optional [B, 3, oh, ow] fp32 CUDA
        tensor to write (else a new one).  Returns the batch tensor."""
        B = len(images)
        if B == 0:
            raise ValueError("empty image batch")
        arrs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"expected [H, W, 3] uint8 images, got {a.shape}")
        sizes = [a.nbytes for a in arrs]
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        total = int(sum(sizes))
        if self._done is not None:
            self._done.synchronize()                      # the last copy out of the staging buffer ended
        self._ensure(total, B)
        host = self._host.numpy()
        for a, o in zip(arrs, offs):
            host[o:o + a.nbytes] = a.reshape(-1)
        desc = (L.ImageDesc * B)(*[L.ImageDesc(int(o), a.shape[0], a.shape[1]) for a, o in zip(arrs, offs)])
        ctypes.memmove(self._hdesc.data_ptr(), ctypes.addressof(desc), ctypes.sizeof(desc))
        self._dev_src[:total].copy_(self._host[:total], non_blocking=True)
        self._ddesc[:B * 16].copy_(self._hdesc[:B * 16], non_blocking=True)
        if out is None:
            out = torch.empty(B, 3, self.oh, self.ow, dtype=torch.float32, device=self.dev)
        if tuple(out.shape) != (B, 3, self.oh, self.ow) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous [{B}, 3, {self.oh}, {self.ow}] fp32 tensor")
        rc = L.load().vqa_resize_linear_u8(self._dev_src.data_ptr(), self._ddesc.data_ptr(), B, self.oh, self.ow,
                                           out.data_ptr(), L.stream_handle())
        L.check(rc, "vqa_resize_linear_u8")
        self._done = torch.cuda.Event()
        self._done.record()
        return out


def pad_question_ids(token_ids, max_length=16, pad_id=0):
    """tokenizer(..., padding="max_length", max_length, truncation=True) layout of already
    tokenized questions: ids truncated (keeping the final EOS, as T5's tokenizer does) or
    right-padded with pad_id; attention mask 1 on real tokens."""
    B = len(token_ids)
    ids = np.full((B, max_length), pad_id, np.int64)
    mask = np.zeros((B, max_length), np.int64)
    for b, t in enumerate(token_ids):
        t = list(t)
        if len(t) > max_length:
            t = t[:max_length - 1] + [t[-1]]
        ids[b, :len(t)] = t
        mask[b, :len(t)] = 1
    return ids, mask


class DaquarCollate:
    """`DaquarFasterRcnnT5CollateFn` (resnet_vqa_daquar_dataset.py:92-231) with the image
    path on the GPU.  A data point is a dict with `image` (uint8 RGB array) or `image_path`,
    `question_ids` (token ids, ending in EOS), and `annotation_id` (answer index)."""

    # cv2 flags the reference collate accepts as `interpolation_strategy` (:156-164); only
    # INTER_LINEAR (the default, cv2 constant 1) has a GPU kernel here
    INTERPOLATIONS = {"linear": 1, "INTER_LINEAR": 1, 1: 1}

    def __init__(self, resizing_dimensions=(256, 256), max_question_length=16, device="cuda", eval_mode=False,
                 interpolation_strategy="linear", decode_workers=0):
        if interpolation_strategy not in self.INTERPOLATIONS:
            raise NotImplementedError(f"interpolation_strategy {interpolation_strategy!r}: only cv2.INTER_LINEAR is "
                                      "implemented on the GPU (vqa_resize_linear_u8); LANCZOS4 / CUBIC would train "
                                      "on different pixels")
        w, h = resizing_dimensions                      # the reference unpacks (width, height) (:132)
        self.batcher = ImageBatcher(h, w, device)
        self.max_len = int(max_question_length)
        self.eval_mode = eval_mode
        self.dev = torch.device(device)
        self._pool = self._decode_pool(decode_workers)

    @staticmethod
    def _decode_pool(decode_workers):
        """host JPEG decode is serial per image; decode_workers > 0 decodes a batch on a thread
        pool (PIL releases the GIL while it decodes)"""
        if decode_workers and decode_workers > 0:
            from concurrent.futures import ThreadPoolExecutor
            return ThreadPoolExecutor(max_workers=int(decode_workers))
        return None

    def _decode(self, data_points):
        get = lambda dp: dp["image"] if "image" in dp else decode_image(dp["image_path"])
        if self._pool is None:
            return [get(dp) for dp in data_points]
        return list(self._pool.map(get, data_points))

    def __call__(self, data_points, out=None):
        images = self._decode(data_points)
        ids, mask = pad_question_ids([dp["question_ids"] for dp in data_points], self.max_len)
        B = len(data_points)
        dec = np.zeros((B, 20), np.int64)                 # decoder_* / answer_* (ignored by the model)
        batch = {
            "question_input_ids": torch.from_numpy(ids).to(self.dev),
            "decoder_question_input_ids": torch.from_numpy(dec).to(self.dev),
            "question_attention_masks": torch.from_numpy(mask).to(self.dev),
            "decoder_question_attention_masks": torch.from_numpy(dec).to(self.dev),
            "annotation_ids": torch.as_tensor([int(dp["annotation_id"]) for dp in data_points],
                                              dtype=torch.int64).to(self.dev),
            "pixel_values": None,
            "image_tensors": self.batcher(images, out=out),
            "question_type_ids": None,
            "answer_input_ids": torch.from_numpy(dec).to(self.dev),
            "answer_attention_masks": torch.from_numpy(dec).to(self.dev),
        }
        if self.eval_mode:
            batch["image_fns"] = [dp.get("image_path") for dp in data_points]
        return batch


PIL_PRECISION_BITS = 22          # Pillow Resample.c: 32 - 8 - 2
PIL_MAX_SIDE = 8192              # vqa_resize_pil_bilinear_u8's largest source side
_PIL_TABLES: dict = {}


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow's resampling table of one axis `in_size -> out_size` for the triangle (BILINEAR)
    filter and 8-bit pixels (Resample.c precompute_coeffs + normalize_coeffs_8bpc), in float64 and
    in Pillow's order of operations: (bounds [out, 2] int32 = {first source index, taps},
    coefs [out, ksize] int32 = the 22-bit fixed-point weights, zero past the taps).  Cached per pair."""
    key = (int(in_size), int(out_size))
    if key in _PIL_TABLES:
        return _PIL_TABLES[key]
    n_in, n_out = key
    if n_in < 1 or n_out < 1:
        raise ValueError(f"pil_bilinear_coeffs: sizes {key}")
    scale = np.float64(n_in) / np.float64(n_out)
    filterscale = max(scale, np.float64(1.0))
    support = np.float64(1.0) * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    w = np.zeros((n_out, ksize), np.float64)
    ww = np.zeros(n_out, np.float64)
    for x in range(ksize):                                 # tap by tap: Pillow's order of the sum
        a = np.abs((x + xmin - center + 0.5) / filterscale)
        w[:, x] = np.where((a < 1.0) & (x < xmax), 1.0 - a, 0.0)
        ww += w[:, x]
    w /= np.where(ww != 0.0, ww, 1.0)[:, None]
    coefs = np.where(w < 0, w * (1 << PIL_PRECISION_BITS) - 0.5, w * (1 << PIL_PRECISION_BITS) + 0.5).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    coefs.setflags(write=False)
    _PIL_TABLES[key] = (bounds, coefs)
    return bounds, coefs


def normalize_lut(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """ViTImageProcessor's rescale + normalise of the 256 levels per channel, [3, 256] fp32, in its
    fp32 arithmetic: (v / 255 - mean) / std with true division (v * (1 / 255) is not bit-equal)."""
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.stack([(v - np.float32(m)) / np.float32(s) for m, s in zip(mean, std)]).astype(np.float32)


class VitImageBatcher:
    """PIL BILINEAR resize + rescale + normalise of a batch of uint8 RGB images on the GPU
    (ViTImageProcessor numerics, bit-equal to Pillow).  ImageBatcher's contract: buffers grow on
    demand and are reused; `__call__` is asynchronous on the current stream (the pinned staging
    buffers are not rewritten before the previous copies ended).  mean 0 / std 1 gives ToTensor."""

    def __init__(self, out_h=224, out_w=224, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), device="cuda"):
        self.oh, self.ow = int(out_h), int(out_w)
        if self.oh < 1 or self.ow < 1:
            raise ValueError(f"output size {out_h} x {out_w}")
        mean, std = np.broadcast_to(mean, 3), np.broadcast_to(std, 3)
        self.lut = normalize_lut(mean, std)
        self.dev = torch.device(device)
        self._host = self._dev_src = None
        self._hmeta = self._dmeta = None
        self._work = None
        self._done = None

    def check(self, images):
        """The images as contiguous uint8 [H, W, 3] arrays; ValueError for anything this path does
        not take.  Needs no device."""
        if len(images) == 0:
            raise ValueError("empty image batch")
        arrs = []
        for im in images:
            a = np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"expected [H, W, 3] uint8 images, got {a.dtype} {a.shape}")
            h, w = a.shape[:2]
            if h > PIL_MAX_SIDE or w > PIL_MAX_SIDE:
                raise ValueError(f"image of {h} x {w}: sides up to {PIL_MAX_SIDE} are supported")
            if h > 100 * w and self.oh < h:
                raise ValueError(f"image of {h} x {w} (height > 100 x width, shrunk to {self.oh} rows): Pillow "
                                 "resamples such images vertical pass first, this path runs the horizontal "
                                 "pass first and would differ by a level")
            arrs.append(np.ascontiguousarray(a))
        return arrs

    def _ensure(self, nbytes, meta_bytes, work_bytes):
        if self._host is None or self._host.numel() < nbytes:
            cap = max(nbytes, 1 << 20)
            self._host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._dev_src = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        if self._hmeta is None or self._hmeta.numel() < meta_bytes:
            cap = max(meta_bytes, 1 << 16)
            self._hmeta = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._dmeta = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        if self._work is None or self._work.numel() < work_bytes:
            self._work = torch.empty(work_bytes, dtype=torch.uint8, device=self.dev)

    def metadata(self, arrs):
        """The launch's metadata block for the checked images `arrs`, packed back to back: one
        vqa_pil_image_desc each | the look-up table | one coefficient table per distinct
        (in, out) pair (all DAQUAR frames are 640 x 480: two tables).  Returns (block as uint8
        array, byte offset of the look-up table, byte offset of the tables).  Needs no device."""
        tabs, parts, n_ints = {}, [], 0
        for key in [(a.shape[1], self.ow) for a in arrs] + [(a.shape[0], self.oh) for a in arrs]:
            if key not in tabs:
                bounds, coefs = pil_bilinear_coeffs(*key)
                tabs[key] = (n_ints, coefs.shape[1])
                parts += [bounds.reshape(-1), coefs.reshape(-1)]
                n_ints += bounds.size + coefs.size
        desc = (L.PilImageDesc * len(arrs))()
        off = 0
        for d, a in zip(desc, arrs):
            (xt, xk), (yt, yk) = tabs[(a.shape[1], self.ow)], tabs[(a.shape[0], self.oh)]
            d.offset, d.h, d.w, d.xtab, d.ytab, d.xk, d.yk = off, a.shape[0], a.shape[1], xt, yt, xk, yk
            off += a.nbytes
        lut_off = ctypes.sizeof(desc)
        tab_off = lut_off + self.lut.nbytes
        block = np.concatenate([np.frombuffer(desc, np.uint8), self.lut.reshape(-1).view(np.uint8),
                                np.concatenate(parts).view(np.uint8)])
        return block, lut_off, tab_off

    def __call__(self, images, out=None):
        """images: list of [H_i, W_i, 3] uint8 arrays; out: optional [B, 3, oh, ow] fp32 CUDA
        tensor to write (else a new one).  Returns the batch tensor."""
        arrs = self.check(images)
        lib = L.load()
        B = len(arrs)
        total = int(sum(a.nbytes for a in arrs))
        block, lut_off, tab_off = self.metadata(arrs)
        max_h, max_w = max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs)
        work_stride = (max_h * self.ow * 3 + 15) // 16 * 16
        if out is None:
            out = torch.empty(B, 3, self.oh, self.ow, dtype=torch.float32, device=self.dev)
        if tuple(out.shape) != (B, 3, self.oh, self.ow) or out.dtype != torch.float32 or not out.is_contiguous() \
                or not out.is_cuda:
            raise ValueError(f"out must be a contiguous [{B}, 3, {self.oh}, {self.ow}] fp32 device tensor")
        if self._done is not None:
            self._done.synchronize()                      # the last copies out of the staging buffers ended
        self._ensure(total, block.nbytes, B * work_stride)
        host, off = self._host.numpy(), 0
        for a in arrs:
            host[off:off + a.nbytes] = a.reshape(-1)
            off += a.nbytes
        self._hmeta.numpy()[:block.nbytes] = block
        self._dev_src[:total].copy_(self._host[:total], non_blocking=True)
        self._dmeta[:block.nbytes].copy_(self._hmeta[:block.nbytes], non_blocking=True)
        base = self._dmeta.data_ptr()
        rc = lib.vqa_resize_pil_bilinear_u8(self._dev_src.data_ptr(), base, B, max_h, max_w, self.oh, self.ow,
                                            base + tab_off, base + lut_off, self._work.data_ptr(), work_stride,
                                            out.data_ptr(), L.stream_handle())
        L.check(rc, "vqa_resize_pil_bilinear_u8")
        self._done = torch.cuda.Event()
        self._done.record()
        return out


def vit_text_batch(data_points, max_question_length, dec_len=20):
    """The token side of `DaquarVitT5CollateFn` (vit_vqa_daquar_dataset.py:156-166) from
    pre-tokenized ids, as int64 numpy arrays.  A data point has `question_ids`
    (`[QUESTION] text </s>`), `decoder_question_ids` (`[QUESTION] text [ANSWER] </s>`),
    `annotation_id` and optionally `answer_ids`.  The question is right-padded with 0 to
    max_question_length, the engine's planned length (the reference pads to the batch's longest;
    padded keys are masked out of the encoder exactly) and never truncated, as in the reference:
    a longer one raises.  The decoder question and the answer are laid out as
    tokenizer(padding="max_length", truncation=True, max_length=dec_len); no answer: zeros."""
    L_q = int(max_question_length)
    B = len(data_points)
    q = np.zeros((B, L_q), np.int64)
    qm = np.zeros((B, L_q), np.int64)
    for b, dp in enumerate(data_points):
        t = list(dp["question_ids"])
        if len(t) > L_q:
            raise ValueError(f"question {b} has {len(t)} tokens; max_question_length is {L_q} (the reference "
                             "does not truncate questions)")
        q[b, :len(t)] = t
        qm[b, :len(t)] = 1
    d, dm = pad_question_ids([dp["decoder_question_ids"] for dp in data_points], dec_len)
    a, am = pad_question_ids([dp["answer_ids"] if dp.get("answer_ids") is not None else [] for dp in data_points],
                             dec_len)
    return {
        "question_input_ids": q, "question_attention_masks": qm,
        "decoder_question_input_ids": d, "decoder_question_attention_masks": dm,
        "answer_input_ids": a, "answer_attention_masks": am,
        "annotation_ids": np.asarray([int(dp["annotation_id"]) for dp in data_points], np.int64),
    }


class DaquarVitCollate(DaquarCollate):
    """`DaquarVitT5CollateFn` (vit_vqa_daquar_dataset.py:92-202) with the image path on the GPU.
    A data point is a dict with `image` (uint8 RGB array) or `image_path`, and vit_text_batch's
    keys.  Decoding is DaquarCollate's."""

    def __init__(self, max_question_length, image_size=224, device="cuda", eval_mode=False, decode_workers=0):
        self.batcher = VitImageBatcher(image_size, image_size, device=device)
        self.max_len = int(max_question_length)
        self.eval_mode = eval_mode
        self.dev = torch.device(device)
        self._pool = self._decode_pool(decode_workers)

    def __call__(self, data_points, out=None):
        images = self._decode(data_points)
        text = vit_text_batch(data_points, self.max_len)
        batch = {k: torch.from_numpy(text[k]).to(self.dev) for k in
                 ("question_input_ids", "decoder_question_input_ids", "question_attention_masks",
                  "decoder_question_attention_masks", "annotation_ids")}
        batch["pixel_values"] = self.batcher(images, out=out)
        batch["image_tensors"] = None
        batch["question_type_ids"] = None
        batch["answer_input_ids"] = torch.from_numpy(text["answer_input_ids"]).to(self.dev)
        batch["answer_attention_masks"] = torch.from_numpy(text["answer_attention_masks"]).to(self.dev)
        if self.eval_mode:
            batch["image_fns"] = [dp.get("image_path") for dp in data_points]
        return batch


def synthetic_images(batch, seed=0, min_side=200, max_side=640):
    """DAQUAR-like variable-size RGB uint8 images (NYU-Depth frames are 640 x 480)."""
    g = np.random.Generator(np.random.PCG64([seed & 0xFFFFFFFF, 0x1A6E]))
    out = []
    for _ in range(batch):
        h, w = int(g.integers(min_side, max_side + 1)), int(g.integers(min_side, max_side + 1))
        out.append(g.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return out


__all__ = ["decode_image", "ImageBatcher", "pad_question_ids", "DaquarCollate", "synthetic_images",
           "pil_bilinear_coeffs", "normalize_lut", "VitImageBatcher", "vit_text_batch", "DaquarVitCollate"]
