"""vqa_channel_cam and vqa_upsample2x_nhwc (csrc/cam.hip).

vqa_channel_cam against a float64 computation of the same bf16 inputs.  Bounds, from the inputs:
the channel mean is an fp32 sum of C exactly representable terms in some fixed order, so
|mean - ref| <= C * 2^-24 * mean_c |x| per position; through the min-max normalisation (three
such means in the quotient, and its own roundings) per image
|heat - ref| <= 4 * C * 2^-24 * max_p mean_c |x| / (max - min) + 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
# (B, P, C): one position (mean only; 0 / 0), lane groups of 32 with 2 / 16 positions, ResNet-50's
# 7 x 7 x 2048 (four loads per lane, 13 workgroups per image), 12 x 12 x 512, one lane per position
# at the largest P (four 256-position workgroups per image)
SHAPES = ((1, 1, 256), (3, 4, 256), (2, 16, 256), (2, 49, 2048), (5, 144, 512), (2, 1024, 8))
FILL = -7.0


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _inputs(B, P, C, signed):
    g = torch.Generator().manual_seed(17 * P + C + int(signed))
    x = torch.randn(B, P, C, generator=g)
    return (x if signed else x.abs()).to(torch.bfloat16).cuda()


def _cam(pkg, x, with_mean=True, cnt=None):
    B, P, C = x.shape
    mean = torch.full((B, P), FILL, device="cuda") if with_mean else None
    heat = torch.full((B, P), FILL, device="cuda")
    cnt = torch.zeros(B * pkg.lib.CAM_COUNTER_STRIDE, dtype=torch.int32, device="cuda") if cnt is None else cnt
    pkg.lib.call("vqa_channel_cam", x.data_ptr(), B, P, C, None if mean is None else mean.data_ptr(), heat.data_ptr(),
                 cnt.data_ptr())
    torch.cuda.synchronize()
    return mean, heat, cnt


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("B,P,C", SHAPES)
def test_channel_cam_matches_fp64(cuda, pkg, parity_report, B, P, C, signed):
    x = _inputs(B, P, C, signed)
    mean, heat, cnt = _cam(pkg, x)
    assert int(cnt.abs().sum()) == 0                       # the arrival counters are left at zero
    x64 = x.double()
    ref = x64.mean(-1)
    mabs = x64.abs().mean(-1)
    merr = (mean.double() - ref).abs()
    print(f"cam {B}x{P}x{C} signed={signed}: mean max-abs {float(merr.max()):.3e}")
    assert bool((merr <= C * 2.0 ** -24 * mabs).all()), float(merr.max())
    if P == 1:
        assert bool(torch.isnan(heat).all())               # a constant map: 0 / 0, as the reference's expression
        return
    mn, mx = ref.amin(1, keepdim=True), ref.amax(1, keepdim=True)
    href = (ref - mn) / (mx - mn)
    herr = (heat.double() - href).abs()
    bound = 4 * C * 2.0 ** -24 * mabs.amax(1, keepdim=True) / (mx - mn) + 1e-6
    print(f"cam {B}x{P}x{C} signed={signed}: heat max-abs {float(herr.max()):.3e} (bound {float(bound.min()):.3e})")
    parity_report.setdefault("channel_cam_heat_max_abs", {})[f"{B}x{P}x{C}_{'signed' if signed else 'abs'}"] = \
        float(herr.max())
    assert bool((herr <= bound).all()), float(herr.max())
    assert float(heat.min()) == 0.0 and float(heat.max()) == 1.0
    # mean may be NULL; a second run gives the same bits
    _, heat2, _ = _cam(pkg, x, with_mean=False, cnt=cnt)
    assert torch.equal(heat, heat2)


def test_channel_cam_graph_replay_equals_eager(cuda, pkg):
    B, P, C = 2, 49, 2048
    x = _inputs(B, P, C, True)
    mean, heat, _ = _cam(pkg, x)
    m2, h2 = torch.full((B, P), FILL, device="cuda"), torch.full((B, P), FILL, device="cuda")
    cnt = torch.zeros(B * pkg.lib.CAM_COUNTER_STRIDE, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pkg.lib.call("vqa_channel_cam", x.data_ptr(), B, P, C, m2.data_ptr(), h2.data_ptr(), cnt.data_ptr(), stream=s)
    for _ in range(2):
        h2.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(h2, heat) and torch.equal(m2, mean)


def test_channel_cam_rejects_unsupported_shapes(cuda, pkg):
    lib = pkg.lib.load()
    x = torch.zeros(2 * 1025 * 8, dtype=torch.bfloat16, device="cuda")
    heat = torch.full((2 * 1025,), FILL, device="cuda")
    cnt = torch.zeros(2 * pkg.lib.CAM_COUNTER_STRIDE, dtype=torch.int32, device="cuda")
    h = pkg.lib.stream_handle()
    for P, C, word in ((4, 12, b"multiple of 8"), (1025, 8, b"positions"), (0, 8, b"positions")):
        rc = lib.vqa_channel_cam(x.data_ptr(), 2, P, C, None, heat.data_ptr(), cnt.data_ptr(), h)
        assert rc != 0 and word in lib.vqa_last_error(), (P, C, lib.vqa_last_error())
    torch.cuda.synchronize()
    assert float(heat.min()) == FILL == float(heat.max())  # nothing was launched


@pytest.mark.parametrize("B,h,w,C", [(2, 1, 1, 256), (2, 3, 3, 256), (1, 8, 8, 64)])
def test_upsample2x_is_bit_exact(cuda, pkg, B, h, w, C):
    g = torch.Generator().manual_seed(h * 100 + C)
    src = torch.randn(B, h, w, C, generator=g).to(torch.bfloat16).cuda()
    dst = torch.full((B, 2 * h, 2 * w, C), FILL, dtype=torch.bfloat16, device="cuda")
    pkg.lib.call("vqa_upsample2x_nhwc", src.data_ptr(), dst.data_ptr(), B, h, w, C)
    torch.cuda.synchronize()
    ref = src.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(dst.view(torch.int16), ref.view(torch.int16))
    rc = pkg.lib.load().vqa_upsample2x_nhwc(src.data_ptr(), dst.data_ptr(), B, h, w, 12, pkg.lib.stream_handle())
    assert rc != 0 and b"multiple of 8" in pkg.lib.load().vqa_last_error()
