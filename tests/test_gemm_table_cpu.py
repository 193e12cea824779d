"""The GEMM tile-config table (VQA_GEMM_TILE_TABLE, include/vqa_hip.h) and the host code that reads
it: the parsed rows against a literal snapshot, vqa_gemm_select / vqa_gemm_workspace_bytes (pure
host code: no launch, no device memory), and the tuner's eligibility helper.  No GPU needed."""
import ctypes
import re

import pytest

TILES = {1: (128, 128, 3), 2: (128, 64, 4), 3: (64, 64, 4), 4: (64, 64, 2), 5: (64, 64, 3), 6: (128, 64, 2),
         7: (64, 128, 2), 8: (128, 128, 2), 9: (256, 128, 2), 10: (128, 256, 2), 11: (256, 256, 2),
         12: (256, 128, 3), 13: (64, 192, 2), 14: (128, 192, 2), 15: (64, 192, 3), 16: (128, 192, 3),
         17: (128, 64, 2), 18: (128, 128, 2), 19: (64, 64, 2), 20: (64, 128, 2),
         21: (64, 64, 2), 22: (64, 128, 2), 23: (128, 64, 2), 24: (64, 128, 2), 25: (128, 128, 3),
         26: (64, 128, 1), 27: (128, 64, 1), 28: (64, 64, 1)}
WAVES = {c: ((4, 2) if c in (9, 12, 25) else (2, 4) if c in (10, 11, 24) else (2, 2)) for c in TILES}
PATCH_ONLY = (17, 18, 19, 20, 25)
KC_B_ONLY = (13, 14, 15, 16)
BK128 = (21, 22, 23, 24)
K64_ONLY = (26, 27, 28)
FP8 = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 21, 22, 23)
NORM = (3, 4, 5, 6, 7, 21)


@pytest.fixture(scope="module")
def L(pkg):
    pkg.lib.load()
    return pkg.lib


def desc(L, m=2048, n=768, k=3072, **kw):
    d = L.GemmDesc()
    d.m, d.n, d.k, d.batch = m, n, k, 1
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def test_parsed_table_equals_the_snapshot(L):
    got = {name: getattr(L, "GEMM_" + name) for name in ("TILES", "WAVES", "PATCH_ONLY", "KC_B_ONLY", "BK128",
                                                         "K64_ONLY", "FP8", "NORM")}
    want = dict(TILES=TILES, WAVES=WAVES, PATCH_ONLY=PATCH_ONLY, KC_B_ONLY=KC_B_ONLY, BK128=BK128, K64_ONLY=K64_ONLY,
                FP8=FP8, NORM=NORM)
    assert got == want
    for name, v in got.items():                                  # dicts keyed by id, tuples in ascending id order
        assert type(v) is type(want[name]) and list(v) == sorted(v), name
    assert L.GEMM_PAIR == (3, 4, 6, 7)


def test_header_defines_agree_with_the_table(L):
    txt = open(L.HEADER).read()
    define = lambda name: int(re.search(rf"#define VQA_GEMM_{name} (\d+)", txt).group(1))
    assert define("CONFIGS") == max(L.GEMM_TILES) == len(L.GEMM_TILES)
    first, last, wide = define("PATCH_FIRST"), define("PATCH_LAST"), define("PATCH_WIDE")
    assert tuple(sorted(set(range(first, last + 1)) | {wide})) == L.GEMM_PATCH_ONLY


@pytest.mark.parametrize("batch", [1, 3])
def test_splitk_workspace_bytes_follow_the_tile(L, batch):
    """65536 counter bytes, then splitk fp32 slabs of BM x BN per tile: ragged m, n so that a wrong BM
    or BN of any row changes the tile count or the slab."""
    ws = L.load().vqa_gemm_workspace_bytes
    m, n, k = 300, 200, 1024
    cdiv = lambda a, b: -(-a // b)
    for cfg, (bm, bn, _) in L.GEMM_TILES.items():
        if cfg in L.GEMM_PATCH_ONLY:
            continue
        d = desc(L, m, n, k, batch=batch, config=cfg, splitk=2)
        assert ws(ctypes.byref(d)) == 65536 + cdiv(m, bm) * cdiv(n, bn) * batch * 2 * bm * bn * 4, cfg
        for sk in (0, 1):
            d.splitk = sk
            assert ws(ctypes.byref(d)) == 0, cfg
    # e4m3 on auto runs the 64x64 tile (k counts bytes there: 1024 bytes = 8 k-tiles, 2 slices)
    d = desc(L, m, n, k, batch=batch, fp8=1, splitk=2)
    assert ws(ctypes.byref(d)) == 65536 + cdiv(m, 64) * cdiv(n, 64) * batch * 2 * 64 * 64 * 4
    geom = dict(n=1, h=28, w=28, c=128, oh=28, ow=28, kh=3, kw=3, stride=1, pad=1)
    for cfg in (0,) + L.GEMM_PATCH_ONLY:
        d = desc(L, 28 * 28, 128, 9 * 128, a_conv=2, config=cfg, splitk=2, ga=L.ConvGeom(**geom))
        assert ws(ctypes.byref(d)) == 0, cfg
    for fp8 in (0, 1):
        for sk in (0, 2):
            d = desc(L, batch=batch, norm=L.NORM_RMS, fp8=fp8, splitk=sk)
            assert ws(ctypes.byref(d)) == 65536


def test_select_answers_the_config_that_runs(L):
    sel = lambda d: L.load().vqa_gemm_select(ctypes.byref(d))
    for cfg in L.GEMM_TILES:                                     # an explicit config as is, whatever the descriptor
        for kw in ({}, dict(fp8=1), dict(norm=L.NORM_LAYER), dict(a_conv=2), dict(a_trans=1, b_trans=1)):
            assert sel(desc(L, config=cfg, **kw)) == cfg, (cfg, kw)
    assert sel(desc(L)) == 3                                     # bf16 auto: k >= 2048
    assert sel(desc(L, fp8=1)) == 4                              # e4m3 auto runs the 64x64 / 2-stage tile
    assert sel(desc(L, 2048, 768, 128)) == 4 and sel(desc(L, 16384, 256, 1024)) == 1
    for shape in ((2048, 768, 3072), (2048, 768, 128), (16384, 256, 1024)):     # bf16 auto: 3, 4, 1
        for norm in (L.NORM_LAYER, L.NORM_RMS):
            assert sel(desc(L, *shape, norm=norm)) in L.GEMM_NORM, shape
            assert sel(desc(L, *shape, norm=norm, fp8=1)) in L.GEMM_NORM, shape
    assert sel(desc(L, 16384, 256, 1024, norm=L.NORM_RMS)) == 3 and sel(desc(L, norm=L.NORM_RMS, fp8=1)) == 4
    for w, n, want in ((56, 64, 17), (28, 128, 18), (7, 64, 19), (7, 512, 20)):
        ga = L.ConvGeom(n=2, h=w, w=w, c=64, oh=w, ow=w, kh=3, kw=3, stride=1, pad=1)
        got = sel(desc(L, 2 * w * w, n, 9 * 64, a_conv=2, ga=ga))
        assert got == want and got in L.GEMM_PATCH_ONLY


@pytest.mark.parametrize("name,kw,want", [
    ("plain AB", dict(), set(range(1, 17)) | {21, 22, 23, 24}),
    ("transposed B", dict(b_trans=1), set(range(1, 13)) | {21, 22, 23, 24}),
    ("dW (A and B transposed)", dict(a_trans=1, b_trans=1), set(range(1, 13)) | {21, 22, 23, 24}),
    ("a_conv = 1", dict(a_conv=1), set(range(1, 17))),
    ("b_conv", dict(a_trans=1, b_trans=1, b_conv=1), set(range(1, 13))),
    ("a_conv = 2", dict(a_conv=2), {17, 18, 19, 20, 25}),
    ("fp8", dict(fp8=1), {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 21, 22, 23}),
    ("norm", dict(norm=1), {3, 4, 5, 6, 7, 21}),
    ("norm, fp8", dict(norm=2, fp8=1), {3, 4, 5, 6, 7, 21}),
    ("k = 64", dict(k=64), set(range(1, 17)) | {21, 22, 23, 24, 26, 27, 28}),
    ("k = 64, transposed B", dict(k=64, b_trans=1), set(range(1, 13)) | {21, 22, 23, 24, 26, 27, 28}),
    ("k = 64, a_conv = 1", dict(k=64, a_conv=1), set(range(1, 17))),
])
def test_tuner_filter_admits_the_configs_the_library_takes(pkg, L, name, kw, want):
    d = desc(L, 2048, 768, **{"k": 1024, **kw})
    assert {c for c in range(1, pkg.tune.lib_gemm_configs() + 1) if L.gemm_config_fits(c, d)} == want
    assert set(L.GEMM_NO_SPLITK) == {17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28}
