"""The GEMM tuner: picks a (tile config, split-K) for every prepared GEMM of an engine by
timing the candidates in place, keyed by the GEMM's shape and epilogue (`_gemm_key`, the
keys of tuning/gemm_gfx950.json).  EngineBase.autotune is the entry point; the engine hands
over the list of calls to tune and drops its captured graphs afterwards."""
from __future__ import annotations

import ctypes
import json
import os
import sys

import torch

from . import lib as L
from . import ops

_TUNE_CACHE = {}
_TUNE_CACHE_COLD = {}            # autotune(cold=True): choices timed from cold caches
SPLITS = (1, 2, 3, 4, 6, 8)        # split-K counts the tuner tries for small grids


def lib_gemm_configs():
    return max(L.GEMM_TILES)


def _gemm_key(d):
    geo = lambda g: (g.n, g.h, g.w, g.c, g.oh, g.ow, g.kh, g.kw, g.stride, g.pad)
    return (d.m, d.n, d.k, d.batch, d.a_trans, d.b_trans, d.a_conv, d.b_conv,
            geo(d.ga) if d.a_conv else None, geo(d.gb) if d.b_conv else None,
            bool(d.c32), bool(d.c16), bool(d.bias), bool(d.res32), bool(d.res16), bool(d.mask16), d.relu,
            d.beta != 0.0, d.drop.p > 0.0) + (("fp8",) if d.fp8 else ()) + (("norm", d.norm) if d.norm else ())


def _tune_scratch(eng, d):
    """Zero-filled split-K workspace shared by every candidate timed during tuning
    (one stream, one launch at a time; each launch leaves its counters zero)."""
    need = int(L.load().vqa_gemm_workspace_bytes(ctypes.byref(d)))
    if eng._scratch is None or eng._scratch.numel() * 4 < need:
        eng._scratch = torch.zeros(need // 4 + 4, dtype=torch.int32, device=eng.dev)
    return eng._scratch


def _apply_choice(eng, c, choice):
    """Tuning-table value = tile config + 100 * splitk (splitk 0/1 = no split).  A split
    call gets its own zero-filled workspace, kept alive by the call."""
    d = c.desc
    d.config, sk = choice % 100, choice // 100
    if d.norm:                                         # a norm tail: no split-K, its workspace stays
        assert sk <= 1 and d.config in L.GEMM_NORM, choice
        return
    if sk > 1:
        ops.set_splitk(d, sk)
        ws = ops.splitk_workspace(d, eng.dev)
        ops.set_splitk(d, sk, ws)
        c.keep = tuple(c.keep or ()) + (ws,)
    else:
        ops.set_splitk(d, 0)


def autotune(eng, calls, reps=5, table=None, save=None, cold=False):
    """Pick the fastest (tile config, split-K) for every prepared GEMM of `calls` by timing
    them in place (HIP events).  Tile configs differ only in speed: each output
    element is accumulated in the same K order whatever the tile.  Split-K
    (tried only for grids < 512 tiles) re-associates the K sum in a fixed slice
    order, so a given choice is deterministic; DP ranks stay in lockstep either
    way because they apply the same all-reduced gradient.  The committed table
    (`table`) pins the choices of known shapes.  Run after a batch is loaded and
    one forward/backward has filled the activations; it scribbles only on
    buffers the next step recomputes.

    cold: time every candidate from cold caches (a 512 MiB write evicts L2 and the
    Infinity Cache before each timed launch), as the launches run inside the step,
    where operands were written by another kernel or last read a step ago; warm
    back-to-back replays favour shallow rings.  Uses (and fills) its own cache."""
    cache = _TUNE_CACHE_COLD if cold else _TUNE_CACHE
    if table and os.path.exists(table):                # measured table (tools: bench --tune-save)
        for k, v in json.load(open(table)).items():
            cache.setdefault(k, int(v))
    s = L.stream_handle()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    flush = torch.empty(128 << 20, dtype=torch.float32, device=eng.dev) if cold else None
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]

    def time_call(c):
        c(s)
        if not cold:
            st.record()
            for _ in range(reps):
                c(s)
            en.record()
            en.synchronize()
            return st.elapsed_time(en)
        for a, b in evs:
            flush.fill_(1.0)
            a.record()
            c(s)
            b.record()
        evs[-1][1].synchronize()
        return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]
    chosen = {}
    timed = []                                         # shapes not in the table: timed here
    for c in calls:
        if c.name == "vqa_gemm_pair":
            d1, d2 = c.desc
            key = repr(("pair", _gemm_key(d1), _gemm_key(d2)))
            if key not in cache:
                timed.append(key)
                best = None
                for c1 in L.GEMM_PAIR:
                    for c2 in L.GEMM_PAIR:
                        d1.config, d2.config = c1, c2
                        t = time_call(c)
                        if best is None or t < best[0]:
                            best = (t, c1 * 10 + c2)
                cache[key] = best[1]
            d1.config, d2.config = cache[key] // 10, cache[key] % 10
            chosen[key] = cache[key]
            continue
        if c.name != "vqa_gemm" or c.desc.relu >= 2:        # GELU / tanh: one fixed kernel
            continue
        d = c.desc
        key = repr(_gemm_key(d))
        if key not in cache:
            timed.append(key)
            best = None
            nk = -(-d.k // 64)
            for cfg in range(1, lib_gemm_configs() + 1):
                if not L.gemm_config_fits(cfg, d):
                    continue
                bm, bn, _ = L.GEMM_TILES[cfg]
                tiles = -(-d.m // bm) * -(-d.n // bn) * max(1, d.batch)
                if d.norm:                             # no split-K; the descriptor's workspace = its counters
                    d.config = cfg
                    t = time_call(c)
                    if best is None or t < best[0]:
                        best = (t, cfg)
                    continue
                for sk in SPLITS:
                    # split only grids that leave CUs idle, with >= 2 k-tiles per slice
                    if sk > 1 and (tiles >= 512 or nk < 2 * sk or tiles > 16384 or cfg in L.GEMM_NO_SPLITK):
                        continue
                    d.config = cfg
                    ops.set_splitk(d, sk)
                    ops.set_splitk(d, sk, _tune_scratch(eng, d) if sk > 1 else None)
                    t = time_call(c)
                    if best is None or t < best[0]:
                        best = (t, cfg + 100 * sk)
            if not d.norm:
                ops.set_splitk(d, 0)
            cache[key] = best[1]
        _apply_choice(eng, c, cache[key])
        chosen[key] = cache[key]
    torch.cuda.synchronize(eng.dev)
    if timed:
        print(f"autotune: {len(timed)} GEMM shapes not in the table, timed at start-up "
              f"(their choice, and with split-K the rounding, can vary by box): {timed}", file=sys.stderr)
    eng._scratch = None
    if save:
        json.dump(dict(sorted(chosen.items())), open(save, "w"), indent=0)
    return chosen
