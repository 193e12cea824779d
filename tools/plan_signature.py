"""Canonical, pointer-free signature of the engines' plans: an A/B of two trees whose planned
call lists must be the same (a refactor of the Python plans).  Engines are only built; no step
runs.  For every config of the matrix below and every call of fwd_calls / bwd_calls / opt_calls
(and zero_calls / tail_calls / tail_calls_unfused / emb_pre / res_calls / quant_all and the calls of
adam_segs where the engine has them) one JSON line
holds the call's name, its `side` tag, its non-address arguments, the non-pointer fields of its
descriptors, and every address as [rank of first appearance of the storage that owns it, byte
offset in that storage] (the owners are the call's `keep`, as ops.uncovered_pointers reads them;
an address no kept storage owns gets a rank of its own).  A host dropout structure passed by
address is written out by value, and the job table of vqa_colsum_batched is decoded.
An accumulating engine (use_accumulation) also gives accum_calls and finish_calls (_finish_calls()).
  python tools/plan_signature.py > plan_new.json               # once per tree, then compare
  python tools/plan_signature.py --digest-of plan_new.json     # per list: calls and a SHA-256
--issue-order: for each config of ISSUE_ORDER one eager, un-captured step is issued and every launch
and stream edge is written down in order, one JSON line per config (a replayed graph submits its
nodes in capture order, so an identical sequence means an unchanged graph):
  [list, index, stream]            a launch: the call's place in the engine's lists, where it went
  ["record", stream, n]            event n (numbered by first appearance) recorded on the stream
  ["wait_event", stream, n]        the stream waits for event n
  ["wait_stream", stream, other]   the stream waits for everything on the other
with the streams named main, side, wside and rstream."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

LISTS = ("fwd_calls", "bwd_calls", "opt_calls", "zero_calls", "tail_calls", "emb_pre", "res_calls", "quant_all",
         "adam_segs", "tail_calls_unfused", "accum_calls", "finish_calls")
MARKS = ("_fsplit", "_bsplit", "ready_marks", "_sq_split", "_t5_layer_start")
RESNET = (("defaults", {}), ("fuse_norm", dict(fuse_norm=True)),
          ("dw_group_1", dict(t5_dw_group=1, sga_dw_batch=False)), ("dw_group_4", dict(t5_dw_group=4)),
          ("dw_group_12", dict(t5_dw_group=12)), ("dw_groups_4431", dict(t5_dw_group=(4, 4, 3, 1))),
          ("pipeline", dict(pipeline=True)), ("dropout_0", dict(dropout=0.0)), ("fp8", dict(fp8=True)),
          ("pair_bwd_off", dict(pair_bwd=False)), ("sga_attn_group_off", dict(sga_attn_group=False)),
          ("blocks_1", dict(num_blocks=1)), ("blocks_1_fuse_norm", dict(num_blocks=1, fuse_norm=True)),
          ("fp8_fuse_norm", dict(fp8=True, fuse_norm=True)), ("defer_optimizer_off", dict(defer_optimizer=False)),
          ("large_6_fp8", dict(language_model="t5-large", num_blocks=6, fp8=True)))
ACCUM = {"accum_2": {}, "accum_2_pipeline": dict(pipeline=True)}        # engines after use_accumulation(2)
ISSUE_ORDER = ("defaults", "pipeline", "fuse_norm", "defer_optimizer_off", "dw_group_1", "dw_group_12",
               "dw_groups_4431") + tuple(ACCUM)
VIT = (("vit_dropout_0.1", dict(dropout=0.1)), ("vit_dropout_0", dict(dropout=0.0)))


class Canon:
    """Addresses of one engine -> [rank, offset]."""

    def __init__(self, pkg):
        self.ops, self.L = pkg.ops, pkg.lib
        self.rank = {}

    def _owners(self, call):
        dev, host = [], []

        def add(o):
            if isinstance(o, torch.Tensor):
                st = o.untyped_storage()
                dev.append((st.data_ptr(), st.data_ptr() + st.nbytes()))
            elif isinstance(o, ctypes.Structure):
                host.append((ctypes.addressof(o), o))
            elif isinstance(o, (tuple, list)):
                for x in o:
                    add(x)
        add(call.keep or ())
        return dev, host

    def addr(self, p, owners):
        if not p:
            return None
        dev, host = owners
        for a, o in host:
            if a == p:
                return {"host": type(o).__name__, **self.struct(o, owners)}
        lo = next((a for a, b in dev if a <= p < b), None)
        key = ("storage", lo) if lo is not None else ("unowned", p)
        r = self.rank.setdefault(key, len(self.rank))
        return [r, p - lo] if lo is not None else [r, 0, "unowned"]

    def struct(self, s, owners):
        ptrs = self.ops._PTR_FIELDS.get(type(s).__name__, ()) + (("rng",) if isinstance(s, self.L.Dropout) else ()) + \
            (("ws", "out") if isinstance(s, self.L.ColsumJob) else ())
        out = {}
        for name, *_ in s._fields_:
            v = getattr(s, name)
            if name in ptrs:
                out[name] = self.addr(v, owners)
            elif isinstance(v, ctypes.Structure):
                out[name] = self.struct(v, owners)
            elif isinstance(v, ctypes.Array):
                out[name] = list(v)
            else:
                out[name] = v
        return out

    def call(self, c):
        owners = self._owners(c)
        ptr_args = {w for w, _ in self.ops._pointers(c)}
        args = []
        for i, a in enumerate(c.args):
            obj = getattr(a, "_obj", None)                      # ctypes.byref(desc)
            if obj is not None:
                args.append({type(obj).__name__: self.struct(obj, owners)})
            elif f"arg{i}" in ptr_args:
                args.append({"addr": self.addr(a, owners)})
            else:
                args.append(a)
        out = {"name": c.name, "side": bool(getattr(c, "side", False)), "args": args}
        if c.name == "vqa_colsum_batched":                      # its job table lives in device memory
            raw = c.keep[-1].cpu().numpy().tobytes()
            jobs = (self.L.ColsumJob * c.args[1]).from_buffer_copy(raw)
            out["jobs"] = [self.struct(j, owners) for j in jobs]
        return out


def flat(calls):
    for c in calls:
        if isinstance(c, tuple):                                # an adam_segs entry: (range name, call)
            c = c[1]
        if hasattr(c, "calls"):                                 # engine_base._Seq
            yield from flat(c.calls)
        else:
            yield c


def lists_of(eng):
    out = {k: getattr(eng, k) for k in LISTS if getattr(eng, k, None) is not None}
    if getattr(eng, "accum", 1) > 1:
        out["finish_calls"] = eng._finish_calls()
    return out


def signature(pkg, eng):
    cn = Canon(pkg)
    out = {k: [cn.call(c) for c in flat(v)] for k, v in lists_of(eng).items()}
    out.update({k: getattr(eng, k, None) for k in MARKS})
    return out


def digest(sig):
    """A signature with every call list replaced by its length and SHA-256 (the matrix in full is
    several MB)."""
    return {k: {"calls": len(v), "sha256": hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()}
            if k in LISTS else v for k, v in sig.items()}


SINGLE = ("clear_pending", "emb_sort_call", "emb_scatter_call", "count_call", "accum_finish")


def issue_order(pkg, eng, step):
    """The launches and stream edges of step(), in issue order.  The recording is patched in at class
    level (ops.Call, torch.cuda.Event / Stream) for the duration of the step only."""
    place = {}
    for k, v in lists_of(eng).items():
        for i, c in enumerate(flat(v)):
            place.setdefault(id(c), (k, i))
    for k in SINGLE:
        if getattr(eng, k, None) is not None:
            place.setdefault(id(getattr(eng, k)), (k, 0))
    streams = {s.cuda_stream: n for n, s in (("side", eng._side), ("wside", eng._wside), ("rstream", eng._rstream),
                                             ("main", torch.cuda.current_stream(eng.dev)))}
    sname = lambda s: streams.get(s.cuda_stream, "other")     # noqa: E731
    events, seen, nested = [], [], [0]
    Call, Event, Stream = pkg.ops.Call, torch.cuda.Event, torch.cuda.Stream
    saved = Call.__call__, Event.record, Stream.wait_event, Stream.wait_stream

    def ordinal(ev):
        if not any(e is ev for e in seen):
            seen.append(ev)                                     # kept alive: one ordinal per event
        return next(i for i, e in enumerate(seen) if e is ev)

    def edge(kind, fn, what):
        def wrapped(self, *a, **kw):
            if not nested[0]:
                events.append([kind] + what(self, *a, **kw))
            nested[0] += 1                                      # wait_stream is a record + wait_event inside
            try:
                return fn(self, *a, **kw)
            finally:
                nested[0] -= 1
        return wrapped

    def launch(self, stream_ptr):
        events.append(list(place.get(id(self), ("other", self.name))) + [streams.get(stream_ptr.value or 0, "other")])
        return saved[0](self, stream_ptr)
    Call.__call__ = launch
    Event.record = edge("record", saved[1], lambda ev, stream=None: [
        sname(stream if stream is not None else torch.cuda.current_stream()), ordinal(ev)])
    Stream.wait_event = edge("wait_event", saved[2], lambda st, ev: [sname(st), ordinal(ev)])
    Stream.wait_stream = edge("wait_stream", saved[3], lambda st, other: [sname(st), sname(other)])
    try:
        step()
    finally:
        Call.__call__, Event.record, Stream.wait_event, Stream.wait_stream = saved
    torch.cuda.synchronize(eng.dev)
    return events


def one_step(pkg, eng, dev):
    """The eager step of `eng` at the tool's shapes, as a function to record."""
    B, k = eng.B, eng.accum
    nb = {key: torch.as_tensor(v).to(dev) for key, v in pkg.synthetic.make_batch(k * B, 16, 64, seed=1).items()
          if v is not None}
    nxt = nb["image_tensors"][:B] if eng.pipeline else None
    if eng.pipeline:
        eng.prime(nb["image_tensors"][:B])
    if k > 1:
        return lambda: eng.accum_step(nb, next_images=nxt, use_graph=False)
    eng.load_batch(nb, next_images=nxt)
    torch.cuda.synchronize(eng.dev)
    return eng._step_pipelined if eng.pipeline else eng._run_step_streams


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--digest-of", default=None, metavar="FILE",
                    help="print the digest form of a saved signature (no engine is built, no GPU needed)")
    ap.add_argument("--only", default=None, help="comma-separated config names (default: the whole matrix)")
    ap.add_argument("--vision", default="resnet50", help="vision model of the VQAEngine configs (resnet50, resnet34, "
                    "resnet18, faster-rcnn); the config names get it as a prefix unless it is resnet50")
    ap.add_argument("--issue-order", action="store_true",
                    help="issue one eager step per config of ISSUE_ORDER and print its launches and stream edges")
    args = ap.parse_args()
    if args.digest_of:
        for line in open(args.digest_of):
            print(json.dumps(digest(json.loads(line)), sort_keys=True))
        return
    pkg = load_package()
    only = set(args.only.split(",")) if args.only else None
    sds = {}                                                    # state dicts by (blocks, language model)
    vsd = pkg.vit_model.make_state_dict(seed=0, image=32)
    matrix = RESNET + tuple(ACCUM.items()) + VIT
    if args.issue_order:
        matrix = tuple((name, dict(matrix)[name]) for name in ISSUE_ORDER)
    for name, kw in matrix:
        if only and name not in only:
            continue
        if name.startswith("vit_"):
            eng = pkg.vit_engine.VitVQAEngine(vsd, batch=2, seq_len=16, dec_len=8, image_size=32, device=args.device,
                                              **kw)
        else:
            key = (kw.get("num_blocks", 3), kw.get("language_model", "t5-base"))
            if key not in sds:
                sds[key] = pkg.synthetic.make_state_dict(args.vision, seed=0, num_attention_blocks=key[0],
                                                         language_model=key[1])
            eng = pkg.engine.VQAEngine(sds[key], vision=args.vision, batch=2, seq_len=16, image_size=64,
                                       device=args.device, **kw)
            if name in ACCUM:
                eng.use_accumulation(2)
            if args.vision != "resnet50":
                name = f"{args.vision}_{name}"
        if args.issue_order:
            print(json.dumps({"config": name, "issue_order": issue_order(pkg, eng, one_step(pkg, eng, args.device))}))
        else:
            print(json.dumps({"config": name, **signature(pkg, eng)}, sort_keys=True))
        del eng


if __name__ == "__main__":
    main()
