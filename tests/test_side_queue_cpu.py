"""The ordering rules of the backward's side queue, read off the dry-run launch log (tests/dry_run.py): every scenario is one
run_forward(with_loss=True, defer_loss_final=True) + run_backward on a CPU-bound engine, nothing else of the engine is touched
(the detached scenario's hook calls take_detached / issue_detached, as the Trainer's does).  The rules state what the engine
does today; the logs' hashes let a later change of the queue's host code show that it issues the same sequence.

    python tests/test_side_queue_cpu.py [scenario ...]      prints scenario, entry count and SHA-256 of each log (DRY_RUN_DUMP=dir:
                                                            also writes dir/<scenario>.log) -- equal logs at two commits: the
                                                            same host-side call sequence
"""
import bisect
import functools
import os
import sys
from functools import partial

import pytest
import torch
import torch.nn as nn

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dry_run import dry_run
from oracle import tulip_oracle as O
from tulip_amd import _lib, ops
from tulip_amd.engine import TulipEngine
from tulip_amd.model import tulip as T

KW = dict(patch_size=(1, 4), in_chans=1, window_size=[2, 8], pixel_shuffle=True, circular_padding=True,
          log_transform=True, patch_unmerging=True)


def _base(**kw):
    return T.tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), **dict(KW, **kw))


def _tiny(**kw):
    cfg = O.tiny_config()
    return T.TULIP(img_size=cfg.img_size, target_img_size=cfg.target_img_size, depths=cfg.depths, embed_dim=cfg.embed_dim,
                   num_heads=cfg.num_heads, norm_layer=partial(nn.LayerNorm, eps=1e-6), **dict(KW, **kw))


# name -> (model factory, batch, engine attributes, run_backward arguments, form)
SCENARIOS = {
    "base8": (_base, 8, {}, {}, None),
    "base8_overwrite": (_base, 8, {}, dict(overwrite=True), None),
    "base8_adamw": (_base, 8, {}, dict(overwrite=True), "adamw"),
    "base8_join": (_base, 8, {}, {}, "join"),
    "base8_bucket_on_side": (_base, 8, {}, dict(bucket_on_side=True), "join"),
    "base8_detach": (_base, 8, dict(detach_buckets=True), {}, "detach"),
    "base8_inline": (_base, 8, dict(overlap_wgrad=False), {}, None),
    "base8_unfused96": (_base, 8, dict(fuse_block96_bwd=False), {}, None),
    "base64": (_base, 64, {}, dict(overwrite=True), None),
    "large2": (lambda: T.tulip_large(img_size=(16, 2048), target_img_size=(64, 2048), **KW), 2, {}, dict(overwrite=True), None),
    "tiny2_expanding": (lambda: _tiny(pixel_shuffle=False, patch_unmerging=False), 2, {}, dict(overwrite=True), None),
    "tiny2_dropout": (lambda: _tiny(drop_rate=0.1), 2, {}, dict(overwrite=True), None),
}


class Run:
    """One scenario's log and what the rules need beside it."""


@functools.lru_cache(maxsize=None)
def scenario(name) -> Run:
    factory, B, attrs, bkw, form = SCENARIOS[name]
    torch.manual_seed(0)
    model = factory().train()
    eng = TulipEngine(model)
    for k, v in attrs.items():
        setattr(eng, k, v)
    eng.bind(torch.device("cpu"))
    W_ = eng.params
    r = Run()
    r.name, r.eng, r.B, r.bkw, r.form = name, eng, B, bkw, form
    g = torch.zeros(W_.total, dtype=torch.float32)
    extra = dict(gflat=g)
    if form == "adamw":
        hyper, mask = torch.zeros(16), torch.zeros((W_.total + 63) // 64, dtype=torch.uint8)
        extra.update(hyper=hyper, exp_avg=torch.zeros_like(g), exp_avg_sq=torch.zeros_like(g), decay_mask64=mask)
    if form == "detach":
        extra["ws_det"] = torch.empty(eng.WS_ELEMS + (1 << 20), dtype=torch.float32)
    with dry_run(eng, **extra) as dry:
        P = eng.plan(B)
        det = dry.stream("detached")
        # (take_detached / issue_detached: the engine's own methods, or its side queue's where the engine has one)
        owner = eng.side if hasattr(eng, "side") else eng

        def hook(tag):
            dry.note("hook", tag)
            if form == "detach":
                d = owner.take_detached()
                dry.note("took", d is not None)
                if d is not None:
                    with torch.cuda.stream(det):
                        owner.issue_detached(d, extra["ws_det"].data_ptr())
                        dry.note("detached_done", tag)

        kw = dict(bkw)
        if form in ("join", "detach"):
            kw["join_tags"] = frozenset(t for t, _ in W_.groups)
        if form == "adamw":
            # the Trainer's eager warm-up pass collects the ranges some launch can step; the step then applies them
            eng.adam_probe = {}
            eng.run_forward(P, with_loss=True, defer_loss_final=True)
            eng.run_backward(P, g, bucket_hook=lambda tag: None, **kw)
            probe, eng.adam_probe = eng.adam_probe, None
            eng.adam_ctx = ops.adamw_ref(extra["hyper"], g, W_.flat, extra["exp_avg"], extra["exp_avg_sq"], W_.shadow,
                                         decay_mask64=extra["decay_mask64"])
            eng.adam_fused, eng.adam_sites = frozenset(probe), {}
            kw.update(apply_adamw=True, pack_at_end=True)
            del dry.log[:]
        eng.run_forward(P, with_loss=True, defer_loss_final=True)
        r.bwd0 = len(dry.log)            # index of the backward's first entry
        eng.run_backward(P, g, bucket_hook=hook, **kw)
        if form == "adamw":         # what the Trainer reads back: the ranges some launch can step, and where each was stepped
            dry.note("adam_probe", tuple(sorted((p - g.data_ptr(), n) for p, n in probe.items())))
            dry.note("adam_sites", tuple(sorted((p - g.data_ptr(), site) for p, site in eng.adam_sites.items())))
    r.dry, r.log, r.P, r.g, r.kw = dry, dry.log, P, g, kw
    return r


# ---------------------------------------------------------------------------------------------------------------- reading a log
ALL = list(SCENARIOS)
QUEUED = [n for n in ALL if n != "base8_inline"]              # scenarios whose weight gradients go through the side queue
OVERWRITE = [n for n, sc in SCENARIOS.items() if sc[3].get("overwrite")]


def _bwd(r):
    """(index, entry) of the backward's entries"""
    return [(i, e) for i, e in enumerate(r.log) if i >= r.bwd0]


def _goff(v):
    """byte offset of a logged pointer into the flat gradient, or None"""
    return v[1] if isinstance(v, tuple) and v[0] == "gflat" else None


def _items_regions(e):
    """(weight-gradient items, fold regions) of a launch entry, as dicts"""
    if e[0] != "launch":
        return [], []
    sym, a = e[1], e[3]
    if sym.startswith("tulip_wgrad_group"):
        return [dict(x) for x in a[0]], [dict(x) for x in a[2]]
    if sym.startswith("tulip_reduce_rows_multi"):
        return [], [dict(x) for x in a[0]]
    return [], []


def _writes(r, e):
    """[lo, hi) byte ranges of the flat gradient a launch entry produces (a scatter region: its whole table)"""
    W_ = r.eng.params
    numel_at = {4 * W_.offset[n]: W_.numel[n] for n in W_.names}
    out = []
    items, regions = _items_regions(e)
    for it in items:
        out.append((_goff(it["dW"]), _goff(it["dW"]) + 4 * it["Nw"] * it["Kw"]))
        if it["db"] is not None:
            out.append((_goff(it["db"]), _goff(it["db"]) + 4 * it["Nw"]))
    for g in regions:
        o = _goff(g["out"])
        if o is not None:
            out.append((o, o + 4 * (numel_at[o] if g["scatter_index"] is not None else g["n"])))
    if e[0] == "launch" and e[1] == "tulip_layernorm_bwd_params":       # (dy, x, mean, rstd, dgamma, dbeta, rows, C, ...)
        out += [(_goff(e[3][k]), _goff(e[3][k]) + 4 * e[3][7]) for k in (4, 5)]
    return out


def _group_bytes(r, tag):
    lo = 0
    for t, end in r.eng.params.groups:
        if t == tag:
            return 4 * lo, 4 * end
        lo = end
    raise KeyError(tag)


def _last_write(r, tag, role=None):
    """index of the last launch (on `role`) that writes into completion group `tag`"""
    lo, hi = _group_bytes(r, tag)
    hit = [i for i, e in _bwd(r) if (role is None or e[2] == role) and any(a < hi and lo < b for a, b in _writes(r, e))]
    return max(hit)


def _hooks(r):
    return [(i, e[1], e[2]) for i, e in _bwd(r) if e[0] == "hook"]


# ---------------------------------------------------------------------------------------------------------------- the rules
@pytest.mark.parametrize("name", ALL)
def test_events_are_recorded_before_they_are_waited_for(name):
    """A fork: the side stream waits for an event the chain recorded; the pack mark: the chain waits for one the side recorded."""
    r = scenario(name)
    recorded = {}
    for e in r.log:
        if e[0] == "record":
            recorded[e[2]] = e[1]
        elif e[0] == "wait_event":
            assert e[2] in recorded, e
            assert (e[1], recorded[e[2]]) in (("side", "chain"), ("chain", "side")), (e, recorded[e[2]])


@pytest.mark.parametrize("name", ALL)
def test_the_fork_is_enqueued_behind_the_chains_next_kernel(name):
    """Between a flush's record on the chain and the side stream's wait for it the chain issues a launch.  The early flush
    (advance=False) forks with wait_stream, no event.  Restated from the parent's behaviour: the backward's LAST fork is exempt --
    the "embed" hook joins right behind its flush, so that group is enqueued at once."""
    r = scenario(name)
    B = _bwd(r)
    forks = [(i, e[2]) for i, e in B if e[0] == "record" and e[1] == "chain"]
    assert forks or name == "base8_detach"
    for i, ev in forks[:-1]:
        j = next(k for k, e in B if e[0] == "wait_event" and e[2] == ev)
        assert r.log[j][1] == "side" and any(e[0] == "launch" and e[2] == "chain" for e in r.log[i + 1:j]), (i, j)
    for i, ev in forks[-1:]:
        assert any(e[0] == "wait_event" and e[1] == "side" and e[2] == ev for k, e in B if k > i)


def test_the_early_flush_forks_at_once():
    """fuse_block96_bwd off: the backward's last block runs unfused and its MLP-half weight gradients are enqueued mid-block"""
    r = scenario("base8_unfused96")
    B = _bwd(r)
    early = [i for i, e in B if e == ("wait_stream", "side", "chain")]
    assert len(early) == 1
    nxt = r.log[early[0] + 1]
    assert nxt[0] == "launch" and nxt[2] == "side" and nxt[1].startswith("tulip_wgrad_group")
    ops_ = {x["dY"][0] for x in _items_regions(nxt)[0]}          # what is queued so far: the last block's MLP half, not its attention half
    assert "layers.0.blocks.0.dh" in ops_ and "layers.0.blocks.0.dyb_m" in ops_ and "layers.0.blocks.0.dqkv" not in ops_


@pytest.mark.parametrize("name", QUEUED)
def test_the_backward_ends_with_the_side_stream_joined(name):
    r = scenario(name)
    last_side = max(i for i, e in _bwd(r) if (e[0] in ("launch", "hook") and e[2 if e[0] == "launch" else 1] == "side")
                    or (e[0] in ("record", "wait_event", "wait_stream") and e[1] == "side"))
    assert ("wait_stream", "chain", "side") in r.log[last_side + 1:]


def test_bucket_hooks_fire_on_the_chain_behind_a_join_one_block_late():
    r = scenario("base8_join")
    B, hooks = _bwd(r), _hooks(r)
    tags = [t for t, _ in r.eng.params.groups]
    assert [t for _, _, t in hooks] == tags and tags[-1] == "embed"
    assert all(role == "chain" for _, role, _ in hooks)
    for h, _, tag in hooks:
        w = _last_write(r, tag, "side")
        joins = [i for i, e in B if e == ("wait_stream", "chain", "side") and w < i < h]
        assert joins, tag
        if tag not in tags[-2:]:
            # the lagged hook: the group's last fork, then at least one more block on the chain, then the join and the hook
            ev = [r.log[i][2] for i in range(w, r.bwd0, -1) if r.log[i][0] == "wait_event" and r.log[i][1] == "side"][0]
            rec = r.log.index(("record", "chain", ev))
            assert any(e[0] == "launch" and e[2] == "chain" and "block_bwd" in e[1] for e in r.log[rec + 1:joins[-1]]), tag


def test_bucket_hooks_on_the_side_stream():
    r = scenario("base8_bucket_on_side")
    B, hooks = _bwd(r), _hooks(r)
    assert [t for _, _, t in hooks] == [t for t, _ in r.eng.params.groups]
    for h, role, tag in hooks:
        assert role == ("chain" if tag == "embed" else "side"), tag
        assert _last_write(r, tag) < h, tag            # the group's launches and the scatters they left for the next launch
    # the chain never waits for a bucket (restated from the parent's behaviour: its one wait_stream is the join at the very end,
    # in front of the "embed" hook)
    waits = [i for i, e in B if e == ("wait_stream", "chain", "side")]
    assert len(waits) == 1 and waits[0] == hooks[-1][0] - 1


def test_a_detached_group_runs_only_on_the_callers_stream():
    r = scenario("base8_detach")
    B = _bwd(r)
    took = [i for i, e in B if e == ("took", "chain", True)]
    done = [i for i, e in B if e[0] == "detached_done"]
    assert len(took) == len(done) >= 4
    inside = set()
    for a, b in zip(took, done):
        seg = r.log[a + 1:b]
        assert seg and all(e[0] == "launch" and e[2] == "detached" for e in seg), seg
        inside.update(range(a + 1, b))
        # the scatters the group carried are folded right behind it, on the same stream
        regs = [(k, g) for k, e in enumerate(seg) for g in _items_regions(e)[1]]
        dense = {g["out"]: k for k, g in regs if g["scatter_index"] is None and g["out"][0].startswith("apd.")}
        scat = {g["partials"]: k for k, g in regs if g["scatter_index"] is not None}
        assert set(scat) == set(dense) and all(k < scat[d] for d, k in dense.items()), (dense, scat)
    assert all(i in inside for i, e in B if e[0] == "launch" and e[2] == "detached")
    # ... and nothing of a detached group is launched on the side stream as well
    side = {w for i, e in B if e[0] == "launch" and e[2] == "side" for w in _writes(r, e)}
    det = {w for i in inside for w in _writes(r, r.log[i])}
    assert det and not (side & det)


@pytest.mark.parametrize("name", OVERWRITE)
def test_every_parameter_has_one_producer_in_overwrite_mode(name):
    """Weight-gradient items (dW, db), the fold regions that land in the flat gradient, the scatter regions' tables and the two
    ranges of the stand-alone LayerNorm parameter pass (C > 2048: it adds into ranges cleared first) are pairwise disjoint and hold
    every parameter's [offset, offset + numel)."""
    r = scenario(name)
    W_ = r.eng.params
    ranges = sorted(w for _, e in _bwd(r) for w in _writes(r, e))
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), [(a, b) for a, b in zip(ranges, ranges[1:]) if a[1] > b[0]][:4]
    starts = [a for a, _ in ranges]
    for n in W_.names:
        lo, hi = 4 * W_.offset[n], 4 * (W_.offset[n] + W_.numel[n])
        k = bisect.bisect_right(starts, lo) - 1
        assert k >= 0 and ranges[k][0] <= lo and hi <= ranges[k][1], n
    if name == "large2":
        assert any(e[0] == "launch" and e[1] == "tulip_layernorm_bwd_params" for _, e in _bwd(r))


@pytest.mark.parametrize("name", QUEUED)
def test_a_scatter_rides_in_a_later_launch_than_its_dense_fold(name):
    r = scenario(name)
    dense_at, n = {}, 0
    for i, e in _bwd(r):
        for g in _items_regions(e)[1]:
            if g["scatter_index"] is None:
                dense_at[g["out"]] = i
    for i, e in _bwd(r):
        for g in _items_regions(e)[1]:
            if g["scatter_index"] is not None:
                n += 1
                assert g["partials"] in dense_at and dense_at[g["partials"]] < i, (i, g["partials"])
                assert r.log[dense_at[g["partials"]]][2] == e[2]           # same stream: ordered
    assert n == len(r.eng.blocks)


@pytest.mark.parametrize("name", QUEUED)
def test_grouped_launch_limits(name):
    r = scenario(name)
    eng = r.eng
    ws_numel = eng.WS_ELEMS + (1 << 20)
    n = 0
    for i, e in _bwd(r):
        items, regions = _items_regions(e)
        if e[0] == "launch" and e[1].startswith("tulip_reduce_rows_multi"):
            assert len(regions) == e[3][1] <= _lib.REDUCE_REGIONS_MAX
        if not (e[0] == "launch" and e[1].startswith("tulip_wgrad_group")):
            continue
        n += 1
        a = e[3]
        assert len(items) == a[1] <= eng.wgrad_group_max <= _lib.WGRAD_GROUP_MAX
        assert len(regions) == a[3] <= _lib.REDUCE_REGIONS_MAX - 2 * len(items)
        (ws_name, ws_off), ws_bytes = a[4], a[5]
        assert ws_name == {"side": "ws_side", "detached": "ws_det"}[e[2]], (i, ws_name)       # never the chain's workspace
        assert ws_off + ws_bytes <= 4 * ws_numel
        assert sum((x["Nw"] * x["Kw"] + x["Nw"]) * x["splits"] * 4 for x in items if x["splits"] > 1) <= ws_bytes
    assert n >= 4


def test_pack_at_end_waits_for_the_last_group_that_steps_a_packed_weight():
    r = scenario("base8_adamw")
    W_ = r.eng.params
    B = _bwd(r)
    packs = [i for i, e in B if e[0] == "launch" and e[1] == "tulip_pack_bf16_multi"]
    assert packs and all(r.log[i][2] == "chain" for i in packs)
    wait = max(i for i, e in B if e[0] == "wait_event" and e[1] == "chain" and i < packs[0])
    rec = r.log.index(("record", "side", r.log[wait][2]))
    maintained = {4 * W_.offset[n] for n in W_.packed_names() if n not in W_.pk_late}
    assert maintained
    stepping = [i for i, e in B if e[0] == "launch" and e[2] == "side"
                and any(x["reserved_"] == 1 and _goff(x["dW"]) in maintained for x in _items_regions(e)[0])]
    assert stepping and max(stepping) < rec < wait < packs[0]
    # (every maintained weight is stepped beside the backward, by a side launch)
    stepped = {_goff(x["dW"]) for i in stepping for x in _items_regions(r.log[i])[0] if x["reserved_"] == 1}
    assert maintained - stepped <= {4 * W_.offset[n] for n in W_.names if n.startswith("skip_connection_layers.")}
    # the bookkeeping the Trainer reads: every probed range was stepped by the launch form that holds its complete gradient
    probe, sites = dict(r.log[-2][2]), dict(r.log[-1][2])
    assert set(sites) == set(probe) and set(sites.values()) == {"fold", "writeout"}
    flagged = {_goff(x["dW"]): x["splits"] for _, e in B for x in _items_regions(e)[0] if x["reserved_"] == 1}
    assert flagged and all(sites[o] == ("fold" if sp > 1 else "writeout") for o, sp in flagged.items())


def test_the_dry_run_restores_what_it_patched():
    scenario("tiny2_dropout")
    lib = _lib.load()
    assert type(lib.tulip_gemm_bf16).__name__ == "_FuncPtr" and lib.tulip_gemm_bf16.argtypes == _lib.SIGNATURES["tulip_gemm_bf16"]
    assert torch.cuda.Stream.__module__.startswith("torch") and ops._stream.__module__ == "tulip_amd.ops"



if __name__ == "__main__":
    for nm in sys.argv[1:] or SCENARIOS:
        import time
        t0 = time.time()
        run = scenario(nm)
        print(f"{nm:24s} {len(run.log):6d} {run.dry.sha256()}  ({time.time() - t0:.1f} s)", flush=True)
        if os.environ.get("DRY_RUN_DUMP"):
            with open(os.path.join(os.environ["DRY_RUN_DUMP"], nm + ".log"), "w") as f:
                f.write(run.dry.text())
