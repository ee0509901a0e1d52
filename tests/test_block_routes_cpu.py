"""Which kernel family runs each Swin block, read off the dry-run launch logs of tests/block_routes.py:

  1. the route of every block of a fixed list of scenarios equals a literal table (written down from the predicates the route
     function was assembled from: it pins today's policy, quirks included);
  2. the launches a log holds for a block are exactly the family its route names;
  3. the hand-off bits agree between the fused forward and the fused backward launch of one block.

A route is written "<forward family>><backward family>" (deep, wide, c96, seq) followed by its flags: +h the fused launches' fc1_pre
operand carries gelu'(h) (bit 2 of `masked`), +lean the C = 96 pair of launches recomputes qkv / the fc1 pre-activation, +sf / +sb the
wide forward / backward asks for the two-workgroups-per-window form (it runs where tulip_swinw_split_bytes says it exists).
"""
import pytest

from block_routes import SCENARIOS, scenario
from tulip_amd import ops

C96, C96H = "c96>c96", "c96>c96+h"
WIDE, WIDE_NS = "wide>wide+h+sf", "wide>wide+h"
DEEP, SEQ = "deep>deep+h", "seq>seq"


def _base(s0, s1, s2, s3):
    """tulip_base in engine order: encoder stages 0..3, then the decoder's stages 2, 1, 0 (two blocks each)"""
    return (s0, s0, s1, s1, s2, s2, s3, s3, s2, s2, s1, s1, s0, s0)


ROUTES = {
    "base8_train": _base(C96H, WIDE, WIDE, DEEP),
    "base8_infer": _base(C96H, WIDE, WIDE, DEEP),
    # batch 2: C = 384 has 32 windows (< wide_min_windows), C = 768 has 8 (< deep_min_windows)
    "base2_train": _base(C96H, WIDE, SEQ, SEQ),
    # batch 64: C = 768 has 256 windows (> deep_max_windows)
    "base64_train": _base(C96H, WIDE, WIDE, SEQ),
    # tulip_large 16 x 2048, batch 2: C = 384 has 64 windows, C = 768 has 16, C = 1536 has 4
    "large2_train_ow": (C96H, C96H, WIDE, WIDE, SEQ, SEQ, SEQ, SEQ, SEQ, SEQ,
                        SEQ, SEQ, SEQ, SEQ, WIDE, WIDE, C96H, C96H),
    # forward-only fusion off: the fused backward still runs (it evaluates gelu' itself: no +h)
    "base8_fuse_block96_train": _base("seq>c96", WIDE, WIDE, DEEP),
    "base8_fuse_wide_train": _base(C96H, "seq>wide", "seq>wide", DEEP),
    # backward-only fusion off
    "base8_fuse_block96_bwd_train": _base("c96>seq", WIDE, WIDE, DEEP),
    "base8_fuse_wide_bwd_train": _base(C96H, "wide>seq", "wide>seq", DEEP),
    "base8_no96_train": _base(SEQ, WIDE, WIDE, DEEP),
    "base8_fuse_deep_train": _base(C96H, WIDE, WIDE, SEQ),
    "base8_fc1_grad96_train": _base(C96, WIDE, WIDE, DEEP),
    "base8_fc1_grad_wide_train": _base(C96H, "wide>wide", "wide>wide", DEEP),
    "base8_recompute96_train": _base("c96>c96+lean", WIDE, WIDE, DEEP),
    "base8_split_wide_train": _base(C96H, WIDE_NS, WIDE_NS, DEEP),
    "base8_split_wide_bwd_train": _base(C96H, WIDE + "+sb", WIDE + "+sb", DEEP),
    "base8_pair96_train": _base(C96H, WIDE, WIDE, DEEP),
    "base8_infer_no_save_infer": _base(C96H, WIDE, WIDE, DEEP),
    # an inference forward without the hand-off asks for the split form all the same (nothing is saved)
    "base8_fc1_grad_wide_infer": _base(C96H, "wide>wide+sf", "wide>wide+sf", DEEP),
    # element dropout: every block with an active site runs the sequence both ways.  The flags are what the knobs and the geometry
    # say, whatever the family: +h stays on the C = 96 / C = 192 / 384 / 768 blocks (the sequence's attention launches of a C = 96
    # block carry the bit, the kernels ignore it)
    "base8_dropout_train_ow": _base("seq>seq+h", "seq>seq+h", "seq>seq+h", "seq>seq+h"),
    "base8_mc_dropout_infer": _base("seq>seq+h", "seq>seq+h", "seq>seq+h", "seq>seq+h"),
    "base8_dropout_infer": _base(C96H, WIDE, WIDE, DEEP),                   # model.eval(): no site is active
    "tiny2_train": (SEQ,) * 6,
    "tiny2_dropout_train_ow": (SEQ,) * 6,
    "tiny2_attn_dropout_train_ow": (SEQ,) * 6,
    "tiny2_mc_dropout_infer": (SEQ,) * 6,
    "tiny2_win8x8_train": (SEQ,) * 6,
}
CASES = list(ROUTES)
TRAIN = [n for n in CASES if SCENARIOS[n][3] != "infer"]


def route_of(eng, sp, B) -> str:
    """The block's route in the table's notation, from the engine's state as the scenario's last forward left it."""
    if hasattr(eng, "_route"):
        r = eng._route(sp, B)
        fwd, bwd, h, lean, sf, sb = r.fwd, r.bwd, r.hgrad, r.lean, r.split_fwd, r.split_bwd
    else:
        # an engine without the route function: the predicates it was assembled from, combined as the launch sites combined them
        drop = eng._dblock(sp)
        deep = eng._fusable_deep(sp, B) and not drop
        fwd = ("seq" if eng._unfused(sp, B) else "deep" if deep
               else "wide" if (eng.fuse_wide and eng._fusable_wide(sp, B)) else "c96")
        bwd = ("deep" if deep else "seq" if not eng._fused_bwd(sp, B)
               else "c96" if (eng.fuse_block96_bwd and eng._fusable96(sp)) else "wide")
        h, lean = bool(eng._mask_arg(sp, B) & 4), eng._recomp96(sp)
        sf = fwd == "wide" and eng.split_wide and (eng._no_save or eng._hgrad_wide(sp, B))
        sb = bwd == "wide" and eng.split_wide_bwd and eng._hgrad_wide(sp, B)
    return f"{fwd}>{bwd}" + "".join(f for f, on in (("+h", h), ("+lean", lean), ("+sf", sf), ("+sb", sb)) if on)


def _parse(route):
    fam, *flags = route.split("+")
    fwd, bwd = fam.split(">")
    return fwd, bwd, set(flags)


@pytest.mark.parametrize("name", CASES)
def test_route_table(name):
    r = scenario(name)
    got = tuple(route_of(r.eng, sp, r.B) for sp in r.eng.blocks)
    assert got == ROUTES[name]


@pytest.mark.parametrize("name", CASES)
def test_the_predicates_read_the_route(name):
    """what tests and tools ask the engine block by block says what the table says"""
    r = scenario(name)
    eng, B = r.eng, r.B
    for sp, route in zip(eng.blocks, ROUTES[name]):
        fwd, bwd, flags = _parse(route)
        assert eng._unfused(sp, B) == (fwd == "seq"), sp.prefix
        assert eng._fused_bwd(sp, B) == (bwd != "seq"), sp.prefix
        assert bool(eng._mask_arg(sp, B) & 4) == ("h" in flags), sp.prefix
        assert bool(eng._mask_arg(sp) & 4) == eng._hgrad96(sp) == ("h" in flags and sp.C == 96), sp.prefix
        assert eng._hgrad_wide(sp, B) == ("h" in flags and sp.C in (192, 384)), sp.prefix
        assert eng._recomp96(sp) == ("lean" in flags), sp.prefix
        assert (eng._mask_arg(sp, B) & 3) == (int(sp.shift) | (2 if eng.attn_fp8 else 0)), sp.prefix


# ---------------------------------------------------------------------------------------------------------------- reading a log
FWD_SYMS = {"tulip_swind_block_fwd": "deep", "tulip_swinw_block_fwd": "wide", "tulip_swinw_block_fwd_split": "wide",
            "tulip_swin96_block_fwd": "c96", "tulip_swin96_pair_fwd": "c96", "tulip_window_attn_fwd": "seq",
            "tulip_window_attn_fwd_drop": "seq"}
BWD_SYMS = {"tulip_swind_block_bwd": "deep", "tulip_swinw_block_bwd": "wide", "tulip_swinw_block_bwd_split": "wide",
            "tulip_swin96_block_bwd": "c96", "tulip_window_attn_bwd": "seq", "tulip_window_attn_bwd_drop": "seq"}


def _block_launches(r):
    """prefix -> ([(symbol, descriptor or None, entry)] of the forward, ... of the backward); a block is recognised by the buffer
    only its launches write: x_out / attention output in the forward, d_qkv in the backward"""
    out = {sp.prefix: ([], []) for sp in r.eng.blocks}
    for i, e in enumerate(r.log):
        if e[0] != "launch" or (e[1] not in FWD_SYMS and e[1] not in BWD_SYMS):
            continue
        sym, a = e[1], e[3]
        assert e[2] == "chain", e[:3]
        if sym in FWD_SYMS:
            assert i < r.bwd0, sym
            if FWD_SYMS[sym] == "seq":
                owners = [(a[3][0][:-len(".o")], None)]
            else:
                descs = [dict(a[0])] + ([dict(a[1])] if sym == "tulip_swin96_pair_fwd" else [])
                owners = [(d["x_out"][0][:-len(".out")], d) for d in descs]
        else:
            assert i >= r.bwd0, sym
            if BWD_SYMS[sym] == "seq":
                owners = [(a[4][0][:-len(".dqkv")], None)]
            else:
                owners = [(dict(a[0])["d_qkv"][0][:-len(".dqkv")], dict(a[0]))]
        for prefix, d in owners:
            out[prefix][0 if sym in FWD_SYMS else 1].append((sym, d, e))
    return out


@pytest.mark.parametrize("name", CASES)
def test_the_log_holds_the_family_the_route_names(name):
    r = scenario(name)
    eng, B = r.eng, r.B
    launches = _block_launches(r)
    pairs = 0
    for sp, route in zip(eng.blocks, ROUTES[name]):
        fwd, bwd, flags = _parse(route)
        f, b = launches[sp.prefix]
        split = ops.swinw_split_bytes(sp.C, B, sp.H, sp.W) > 0 if sp.C in (192, 384) else False
        want = {"deep": "tulip_swind_block_fwd",
                "wide": "tulip_swinw_block_fwd_split" if ("sf" in flags and split) else "tulip_swinw_block_fwd",
                "c96": "tulip_swin96_block_fwd",
                "seq": "tulip_window_attn_fwd_drop" if eng._dp(sp, 0) else "tulip_window_attn_fwd"}[fwd]
        got = [s for s, _, _ in f]
        if got == ["tulip_swin96_pair_fwd"]:             # one launch for two blocks: both routed c96, the second is the shifted one
            assert fwd == "c96" and eng.pair96, sp.prefix
            e = f[0][2]
            first, second = dict(e[3][0])["x_out"][0], dict(e[3][1])["x_out"][0]
            assert sp.prefix + ".out" in (first, second) and dict(e[3][1])["x_in"] == (first, 0)
            pairs += 1
        else:
            assert got == [want], (sp.prefix, got)
        if r.form == "infer":
            assert b == []
            continue
        want = {"deep": ["tulip_swind_block_bwd"] * 2,
                "wide": ["tulip_swinw_block_bwd_split" if ("sb" in flags and split) else "tulip_swinw_block_bwd"],
                "c96": ["tulip_swin96_block_bwd"],
                "seq": ["tulip_window_attn_bwd_drop" if eng._dp(sp, 0) else "tulip_window_attn_bwd"]}[bwd]
        assert [s for s, _, _ in b] == want, (sp.prefix, [s for s, _, _ in b])
        if bwd == "deep":
            assert [e[3][5] for _, _, e in b] == [3, 12], sp.prefix         # (desc, C, wh, ww, d_norm_out, phases, stamps)
    assert pairs == (4 if name.startswith("base8_pair96") else 0)           # the two C = 96 stages, two blocks each
    if "split_wide_bwd" in name:
        assert any(s == "tulip_swinw_block_bwd_split" for _, b in launches.values() for s, _, _ in b)
    if name in ("base8_train", "base8_infer"):
        assert any(s == "tulip_swinw_block_fwd_split" for f, _ in launches.values() for s, _, _ in f)


@pytest.mark.parametrize("name", TRAIN)
def test_forward_and_backward_agree_on_the_hand_off(name):
    """gelu'(h) in fc1_pre: the bit of the fused forward launch is the bit of the fused backward launch; the C = 96 backward
    gets qkv / fc1_pre exactly where the forward (fused or the sequence, which always writes them) wrote them."""
    r = scenario(name)
    n = 0
    for sp, route in zip(r.eng.blocks, ROUTES[name]):
        fwd, bwd, flags = _parse(route)
        f, b = _block_launches(r)[sp.prefix]
        fd = [d for _, d, _ in f if d is not None and d["x_out"][0] == sp.prefix + ".out"]
        bd = [d for _, d, _ in b if d is not None]
        if fd and bd:
            n += 1
            assert len(fd) == 1
            assert {d["masked"] & 4 for d in bd} == {fd[0]["masked"] & 4} == {4 if "h" in flags else 0}, sp.prefix
            assert {d["masked"] & 3 for d in bd} == {fd[0]["masked"] & 3}, sp.prefix
        if bwd == "c96":
            wrote = {k: (not fd or fd[0][k] is not None) for k in ("qkv", "fc1_pre")}
            assert {k: bd[0][k] is not None for k in wrote} == wrote, sp.prefix
            assert wrote["qkv"] == wrote["fc1_pre"] == ("lean" not in flags), sp.prefix
            # the recomputing backward needs the biases the saved tensors had folded in
            assert all((bd[0][k] is not None) == ("lean" in flags) for k in ("b_qkv", "b_fc1", "norm1_bias", "norm2_bias"))
    assert n or all(_parse(x)[0] == "seq" or _parse(x)[1] == "seq" for x in ROUTES[name])
