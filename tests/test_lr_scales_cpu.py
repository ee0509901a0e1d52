"""CPU: per-parameter learning-rate scales of the fused AdamW -- the grouping rule (tulip_amd.trainer.layer_decay_scales, the
reference's timm recipe restated) and the carrier (ops.pack_lr_groups: the group index in bits 2-7 of the decay-mask bytes, the
scales in a 64-float table).  No kernel is launched."""
import pytest
import torch

from tulip_amd import _lib, ops
from tulip_amd.model import tulip as T
from tulip_amd.trainer import layer_decay_scales

KW = dict(patch_size=(1, 4), in_chans=1, window_size=[2, 8], swin_v2=False, pixel_shuffle=True, circular_padding=True,
          log_transform=True, patch_unmerging=True)          # bench.py's make_model


def base():
    torch.manual_seed(0)
    return T.tulip_base(img_size=(16, 1024), target_img_size=(64, 1024), **KW)


def large():
    torch.manual_seed(0)
    return T.tulip_large(img_size=(16, 2048), target_img_size=(64, 2048), **KW)


def check_rule(model, layer_decay, per_group):
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    sc = layer_decay_scales(model, layer_decay, per_group)
    assert list(sc) == names                                   # named_parameters() order, every trainable name once
    G = -(-len(names) // per_group)
    vals = [sc[n] for n in names]
    for i, v in enumerate(vals):
        assert v == layer_decay ** (G - 1 - i // per_group), (i, v)
    assert all(a <= b for a, b in zip(vals, vals[1:]))         # non-decreasing along the order
    last = len(names) - per_group * (G - 1)
    assert all(v == layer_decay ** (G - 1) for v in vals[:min(per_group, len(names))]) and all(v == 1.0 for v in vals[-last:])
    return names, G, vals


def test_tulip_base_is_18_groups_of_12():
    names, G, vals = check_rule(base(), 0.75, 12)
    assert len(names) == 212 and G == 18 and len(set(vals)) == 18
    assert vals[:12] == [0.75 ** 17] * 12 and vals[12] == 0.75 ** 16
    assert vals[-8:] == [1.0] * 8 and vals[-9] == 0.75


def test_tulip_large_and_other_arguments():
    m = large()
    names, G, vals = check_rule(m, 0.75, 12)
    assert G == -(-len(names) // 12) > 18 and len(set(vals)) == G <= 64
    check_rule(m, 0.9, 7)
    frozen = base()
    first = next(iter(dict(frozen.named_parameters())))
    dict(frozen.named_parameters())[first].requires_grad_(False)
    sc = layer_decay_scales(frozen)
    assert first not in sc and len(sc) == 211 and list(sc.values())[:12] == [0.75 ** 17] * 12
    with pytest.raises(ValueError):
        layer_decay_scales(frozen, 0.75, 0)


def flat_layout(model):
    """FlatParams' layout rule without a device: every tensor starts on a 64-float boundary."""
    off, offset, numel = 0, {}, {}
    for n, p in model.named_parameters():
        offset[n], numel[n] = off, p.numel()
        off = (off + p.numel() + 63) // 64 * 64
    return offset, numel, off


def block_scales(offset, numel, total, scales):
    b = torch.ones(total // 64)
    for n, s in scales.items():
        b[offset[n] // 64:(offset[n] + numel[n] + 63) // 64] = s
    return b


def test_one_name_per_group_is_more_than_64_scales_and_is_refused():
    m = base()
    sc = layer_decay_scales(m, 0.75, 1)
    assert len(set(sc.values())) == 212 > _lib.LR_GROUPS_MAX == 64
    offset, numel, total = flat_layout(m)
    mask = torch.zeros(total // 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="distinct learning-rate scales"):
        ops.pack_lr_groups(mask, block_scales(offset, numel, total, sc))
    # ... and 18 groups fit
    packed, table = ops.pack_lr_groups(mask, block_scales(offset, numel, total, layer_decay_scales(m)))
    assert int((packed >> 2).max()) == 17 and table.shape == (64,) and float(table[0]) == 1.0


def test_mask_byte_packing_on_a_hand_made_layout():
    # six blocks: decay / no decay / skip bits in every combination, three scales, 1.0 not first in the list
    mask = torch.tensor([1, 0, 3, 2, 1, 0], dtype=torch.uint8)
    scale = [0.5, 1.0, 0.0078125, 0.5, 1.0, 0.0078125]
    packed, table = ops.pack_lr_groups(mask, scale)
    assert packed.dtype == torch.uint8 and packed.shape == mask.shape
    assert torch.equal(packed & 3, mask)                                          # bits 0 and 1 preserved
    group = (packed >> _lib.LR_GROUP_SHIFT).tolist()
    assert _lib.LR_GROUP_SHIFT == 2 and max(group) < 64
    assert table.dtype == torch.float32 and table.numel() == 64 and float(table[0]) == 1.0      # entry 0 is 1.0
    assert [float(table[g]) for g in group] == scale                              # the byte's group names the block's scale
    assert group[1] == group[4] == 0                                              # 1.0 is group 0: those bytes are the plain mask
    assert torch.equal(table[3:], torch.ones(61))
    # packing again over bytes that already carry a group replaces it
    again, _ = ops.pack_lr_groups(packed, [1.0] * 6)
    assert torch.equal(again, mask)
    # all ones: the mask itself, a table of ones
    same, ones = ops.pack_lr_groups(mask, [1.0] * 6)
    assert torch.equal(same, mask) and torch.equal(ones, torch.ones(64))
    # the scales are quantised to float32 before they are numbered
    q, t = ops.pack_lr_groups(mask[:2], [0.75 ** 17, 0.75 ** 17 * (1 + 1e-12)])
    assert q[0] >> 2 == q[1] >> 2 == 1 and float(t[1]) == float(torch.tensor(0.75 ** 17, dtype=torch.float32))
    # exactly 64 groups fit, 65 do not
    m64 = torch.zeros(65, dtype=torch.uint8)
    ok, t64 = ops.pack_lr_groups(m64[:64], [1.0] + [1.0 / (k + 2) for k in range(63)])
    assert sorted((ok >> 2).tolist()) == list(range(64))
    with pytest.raises(ValueError):
        ops.pack_lr_groups(m64, [1.0] + [1.0 / (k + 2) for k in range(64)])
    with pytest.raises(ValueError):
        ops.pack_lr_groups(mask, [1.0] * 5)
    with pytest.raises(ValueError):
        ops.pack_lr_groups(mask, [float("nan")] * 6)


def test_adamw_ref_refuses_a_table_without_a_mask():
    with pytest.raises(ValueError):
        ops.adamw_ref(1, 2, 3, 4, 5, 6, decay_mask64=None, lr_scale64=7)
    ref = ops.adamw_ref(1, 2, 3, 4, 5, 6, decay_mask64=8, lr_scale64=7)
    assert ref.lr_scale64 == 7 and ref.decay_mask64 == 8
    assert ops.adamw_ref(1, 2, 3, 4, 5, 6).lr_scale64 is None


def test_a_table_without_a_mask_is_an_argument_error_before_any_launch():
    """The `_s` entry points find the group in the mask bytes: a scale table with decay_mask64 == NULL (or without the
    optimizer buffers) returns TULIP_ERR_ARG from the host code -- nothing is launched, so this runs without a GPU."""
    import ctypes
    lib = _lib.load()
    table = 0x1000                                                     # never dereferenced on the host
    assert lib.tulip_adamw_s(0x1000, 0x1000, 0x1000, 0x1000, None, 64, 0x1000, None, table, 0, None) == -1
    assert lib.tulip_adamw_blocks_s(0x1000, 0x1000, 0x1000, 0x1000, None, 0x1000, 1, 0x1000, None, table, 0, None) == -1
    regions = (_lib.ReduceRegion * 1)()
    assert lib.tulip_reduce_rows_multi_adamw_s(regions, 0, None, table, None) == -1
    ref = ops.adamw_ref(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000)            # no mask
    assert lib.tulip_reduce_rows_multi_adamw_s(regions, 0, ctypes.byref(ref), table, None) == -1
    items = (_lib.WgradItem * 1)()
    assert lib.tulip_wgrad_group_adamw_s(items, 0, regions, 0, None, 0, 1, None, table, None) == -1
    assert lib.tulip_wgrad_group_adamw_s(items, 0, regions, 0, None, 0, 1, ctypes.byref(ref), table, None) == -1
    # nothing to do and nothing wrong: TULIP_OK without a launch
    assert lib.tulip_adamw_s(0x1000, 0x1000, 0x1000, 0x1000, None, 0, 0x1000, None, None, 0, None) == 0
    assert lib.tulip_reduce_rows_multi_adamw_s(regions, 0, None, None, None) == 0
