#!/usr/bin/env python3
"""Generate tests/golden/g18_clip.npz: the reference's optimizer loop WITH gradient clipping (build container only).

The reference model (imported as make_golden.py imports it) + torch.optim.AdamW with the decay / no-decay groups
(main_lidar_upsampling.py:282-283), 4 optimizer steps at a constant lr on 4 seeded batches, accum_iter = 1, fp32, CPU.  Between
backward() and optimizer.step() every step calls torch.nn.utils.clip_grad_norm_(parameters, clip_grad), exactly as
NativeScalerWithGradNormCount does (util/misc.py:299-300; bf16 needs no GradScaler, so scale / unscale_ are the identity).
Recorded per step: the loss, the returned PRE-clip norm, and the global L2 norms (float64) of all exp_avg and of all exp_avg_sq
behind the step -- and the same four series of an identical run that only reads the norm (util.misc.get_grad_norm_, misc.py:303).

Two conditions make the fixture able to tell clipping from no clipping, asserted here and again by tests/test_clip_cpu.py:
  1. every pre-clip norm exceeds 1.25 x clip_grad (the clip is active at every step, coef < 0.8);
  2. the clipped and the unclipped exp_avg norms differ by more than 5 x the GPU test's tolerance at every step (5 x 2e-2), and
     the exp_avg_sq norms by more than 5 x 4e-2.
clip_grad starts at 1.0 and is halved until both hold.  Only data is written: nothing of the reference's text.

Usage:  python tests/golden/make_golden_clip.py
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from oracle import tulip_oracle as O  # noqa: E402

SEED, BATCH, DATA_SEED0, STEPS, LR = 3, 4, 300, 4, 5e-4
RTOL_M, RTOL_V, MARGIN = 2e-2, 4e-2, 1.25


def moment_norm(opt, key: str) -> float:
    return math.sqrt(sum(float(st[key].double().pow(2).sum()) for st in opt.state.values()))


def run(T, misc, clip_grad):
    """clip_grad None: the norm is only read (misc.py:302-303)."""
    cfg = O.tiny_config(drop_path_rate=0.0)
    m = MG.ref_model(T, cfg, drop_path_rate=0.0)
    m.load_state_dict(O.key_seeded_state_dict(cfg, seed=SEED), strict=True)
    m.train()
    decay = [p for p in m.parameters() if p.ndim > 1]
    nodecay = [p for p in m.parameters() if p.ndim <= 1]
    opt = torch.optim.AdamW([{"params": decay, "weight_decay": 0.01}, {"params": nodecay, "weight_decay": 0.0}],
                            lr=LR, betas=(0.9, 0.95))
    out = {"loss": [], "norm": [], "m_norm": [], "v_norm": []}
    for step in range(STEPS):
        lo, hi = O.synthetic_batch(cfg, BATCH, seed=DATA_SEED0 + step)
        opt.zero_grad()
        _, loss, _ = m(lo, hi)
        loss.backward()
        if clip_grad is not None:
            norm = torch.nn.utils.clip_grad_norm_(m.parameters(), clip_grad)          # misc.py:299-300
        else:
            norm = misc.get_grad_norm_(m.parameters())                                # misc.py:302-303
        opt.step()
        out["loss"].append(loss.item())
        out["norm"].append(float(norm))
        out["m_norm"].append(moment_norm(opt, "exp_avg"))
        out["v_norm"].append(moment_norm(opt, "exp_avg_sq"))
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


def separated(a, b, rtol) -> bool:
    """|a - b| > 5 x the tolerance assert_allclose(a, b, rtol) grants, at every step."""
    return bool(np.all(np.abs(a - b) > 5.0 * rtol * np.abs(b)))


def main():
    T = MG.import_reference()
    six = types.ModuleType("torch._six")          # util/misc.py:21 imports `inf` from a module torch no longer has
    six.inf = math.inf
    sys.modules["torch._six"] = six
    import util.misc as misc
    torch.manual_seed(0)
    plain = run(T, misc, None)
    clip_grad = 1.0
    while True:
        clipped = run(T, misc, clip_grad)
        ok = (bool(np.all(clipped["norm"] > MARGIN * clip_grad)) and separated(plain["m_norm"], clipped["m_norm"], RTOL_M)
              and separated(plain["v_norm"], clipped["v_norm"], RTOL_V))
        if ok:
            break
        clip_grad *= 0.5
        assert clip_grad > 1e-3, "no clip_grad separates the two runs"
    assert np.all(clipped["norm"] > MARGIN * clip_grad)
    assert separated(plain["m_norm"], clipped["m_norm"], RTOL_M) and separated(plain["v_norm"], clipped["v_norm"], RTOL_V)
    assert abs(plain["loss"][0] - clipped["loss"][0]) == 0.0 and abs(plain["norm"][0] - clipped["norm"][0]) <= 1e-6 * plain["norm"][0]
    np.savez_compressed(os.path.join(HERE, "g18_clip.npz"), clip_grad=np.float64(clip_grad),
                        loss=clipped["loss"], grad_norm=clipped["norm"], m_norm=clipped["m_norm"], v_norm=clipped["v_norm"],
                        loss_unclipped=plain["loss"], grad_norm_unclipped=plain["norm"], m_norm_unclipped=plain["m_norm"],
                        v_norm_unclipped=plain["v_norm"], seed=np.int64(SEED), batch=np.int64(BATCH),
                        data_seed0=np.int64(DATA_SEED0), steps=np.int64(STEPS), lr=np.float64(LR),
                        betas=np.array([0.9, 0.95]), weight_decay=np.float64(0.01))
    for k in ("loss", "norm", "m_norm", "v_norm"):
        print(f"{k:7s} clipped {np.round(clipped[k], 6).tolist()}  unclipped {np.round(plain[k], 6).tolist()}")
    print("clip_grad", clip_grad)


if __name__ == "__main__":
    main()
