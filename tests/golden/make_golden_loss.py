#!/usr/bin/env python3
"""Generate tests/golden/g19_loss.npz: the reference's berHu function on seeded inputs (build container only).

The reference model module imports `inverse_huber_loss` (tulip.py:11; util/evaluation.py:177-180) and never calls it; it is the
definition TULIP(loss="berhu") follows (tulip_amd/loss.py).  For two seeded float32 (pred, target) pairs the function is evaluated
in float64 on the float32 values, and recorded are: the elementwise values it returns, their mean (how forward_loss would use
them), C = 0.2 max|pred - target|, the autograd gradient of the mean with respect to pred (C is read with .item() there, so nothing
flows through it), and the share of elements at or above C.

Two conditions make the fixture able to tell the branches and the losses apart, asserted here and again by tests/test_loss_cpu.py:
  1. the share of elements at or above C lies in [0.1, 0.9] for each case (both branches of the function are exercised);
  2. the berHu gradient differs from the L1 gradient sign(d) / n by more than 10 % in relative L2.
Only data is written: nothing of the reference's text.

Usage:  python tests/golden/make_golden_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

CASES = (((2, 1, 16, 64), 1901), ((2, 2, 8, 32), 1902))
SHARE_LO, SHARE_HI, SEPARATION = 0.1, 0.9, 0.10


def rel_l2(a, b) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    T = MG.import_reference()
    out = {"n_cases": np.int64(len(CASES)), "share_lo": np.float64(SHARE_LO), "share_hi": np.float64(SHARE_HI),
           "separation": np.float64(SEPARATION)}
    for k, (shape, seed) in enumerate(CASES):
        gen = torch.Generator().manual_seed(seed)
        pred32 = torch.randn(shape, generator=gen, dtype=torch.float32)
        target32 = torch.randn(shape, generator=gen, dtype=torch.float32)
        pred = pred32.double().requires_grad_(True)
        target = target32.double()
        values = T.inverse_huber_loss(pred, target)
        mean = values.mean()
        mean.backward()
        d = (pred.detach() - target).numpy()
        c = 0.2 * np.abs(d).max()
        share = float(np.mean(np.abs(d) >= c))
        grad = pred.grad.numpy()
        l1_grad = np.sign(d) / d.size
        sep = rel_l2(grad, l1_grad)
        assert SHARE_LO <= share <= SHARE_HI, (k, share)
        assert sep > SEPARATION, (k, sep)
        out.update({f"pred{k}": pred32.numpy(), f"target{k}": target32.numpy(), f"values{k}": values.detach().numpy(),
                    f"mean{k}": np.float64(mean.item()), f"c{k}": np.float64(c), f"grad{k}": grad,
                    f"share{k}": np.float64(share), f"seed{k}": np.int64(seed)})
        print(f"case {k} {shape}: mean {mean.item():.9f}  C {c:.9f}  share(|d| >= C) {share:.3f}  rel_l2(berhu grad, l1 grad) {sep:.3f}")
    np.savez_compressed(os.path.join(HERE, "g19_loss.npz"), **out)


if __name__ == "__main__":
    main()
