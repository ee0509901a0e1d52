#!/usr/bin/env python3
"""Generate tests/golden/g20_edge.npz: the reference's two edge filters on seeded inputs (build container only).

The reference model module imports util/filter.py (tulip.py:9) and never uses it: HorizontalEdgeDetectionCNN and
VerticalEdgeDetectionCNN, each a fixed 3x3 Sobel filter in a Conv2d(1, 1, 3, padding=1, bias=False).  They are the two responses the
edge term of TULIP(loss_edge_weight=...) is built from (tulip_amd/loss.py, edge_responses).  For seeded float64 arrays d of the
shapes below -- one pixel, one row, the 3x3 plane that is all border, adjacent planes and samples with an odd width, and a plane
larger than nothing in particular -- every (b, c) plane is passed through both modules (cast to float64) on its own, and recorded
are d and the two outputs.  The values of d are multiples of 2^-10 below 8 in magnitude, so every response is exact in float64
whatever order the convolution sums in, and the test can ask for equality.

Only arrays are written: nothing of the reference's text.

Usage:  python tests/golden/make_golden_edge.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

SHAPES = ((1, 1, 1, 1), (1, 1, 1, 5), (1, 1, 3, 3), (2, 3, 5, 7), (1, 2, 17, 65))
SEED = 2001


def main():
    MG.import_reference()
    import util.filter as F
    h, v = F.HorizontalEdgeDetectionCNN().double(), F.VerticalEdgeDetectionCNN().double()
    out = {"n_cases": np.int64(len(SHAPES)), "seed": np.int64(SEED)}
    rng = np.random.default_rng(SEED)
    for k, shape in enumerate(SHAPES):
        d = np.round(np.clip(rng.standard_normal(shape) * 2.0, -7.9, 7.9) * 1024.0) / 1024.0
        planes = torch.from_numpy(d).reshape(-1, 1, *shape[-2:])
        with torch.no_grad():
            e_h, e_v = h(planes).reshape(shape).numpy(), v(planes).reshape(shape).numpy()
        assert e_h.dtype == np.float64 and e_h.shape == shape == e_v.shape
        out.update({f"d{k}": d, f"e_h{k}": e_h, f"e_v{k}": e_v})
        print(f"case {k} {shape}: max|e_h| {np.abs(e_h).max():.6f}  max|e_v| {np.abs(e_v).max():.6f}")
    np.savez_compressed(os.path.join(HERE, "g20_edge.npz"), **out)


if __name__ == "__main__":
    main()
