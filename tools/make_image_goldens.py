#!/usr/bin/env python3
"""Records the two fixtures of the image tests with matplotlib's public API (needs matplotlib; the tests do not):

  tests/golden/gui_density_cmap_256.npy   the 256 RGB triples of the 2-D viewer's colour map, a LinearSegmentedColormap
                                          from its seven colour names: the table written out in csrc/image.h
  tests/golden/gui_slice_image.npz        a small float32 slice, its obs slice, and the bytes matplotlib produces for them at
                                          the viewer's three colour ranges with its obstacle overlay (alpha 0.2)

    python tools/make_image_goldens.py [--print-table]     (--print-table: the table as C initialiser rows for image.h)
"""
import os
import sys

import numpy as np
from matplotlib.colors import LinearSegmentedColormap, Normalize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STOPS = ["white", "lightgreen", "green", "deepskyblue", "blue", "darkred", "red"]
RANGES = [(0.0, 0.01), (-10.0, 10.0), (-1.0, 1.0)]      # density, v_x, v_y / v_z
ALPHA = 0.2


def colour_map():
    return LinearSegmentedColormap.from_list("density_cmap", STOPS)


def table():
    rgba = colour_map()(np.arange(256))
    return (rgba[:, :3] * 255).astype(np.uint8)


def to_bytes(data, obs, vmin, vmax):
    """colour-map a 2-D float array as the viewer does, then darken the pixels whose obs exceeds one half"""
    rgba = colour_map()(Normalize(vmin=vmin, vmax=vmax, clip=True)(data))
    rgb = (rgba[..., :3] * 255).astype(np.uint8)
    solid = obs > 0.5
    rgb[solid] = (rgb[solid].astype(np.float32) * (1 - ALPHA)).astype(np.uint8)
    return rgb


def slice_case():
    rng = np.random.default_rng(2026)
    rows, cols = 18, 26
    data = np.zeros((rows, cols), dtype=np.float32)
    third = rows // 3
    for band, (vmin, vmax) in enumerate(RANGES):         # each band of rows exercises one of the ranges, beyond both ends
        span = vmax - vmin
        data[band * third:(band + 1) * third] = (vmin - 0.2 * span + 1.4 * span * rng.random((third, cols))).astype(np.float32)
    edges = np.concatenate([np.float32(vmin + (vmax - vmin) * np.arange(0, 257, 8) / 256.0) for vmin, vmax in RANGES])
    data.reshape(-1)[:edges.size] = edges                # values on (or, after rounding to float32, beside) bin edges
    data[-1, :6] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-30]
    obs = (rng.random((rows, cols)) < 0.3).astype(np.float32)
    obs[-1, :3] = 1.0
    return data, obs


def main():
    t = table()
    if "--print-table" in sys.argv[1:]:
        for i in range(0, 256, 8):
            print("    " + " ".join("%d,%d,%d," % tuple(t[j]) for j in range(i, i + 8)))
        return
    os.makedirs(GOLDEN, exist_ok=True)
    np.save(os.path.join(GOLDEN, "gui_density_cmap_256.npy"), t)
    data, obs = slice_case()
    arrays = {"data": data, "obs": obs, "ranges": np.array(RANGES, dtype=np.float64), "alpha": np.float64(ALPHA)}
    for k, (vmin, vmax) in enumerate(RANGES):
        arrays["rgb_%d" % k] = to_bytes(data, obs, vmin, vmax)
    np.savez_compressed(os.path.join(GOLDEN, "gui_slice_image.npz"), **arrays)
    print("wrote", os.path.join(GOLDEN, "gui_density_cmap_256.npy"), "and gui_slice_image.npz")


if __name__ == "__main__":
    main()
