"""Scenes of every datum defect d = 0 .. 7 on two base scenes (host only: no device, no oracle).

The border of the normal equations has d = popcount(datum_flags) rows, built from the condition rows TX TY TZ RX RY RZ SCALE that
detectRankDefect (BA:836-1042, numbering.detect_rank_defect) leaves free.  The scenes of the rest of the suite have d = 0 (control
points) or d = 6 (no control, one scale bar); the recipes here reach the other six by fixing parameters (helpers.renumber):

  d  recipe                                                        conditions present
  7  no control, no scale bar                                      TX TY TZ RX RY RZ SCALE
  6  no control, scale bar                                         TX TY TZ RX RY RZ
  5  X of points 0 and 5 fixed                                     TY TZ RX RY RZ          (two fixed X: TX and SCALE are gone)
  4  point 3 fixed in X, Y, Z                                      RX RY RZ SCALE
  3  scale bar + point 3 fixed                                     RX RY RZ
  2  scale bar + point 3 fixed + omega of image 1 fixed            RY RZ
  1  point 3 fixed + omega, phi, kappa of image 0 fixed            SCALE
  0  control points (directly observed in X, Y, Z)                 none

A point with a fixed coordinate is no datum point (BA:506), so the centroid and the rows of d = 1 .. 5 run over the others.
With TX absent the TY row is row 0, and so on (BA:523-530): d = 5, 4, 3, 2, 1 number their rows with gaps in the flag order.

The two base scenes: "diag" (6 images, 40 points, 24 per image, radial distortion, ordinary diagonal weights, U = 133 .. 145) and
"block" (8 images, 60 points, 40 per image, the full distortion set, one dense dispersion per image, U = 228 .. 240).  `DEFECT` and
`FLAGS` are literal: what the recipes must give, not what they gave."""
import functools

import numpy as np

from bundle_adjustment_amd import scene
from helpers import renumber

TX, TY, TZ, RX, RY, RZ, SCALE = 1, 2, 4, 8, 16, 32, 64
CONDITIONS = (TX, TY, TZ, RX, RY, RZ, SCALE)        # the order of the border rows (BA:523-530)

# d -> datum_flags
FLAGS = {7: TX | TY | TZ | RX | RY | RZ | SCALE,    # 127
         6: TX | TY | TZ | RX | RY | RZ,            # 63
         5: TY | TZ | RX | RY | RZ,                 # 62
         4: RX | RY | RZ | SCALE,                   # 120
         3: RX | RY | RZ,                           # 56
         2: RY | RZ,                                # 48
         1: SCALE,                                  # 64
         0: 0}
BASES = ("diag", "block")
DEFECTS = (0, 1, 2, 3, 4, 5, 6, 7)
# scene -> rank_defect and scene -> datum_flags, written out
DEFECT = {"diag_d0": 0, "diag_d1": 1, "diag_d2": 2, "diag_d3": 3, "diag_d4": 4, "diag_d5": 5, "diag_d6": 6, "diag_d7": 7,
          "block_d0": 0, "block_d1": 1, "block_d2": 2, "block_d3": 3, "block_d4": 4, "block_d5": 5, "block_d6": 6, "block_d7": 7}
EXPECTED_FLAGS = {"diag_d0": 0, "diag_d1": 64, "diag_d2": 48, "diag_d3": 56, "diag_d4": 120, "diag_d5": 62, "diag_d6": 63, "diag_d7": 127,
                  "block_d0": 0, "block_d1": 64, "block_d2": 48, "block_d3": 56, "block_d4": 120, "block_d5": 62, "block_d6": 63, "block_d7": 127}
NAMES = list(DEFECT)


def _base(base, **kw):
    if base == "diag":
        return scene.make_scene(6, 40, 24, dist=scene.DIST_RADIAL, weights="diag", **kw)
    return scene.make_scene(8, 60, 40, dist=scene.DIST_FULL, weights="block", **kw)


def _fixed_points(fp, components):
    pf = np.zeros((fp.n_points, 3), bool)
    for p, a in components:
        pf[p, a] = True
    return pf


def _fixed_angles(fp, image, angles):
    ef = np.zeros((fp.n_images, 6), bool)
    ef[image, [3 + a for a in angles]] = True
    return ef


POINT3 = [(3, 0), (3, 1), (3, 2)]


def _build(base, d):
    if d == 0:
        return _base(base, n_control=4) if base == "diag" else _base(base, n_control=5, control_dense=True)
    if d == 7:
        return _base(base, n_control=0)
    if d == 6:
        return _base(base, n_control=0, scale_bar=True)
    fp = _base(base, n_control=0, scale_bar=d in (3, 2))
    if d == 5:
        return renumber(fp, point_fixed=_fixed_points(fp, [(0, 0), (5, 0)]))
    if d in (4, 3):
        return renumber(fp, point_fixed=_fixed_points(fp, POINT3))
    if d == 2:
        return renumber(fp, point_fixed=_fixed_points(fp, POINT3), eo_fixed=_fixed_angles(fp, 1, [0]))
    if d == 1:
        return renumber(fp, point_fixed=_fixed_points(fp, POINT3), eo_fixed=_fixed_angles(fp, 0, [0, 1, 2]))
    raise KeyError(d)


@functools.lru_cache(maxsize=None)
def get_scene(name):
    """The scene of `name` ("diag_d7", "block_d4", ...), built once; nobody writes into it."""
    base, d = name.rsplit("_d", 1)
    return _build(base, int(d))


def eo_columns_are_trailing(fp):
    """The exterior orientations own the last 6 I columns in image order: what the engine's EO pre-elimination needs
    (create_plan.h, eo_columns_trailing).  Not so where an angle is fixed (d = 1, 2)."""
    e0 = fp.n_unknowns - 6 * fp.n_images
    return np.array_equal(np.asarray(fp.eo_col).ravel(), np.arange(e0, fp.n_unknowns))
