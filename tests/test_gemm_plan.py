"""CPU: the launch plan of the fp64 GEMM family (gemm_f64_plan, csrc/gemm_f64.h) through jaicov_debug_gemm with plan_only -- no device is
looked for.  gemm_f64() launches from that plan with one switch over the instances, so what is held here is what runs: the instance and
grid of every call shape of tests/gemm_family_cases.py (the shapes tests/test_gpu_gemm_family.py runs), the two size rules on both sides
of their limits, the refusals, and the XCD tile order."""
import numpy as np
import pytest

import gemm_family_cases as gc
from bundle_adjustment_amd import engine

CASES = gc.instance_cases() + gc.krange_cases() + gc.batch_cases() + gc.map_cases() + gc.real_cases()


def plan_of(c, **over):
    c = dict(c, **over)
    L = gc.layout(c)
    kw = gc.hook_kwargs(c, L)
    A = np.zeros(1)
    tmap = None
    if c["map"] is not None:
        tmap = c["map"](c["M"] // 128, c["N"] // 128, c["lower_only"], np.random.default_rng(0))
    rc, plan, Cm = engine.debug_gemm(A=A, B=A if c["same_ab"] else None, tile_map=tmap, plan_only=True, **kw)
    assert Cm is None
    return rc, plan


def test_case_ids_are_unique():
    ids = [c["id"] for c in CASES] + [c["id"] for c, _ in gc.refusal_cases()]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_plan_of_every_call_shape(case):
    rc, plan = plan_of(case)
    assert rc == 0
    assert plan == (gc.HIP_SUCCESS,) + tuple(case["plan"]) + (case["batch"], case["batch2"])


def test_every_instance_is_in_the_table():
    """The eleven instances the launcher can choose for a correct product (tags 2 and 3 are the timing experiments)."""
    seen = {(c["alay"], c["blay"]) + tuple(c["plan"][:3]) for c in gc.instance_cases()}
    want = {(0, 0, 128, 128, 0), (0, 0, 128, 128, 1), (0, 1, 128, 128, 0), (1, 1, 128, 128, 0), (1, 0, 128, 128, 0), (0, 0, 64, 64, 0),
            (0, 0, 64, 64, 1), (0, 0, 32, 32, 0), (0, 0, 64, 128, 0), (0, 0, 32, 128, 0)}
    assert seen == want
    lower64 = {c["plan"][2] for c in gc.instance_cases() if c["lower_only"] and c["plan"][0] == 64}
    rect64 = {c["plan"][2] for c in gc.instance_cases() if not c["lower_only"] and c["plan"][:2] == (64, 64)}
    assert lower64 == {0, 1} and rect64 == {0}          # <64, 64> tag 0 is one kernel with two grids: 10 symbols + the lower grid = 11 rows


@pytest.mark.parametrize("tiles_m,batch,tile", [(1, 479, 64), (1, 480, 128), (1, 63, 32), (1, 64, 64), (3, 21, 32), (4, 16, 64), (3, 160, 128),
                                                (3, 159, 64)])
def test_size_rules_on_both_sides_of_their_limits(tiles_m, batch, tile):
    """small_tiles < 0: the 64-tile below 480 tiles x batch, the 32-tile while tiles x batch x 4 < 256 (252 / 256)."""
    base = gc._case("rule", "kckc", 128 * tiles_m, 128, 48, None)
    want = (tile, tile, tiles_m * (128 // tile) ** 2)              # grid x counts the tiles of ONE batch
    rc, plan = plan_of(base, batch=batch)
    assert rc == 0 and plan[:4] == (0, want[0], want[1], 0) and plan[4] == want[2] and plan[5:] == (batch, 1)
    # in place the same rule picks the row strips
    rc, plan = plan_of(base, batch=batch, c_alias=1)
    tn = 128 if want[0] < 128 else want[1]
    assert rc == 0 and plan[1:3] == (want[0], tn) and plan[4] == want[2] * want[1] // tn
    # other layouts, a restricted k range, the lower grid and small_tiles = 0 never leave the 128-tile
    for over in (dict(blay=1), dict(alay=1), dict(kmode=1), dict(kmode=2), dict(kmode=3), dict(small_tiles=0),
                 dict(lower_only=1, M=128, N=128)):
        rc, plan = plan_of(base, **dict(over, batch=batch))
        assert rc == 0 and plan[1:4] == (128, 128, 0), over


def test_small_tiles_1_is_ignored_where_the_small_instances_cannot_go():
    base = gc._case("rule", "kckc", 256, 256, 256, None, small_tiles=1)
    assert plan_of(base)[1][1:5] == (64, 64, 0, 16)
    assert plan_of(base, lower_only=1)[1][1:5] == (64, 64, 0, 10)
    assert plan_of(base, lower_only=1, tag=1)[1][1:5] == (64, 64, 1, 10)
    for over in (dict(kmode=1), dict(blay=1), dict(lower_only=1, kmode=2), dict(lower_only=1, alay=1, blay=1)):
        assert plan_of(base, **over)[1][1:3] == (128, 128), over
    assert plan_of(base, tag=1)[1][1:4] == (64, 64, 0)            # the rectangular small instances have no tagged twin
    assert plan_of(base, tag=1, small_tiles=0)[1][1:4] == (128, 128, 1)
    assert plan_of(base, tag=1, small_tiles=0, blay=1)[1][1:4] == (128, 128, 0)


@pytest.mark.parametrize("case,status", [pytest.param(c, s, id=c["id"]) for c, s in gc.refusal_cases()])
def test_refusals(case, status):
    rc, plan = plan_of(case)
    assert rc == gc.BAD_ARGUMENT
    if status is None:
        assert plan == (-1,) * 7          # refused before anything is planned
    else:
        assert plan[0] == status and plan[1:5] == (0, 0, 0, 0)


def test_the_refusals_are_no_wider_than_they_say():
    one = gc._case("ok", "kckc", 384, 128, 128, None, ab=1, c_alias=1)
    for small, tile in ((1, (64, 128)), (-1, (32, 128)), (0, (128, 128))):
        rc, plan = plan_of(one, small_tiles=small)
        assert rc == 0 and plan[1:3] == tile
    assert plan_of(one, lower_only=1, M=128)[0] == 0                         # the lower grid with one tile
    assert plan_of(one, ab=(1e-300, 1.0))[0] == 0 and plan_of(one, ab=(-0.0, 1.0))[0] == gc.BAD_ARGUMENT


@pytest.mark.parametrize("T", range(1, 41))
def test_xcd_tile_map(T):
    m = engine.debug_xcd_tile_map(T)
    assert m.shape[0] % 8 == 0 and m.shape[1] == 2
    tiles = [tuple(t) for t in m if t[0] >= 0]
    assert sorted(tiles) == gc.lower_tiles(T)                    # every tile of the lower triangle exactly once
    holes = m[m[:, 0] < 0]
    assert (holes == -1).all() and len(holes) + len(tiles) == len(m)
    lengths = [(m[x::8, 0] >= 0).sum() for x in range(8)]        # workgroup w runs on XCD w % 8
    assert max(lengths) - min(lengths) <= 1 and max(lengths) == len(m) // 8
    for x in range(8):                                           # a list has no holes before its end
        col = m[x::8, 0] >= 0
        assert col[:col.sum()].all()
