"""The trimesh terrain query (gs_terrain.h, tables from gs_terrain_build.hip) held to the float64 oracle on the CPU:
the host backend compiles the same gs_terrain.h as every kernel form, so every cull is checked here without a GPU
(tests/terrain_cases.py states the meshes, the queries and the rule; test_terrain_query_gpu.py runs the kernel).

Mutations, each built into a copy of the library and run on the host backend; the tests that fail:
  * extent bytes written as 0 (gs_terrain_build.hip)           test_host_backend_query_meets_the_rule[rough, walls,
                                                               far, fine], test_terrain_query_on_jittered_mesh_...
  * the box cull's dz from the cell top, not its bottom        ..._meets_the_rule[all five], the stair riser test
  * reach = thr instead of max(thr, r + TERRAIN_BACK)          ..._meets_the_rule[rough, walls, far, fine]
  * row-end trimming off by one (ja += 2)                      ..._meets_the_rule[rough, walls, far, fine]
  * the four-corner block shortcut for three-block spans too   test_plateau_between_the_corner_blocks_is_seen (the
                                                               random families did not see it: a centre's height
                                                               follows the ground under it, and some corner block
                                                               nearly always reaches as high)
  * the centre cell visited in (i, j) order, not first         the exact tie in test_sphere_in_a_stair_riser_...,
                                                               ..._meets_the_rule[fine]
  * ib = i1 - 3 without the clamp to i0                        none, and none can by its outputs: where the clamp
        acts (i1 - 3 < i0) the two squares of row i0 cover the whole range, so the other two only add reasons to go
        on, whatever they hold; what the clamp prevents is a read before the table (rows -1 to -3 at the low edge)
  * TERRAIN_DOWN_NZ dropped from the host-side normal          none: an equivalent mutant, triangle_n repeats the
        test on the stored normal (the flag only spares the kernels the degenerate case's division)
"""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import terrain_cases as TC

TAG = "terrain-parity"
UNDECIDED_MAX = 0.005  # share of a family's queries
KIND_MIN = 0.05        # each contact kind, of the found queries (rough, walls, fine)
CLASS_MIN = 0.02       # each range class, of the family's queries
EMPTY_MIN = 50         # "no cell in range" queries per family


@pytest.mark.parametrize("fam", TC.FAMILIES)
def test_query_sets_cover_what_they_claim(fam):
    """The conditions on the inputs, from the oracle and the index arithmetic alone: few undecided queries, every
    contact kind and every range class of may_contact present in numbers."""
    n = TC.counts(fam)
    print(f"[{TAG}] {fam} counts: {n}")
    assert n["queries"] == TC.QUERIES
    assert n["undecided"] <= UNDECIDED_MAX * n["queries"], n
    if fam in ("rough", "walls", "fine"):
        for kind in TC.KINDS.values():
            assert n[kind] >= KIND_MIN * n["found"], (kind, n)
    for cl in TC.RANGE_CLASSES:
        if cl == "empty":
            assert n[cl] >= EMPTY_MIN, n
        else:
            assert n[cl] >= CLASS_MIN * n["queries"], (cl, n)
    for m in TC.family(fam):  # inputs are float32 values, shared bit for bit by every implementation
        assert m["c"].dtype == np.float32 and m["r"].dtype == np.float32
        assert set(np.unique(m["r"]).tolist()) <= {float(np.float32(r)) for r in TC.RADII}


@pytest.mark.parametrize("fam", TC.FAMILIES)
def test_float32_oracle_meets_the_rule(fam):
    """The float32 build of the oracle source under the rule it defines: its found flags match on every decided
    query (the decided set is not vacuous: float rounding alone flips nothing in it), and its errors are the
    err_f32 of the records."""
    seen, fails = {}, []
    TC.judge(TAG, seen, fails, fam, [m["ref32"] for m in TC.family(fam)])
    assert not fails, fails
    assert seen, "no decided query found by both"


@pytest.mark.parametrize("fam", TC.FAMILIES)
def test_host_backend_query_meets_the_rule(fam):
    """gs_debug_terrain_query on the host backend: every decided query's found flag, and separation and normal
    within the bar, per family and field."""
    seen, fails = {}, []
    TC.judge(TAG, seen, fails, fam, [TC.host_query(m["ter"], m["c"], m["r"]) for m in TC.family(fam)])
    print(f"[{TAG}] {fam} host backend (err_kernel/err_f32, err_kernel/bar): {seen}")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------- mesh refusals
def _grid(rows, cols, hs=0.1):
    from isaacgymenv_amd.isaacgym import terrain_utils
    return terrain_utils.convert_heightfield_to_trimesh(np.zeros((rows, cols), np.int16), hs, 0.005, None)


def _broken_meshes():
    """(cause in the message, vertices, num_vertices, triangles, num_triangles): one minimal mesh per refusal of
    terrain_build, in its order."""
    v22, t22 = _grid(2, 2)
    yield "empty mesh", v22, 4, t22, 0
    t = t22.copy()
    t[0] = (1, 3, 0)
    yield "first triangle", v22, 4, t, 2
    v32, t32 = _grid(3, 2)
    yield "triangle count", v32, 6, t32[:2], 2
    # a 2-column grid of 2^24 + 1 rows: refused on its shape alone, before any but the first triangle is read
    # (zero pages: neither array is ever touched beyond its first triangle)
    rows = (1 << 24) + 1
    big_v, big_t = np.zeros((2 * rows, 3), np.float32), np.zeros((2 * (rows - 1), 3), np.uint32)
    big_t[0] = (0, 3, 1)
    yield "grid too large", big_v, 2 * rows, big_t, 2 * (rows - 1)
    v23, t23 = _grid(2, 3)
    t = t23.copy()
    t[2] = t[2][[1, 2, 0]]
    yield "grid layout", v23, 6, t, 4
    v = v22.copy()
    v[:, 0] = 0.0
    yield "grid spacing", v, 4, t22, 2
    v33, t33 = _grid(3, 3)
    v = v33.copy()
    v[4, 0] += 0.15
    yield "more than one cell", v, 9, t33, 8


def test_add_triangle_mesh_refuses_each_broken_mesh_and_then_accepts_a_valid_one():
    from isaacgymenv_amd.isaacgym import _lib, gymapi
    L = _lib.lib()
    sp = gymapi.SimParams()
    sp.use_gpu_pipeline = False
    sp.physx.use_gpu = False
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    assert sim is not None and sim.host
    tp = (C.c_double * 3)(0.5, -0.25, 0.1)
    causes = []
    for cause, v, nv, t, nt in _broken_meshes():
        v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.uint32)
        rc = L.gs_sim_add_triangle_mesh(sim.handle, v.ctypes.data, nv, t.ctypes.data, nt, tp, 1.0, 1.0, 0.0)
        msg = L.gs_last_error().decode()
        assert rc != 0, cause
        assert cause in msg and "gs_sim_add_triangle_mesh" in msg, (cause, msg)
        causes.append(cause)
    assert len(causes) == 7
    v, t = _grid(3, 4)
    assert L.gs_sim_add_triangle_mesh(sim.handle, v.ctypes.data, 12, t.ctypes.data, 12, tp, 1.0, 1.0, 0.0) == 0, \
        L.gs_last_error().decode()
    # and one mesh per sim: a second valid mesh is refused by the sim, not by the build
    assert L.gs_sim_add_triangle_mesh(sim.handle, v.ctypes.data, 12, t.ctypes.data, 12, tp, 1.0, 1.0, 0.0) != 0
    assert "one triangle mesh per sim" in L.gs_last_error().decode()


# ------------------------------------------------------------------------------- planes: ties between coplanar faces
PLANE_R = 0.06
# heights h of the centre above the plane along its normal: beyond the contact offset, within it, touching,
# penetrating, behind the plane, and behind it by more than r + TERRAIN_BACK
PLANE_H = (0.09, 0.075, 0.06, 0.01, -0.03, -0.12, -0.17)


def _plane_points(ter, rows, cols):
    """Surface points of a planar grid mesh: vertices, cell-border midpoints, diagonal midpoints and quarter points,
    and interior points, all inside the outer cells' ring, as float64 [m, 3] from the float32 vertices."""
    g = ter["oracle"]["vertices"].reshape(rows, cols, 3).astype(np.float64)
    a, b, c, d = g[1:-2, 1:-2], g[1:-2, 2:-1], g[2:-1, 1:-2], g[2:-1, 2:-1]  # v00, v01, v10, v11 of interior cells
    pts = [a, 0.5 * (a + b), 0.5 * (a + c), 0.5 * (a + d), 0.75 * a + 0.25 * d, 0.5 * a + 0.25 * b + 0.25 * d,
           0.5 * a + 0.25 * c + 0.25 * d, 0.125 * a + 0.5 * b + 0.375 * d]
    return np.concatenate([p.reshape(-1, 3) for p in pts])


@pytest.mark.parametrize("slope", [(0, 0), (3, -2)], ids=["flat", "inclined"])
def test_plane_mesh_gives_the_analytic_contact_on_every_tie(slope):
    """A flat and an inclined planar mesh: wherever the centre is over it -- on a vertex, a cell border, the diagonal
    or inside a triangle -- in front of the plane or behind it, the contact is the plane's: separation h - r along
    the plane's normal.  On borders and diagonals two to six coplanar triangles tie; the answer may not depend on
    which wins, nor on whether the closest point counts as interior or as on the edge.
    Bounds: coordinates below 4 m carry float32 roundings of 2^-22 m = 2.4e-7 m; the separation is a sum of about
    8 such terms (vertex, centre, the dot product), so 2e-6 m; a face normal of cells of 0.1 m from vertices rounded
    by 2.4e-7 m turns by up to 2.4e-6 per axis; where the contact comes as an edge contact, its normal (c - q)/|c - q|
    divides two such roundings by the smallest distance used, 0.01 m: 4.8e-5, so 5e-5."""
    rows, cols, hs, vs = 9, 8, 0.1, 0.005
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    hf = (slope[0] * i + slope[1] * j + 20).astype(np.int16)
    ter = H.terrain_from_heights(hf, hs=hs, vs=vs, slope_threshold=None, shift=(-1.5, 2.25, 0.3))
    nrm = np.array([-slope[0] * vs / hs, -slope[1] * vs / hs, 1.0])
    nrm /= np.linalg.norm(nrm)
    q = _plane_points(ter, rows, cols)
    c = np.concatenate([q + h * nrm for h in PLANE_H])
    hh = np.repeat(PLANE_H, q.shape[0])
    c32 = c.astype(np.float32)
    # the height of the float32 centre over the plane through vertex (0, 0), in float64
    h32 = (c32.astype(np.float64) - ter["oracle"]["vertices"][0].astype(np.float64)) @ nrm
    out = TC.host_query(ter, c32, np.full(c.shape[0], PLANE_R, np.float32)).astype(np.float64)
    want = (h32 < PLANE_R + TC.PARAMS["contact_offset"] - 1e-4) & (h32 > -(PLANE_R + 0.1) + 1e-4)
    assert want.sum() == ((hh < 0.08) & (hh > -0.16)).sum() == 5 * q.shape[0]
    bad = np.nonzero((out[:, 0] > 0.5) != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), c32[bad[:8]].tolist(), hh[bad[:8]].tolist())
    f = want
    assert np.abs(out[f, 1] - (h32[f] - PLANE_R)).max() <= 2e-6, np.abs(out[f, 1] - (h32[f] - PLANE_R)).max()
    assert np.abs(out[f, 2:5] - nrm).max() <= 5e-5, np.abs(out[f, 2:5] - nrm).max()


# --------------------------------------------------------------------------------------------------- stair riser
def test_sphere_in_a_stair_riser_is_pushed_out_of_the_riser():
    """The header's rule on a stair: heights 0 for rows 0-4 and 0.2 m from row 5 on; the slope correction moves row 4
    to x = 0.5, so the riser is the plane x = 0.5 facing -x between z = 0 and z = 0.2, the tread z = 0.2 for x >= 0.5.
    Sphere radius 0.05, contact offset 0.02, y mid-cell; expectations computed by hand:
      (0.52, 0.10): 0.02 behind the riser, 0.10 below the tread: the riser is nearer -> (-1, 0, 0), sep -0.02 - 0.05
      (0.58, 0.17): 0.08 behind the riser, 0.03 below the tread: the tread is nearer -> (0, 0, 1), sep -0.03 - 0.05
      (0.46, 0.10): 0.04 in front of the riser, the ground 0.10 below (beyond 0.07) -> (-1, 0, 0), sep 0.04 - 0.05
      (0.47, 0.23): in front of and above the tread's edge (0.5, 0.2): distance 0.03 sqrt 2 -> the edge contact
                    (-1, 0, 1) / sqrt 2, sep 0.03 sqrt 2 - 0.05, whichever of the riser and the tread gives it
      (0.4375, 0.0625): 0.0625 in front of the riser and 0.0625 above the ground, both exact in float32: an exact tie
                    of two faces, which the visiting order decides: the cell under the centre first, and at y = 0.585
                    that is the riser's (row 4 is collapsed onto x = 0.5 and, by the diagonal rule, sheared one cell
                    along y: cell (4, 5) covers y from 0.6 - z/2 to 0.7 - z/2) -> (-1, 0, 0), sep 0.0125; in plain
                    (i, j) order a ground cell of row 3 (stretched to x = 0.5) would win with (0, 0, 1)
    Bounds: float32 coordinates below 1 m (6e-8 m roundings), a handful of terms: 5e-7 m; a face normal 1e-6; the
    edge normal divides roundings of 6e-8 m by a distance of 0.042 m: 1e-5."""
    hf = np.zeros((10, 10), np.int16)
    hf[5:] = 40
    ter = H.terrain_from_heights(hf)
    g = ter["oracle"]["vertices"].reshape(10, 10, 3)
    assert np.all(g[4, :, 0] == np.float32(0.5)) and np.all(g[4, :, 2] == 0) and np.all(g[5, :, 0] == g[4, :, 0])
    y, s = 0.537, np.sqrt(0.5)
    c = np.array([[0.52, y, 0.10], [0.58, y, 0.17], [0.46, y, 0.10], [0.47, y, 0.23], [0.4375, 0.585, 0.0625]],
                 np.float32)
    want = np.array([[1, -0.07, -1, 0, 0], [1, -0.08, 0, 0, 1], [1, -0.01, -1, 0, 0],
                     [1, 0.03 * np.sqrt(2) - 0.05, -s, 0, s], [1, 0.0125, -1, 0, 0]])
    out = TC.host_query(ter, c, np.full(5, 0.05, np.float32)).astype(np.float64)
    assert np.array_equal(out[:, 0], want[:, 0]), out
    assert np.abs(out[:, 1] - want[:, 1]).max() <= 5e-7, out
    assert np.abs(out[[0, 1, 2, 4], 2:5] - want[[0, 1, 2, 4], 2:5]).max() <= 1e-6, out
    assert np.abs(out[3, 2:5] - want[3, 2:5]).max() <= 1e-5, out


# ------------------------------------------------------------------------------------ the block cull's shortcut
def test_plateau_between_the_corner_blocks_is_seen():
    """may_contact's four-corner shortcut holds for ranges of at most two 8 x 8 blocks a side; a range of three has
    blocks between the corners.  A plateau 0.3 m high on cells 10-13 of a level 30 x 30 grid lies inside block (1, 1);
    a sphere of radius 0.6 resting 0.01 above it reaches cells 4-20, blocks 0-2, whose four corner blocks are level
    ground 0.29 below the sphere's reach: only the block loop sees the plateau.  Beside it a sphere of radius 0.35
    whose range, cells 8-19, spans two blocks a side (the shortcut itself).  Expected: the plateau's face, separation
    0.01 (coordinates below 2 m: 1.2e-7 m roundings, 1e-6 for the sum)."""
    hf = np.zeros((30, 30), np.int16)
    hf[10:15, 10:15] = 60
    ter = H.terrain_from_heights(hf)
    c = np.array([[1.2, 1.2, 0.3 + 0.6 + 0.01], [1.38, 1.38, 0.3 + 0.35 + 0.01]], np.float32)
    r = np.array([0.6, 0.35], np.float32)
    cl = TC.range_classes(ter, c, r)
    assert cl["three_block"][0] and cl["two_block"][1]
    out = TC.host_query(ter, c, r).astype(np.float64)
    assert np.array_equal(out[:, 0], [1, 1]), out
    assert np.abs(out[:, 1] - 0.01).max() <= 1e-6 and np.abs(out[:, 2:5] - [0, 0, 1]).max() <= 1e-6, out


def test_the_two_queries_that_found_bugs_stay_in_the_sets():
    """Regressions kept inside the families (test_host_backend_query_meets_the_rule holds them): `far` query 5072, a
    centre 0.064 m behind a level face with its x on a grid line (no surface found before on_rim), and `walls` query
    9084, a centre 0.11 m behind an overhanging face and above its cell's top by more than r + contact_offset (culled
    before low_reach).  Both must stay decided, found, and face contacts from behind."""
    for name, k, nz in (("far", 5072, 1.0), ("walls", 9084, -0.408)):
        m = TC.member(name)
        assert m["decided"][k] and m["ref64"][k, 0] == 1 and m["ref64"][k, 5] == 2, (name, m["ref64"][k])
        assert abs(m["ref64"][k, 4] - nz) < 1e-3
        out = TC.host_query(m["ter"], m["c"][k:k + 1], m["r"][k:k + 1])[0]
        assert out[0] == 1 and abs(out[1] - m["ref64"][k, 1]) < 1e-6, out
