"""Meshes, queries and the judging rule of the trimesh terrain query tests (gs_terrain.h, gs_terrain_build.hip;
test_terrain_query_cpu.py asserts what is claimed here, test_terrain_query_gpu.py relies on it).

Families (cells of 0.1 m unless said; every mesh carries a non-zero shift):
  rough   H.rough_terrain(seed=5, rows=45, cols=38): stairs, obstacles, a random field; 44 x 37 cells, so partial
          8 x 8 blocks and clipped 4 x 4 squares on both axes
  walls   random heights in steps of 4 counts inside a level rim, through the slope correction at threshold 0.75
          (moved vertices, vertical walls, inverted, degenerate and folded triangles); and the same heights without
          the correction but jittered off their grid points (+-0.2 cell, 2 % by 0.75 cell, the outer lines kept on
          the grid): half of the queries each
  tiny    grids of 2 x 2, 2 x 3, 3 x 10 and 10 x 18 vertices (gentle random heights; 15 / 15 / 20 / 50 % of the queries)
  far     the rough mesh shifted by (150, -170, 3)
  fine    the rough heights on cells of 0.025 m (walls from the same steps as on 0.1 m cells): a foot-sized radius
          spans more than 8 and more than 16 cells

Queries: QUERIES per family; centres uniform over the footprint widened by MARGIN on every side (on, across and
beyond every edge and corner), z = the nearest vertex's height + U(-0.15, 0.2) (+ r - 0.1 for radii above 0.3), radii
from RADII; centres and radii rounded to float32 first, so that every implementation sees the same inputs.

The rule (judge): against OracleSim.terrain_query_kind in float64,
  * a query is DECIDED when the float64 oracle gives the same found flag, and a separation within 4 delta, at all
    eight perturbed inputs (centre +-delta along x, y, z; radius +-delta); delta = 2e-5 m, for `far` 1.5e-4 m
    (8 ulp of its largest coordinate);
  * every decided query must match the oracle's found flag exactly;
  * on decided queries found by both, separation and normal are held to H.field_check's bar
    (max|got - ref64| <= 4 max|ref32 - ref64| + 4 2^-23 max|ref64|, ref32 = the float32 build of the oracle over the
    same set), face contacts and edge / vertex contacts as separate fields (an edge normal is (c - q)/|c - q|: its
    error grows as the distance shrinks);
  * undecided queries are only counted.
One condition more makes a query decided: the winning surface is nearer than every surface with another answer by
more than delta / 16 (OracleSim.terrain_query_kind's margin; for `far` half an ulp of its largest coordinate).  The
slope correction folds cells onto themselves: two
coincident faces with opposite normals, which tie exactly for every centre near them and under every perturbation; the
float32 oracle picks the other one of the pair (a normal off by 2, a separation by twice the depth), and one such
query in a family would make 4 max|ref32 - ref64| a bar that holds nothing.
"""
import functools

import numpy as np

from oracle.oracle import OracleSim
from tests import helpers as H

QUERIES = 20000
MARGIN = 0.6
RADII = (0.02, 0.06, 0.1, 0.35, 0.6)
DELTA = 2e-5
DELTA_FAR = 1.5e-4
TIE_MARGIN_DIV = 16.0  # a winner nearer by less than delta / 16 (half an ulp of the largest coordinate) is a tie
FAMILIES = ("rough", "walls", "tiny", "far", "fine")
KINDS = {1: "face_front", 2: "face_behind", 3: "edge_vertex"}
RANGE_CLASSES = ("narrow", "two_block", "three_block", "clamp_ilo", "clamp_ihi", "clamp_jlo", "clamp_jhi",
                 "centre_off", "empty")
PARAMS = dict(H.ANYMAL_PARAMS, has_ground=0)
TERRAIN_BACK = np.float32(0.1)
TERRAIN_BLK = 8
# members of each family: (name, share of the family's queries)
MEMBERS = {"rough": (("rough", 1.0),), "walls": (("walls", 0.5), ("walls_jitter", 0.5)),
           "tiny": (("tiny_2x2", 0.15), ("tiny_2x3", 0.15), ("tiny_3x10", 0.2), ("tiny_10x18", 0.5)),
           "far": (("far", 1.0),), "fine": (("fine", 1.0),)}
ROUGH = dict(seed=5, rows=45, cols=38)
WALLS = dict(seed=9, rows=30, cols=35, shift=(1.3, -0.7, 0.2))
FAR_SHIFT = (150.0, -170.0, 3.0)


def _walls(jitter):
    from isaacgymenv_amd.isaacgym import terrain_utils
    rng = np.random.RandomState(WALLS["seed"])
    rows, cols, hs = WALLS["rows"], WALLS["cols"], 0.1
    hf = (rng.randint(-12, 12, (rows, cols)) * 4).astype(np.int16)
    # a level rim two samples wide: the outer lines stay on the grid (terrain_build takes the grid's origin and
    # spacing from them, as a map's border gives them)
    hf[:2], hf[-2:], hf[:, :2], hf[:, -2:] = 0, 0, 0, 0
    # (the jittered variant without the slope correction: a corrected vertex is already a whole cell off its point)
    v, t = terrain_utils.convert_heightfield_to_trimesh(hf, hs, 0.005, None if jitter else 0.75)
    if jitter:
        v = v.astype(np.float64)
        v[:, :2] += rng.uniform(-0.2, 0.2, (v.shape[0], 2)) * hs
        whole = rng.rand(v.shape[0]) < 0.02
        v[whole, 0] += np.where(rng.rand(whole.sum()) < 0.5, -1.0, 1.0) * hs * 0.75
        grid = v.reshape(rows, cols, 3)
        # the outer rows' x and columns' y on their grid lines: they define the grid origin and spacing
        grid[0, :, 0], grid[-1, :, 0] = 0.0, (rows - 1) * hs
        grid[:, 0, 1], grid[:, -1, 1] = 0.0, (cols - 1) * hs
        v = v.astype(np.float32)
    return H.mesh_terrain(v, t, rows, cols, hs, shift=WALLS["shift"])


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The terrain dict (H.mesh_terrain) of one family member."""
    if name == "rough":
        return H.rough_terrain(**ROUGH)
    if name == "far":
        return H.terrain_from_heights(H.rough_heights(**ROUGH), shift=FAR_SHIFT)
    if name == "fine":
        # (slope threshold 2: steps above 10 counts make walls, the same steps as on cells of 0.1 m)
        return H.terrain_from_heights(H.rough_heights(**ROUGH), hs=0.025, slope_threshold=2.0,
                                      shift=(-0.55, 0.45, -0.1))
    if name in ("walls", "walls_jitter"):
        return _walls(name == "walls_jitter")
    rows, cols = (int(x) for x in name[len("tiny_"):].split("x"))
    rng = np.random.RandomState(100 * rows + cols)
    # steps of at most 8 counts stay below the slope correction's 10: the tiny grids are about the index arithmetic
    return H.terrain_from_heights(rng.randint(-4, 5, (rows, cols)).astype(np.int16), shift=(0.35, -1.15, 0.05))


def queries(ter, n, seed):
    """(centres [n, 3], radii [n]) in float32 around and beyond the mesh of `ter`."""
    o = ter["oracle"]
    rows, cols, hs = o["rows"], o["cols"], o["hs"]
    rng = np.random.RandomState(seed)
    c = np.zeros((n, 3))
    c[:, 0] = rng.uniform(o["x0"] - MARGIN, o["x0"] + (rows - 1) * hs + MARGIN, n)
    c[:, 1] = rng.uniform(o["y0"] - MARGIN, o["y0"] + (cols - 1) * hs + MARGIN, n)
    gi = np.clip(np.round((c[:, 0] - o["x0"]) / hs).astype(int), 0, rows - 1)
    gj = np.clip(np.round((c[:, 1] - o["y0"]) / hs).astype(int), 0, cols - 1)
    r = rng.choice(RADII, n)
    c[:, 2] = o["vertices"].reshape(rows, cols, 3)[gi, gj, 2] + rng.uniform(-0.15, 0.2, n) + \
        np.where(r > 0.3, r - 0.1, 0.0)
    return c.astype(np.float32), r.astype(np.float32)


def range_classes(ter, c, r, offset=PARAMS["contact_offset"]):
    """{class: [n] bool}: gs_terrain::may_contact's index arithmetic restated in float32 from the inputs (the grid
    origin and spacing as terrain_build derives them: float32 of the double values)."""
    o = ter["oracle"]
    f = np.float32
    x0, y0, inv_hs = f(o["x0"]), f(o["y0"]), f(1.0 / o["hs"])
    rows, cols = o["rows"], o["cols"]
    thr = r + f(offset)
    reach = np.maximum(thr, r + TERRAIN_BACK)
    gx, gy, gt = (c[:, 0] - x0) * inv_hs, (c[:, 1] - y0) * inv_hs, reach * inv_hs
    ia, ib = np.floor(gx - gt).astype(np.int64) - 1, np.floor(gx + gt).astype(np.int64) + 1
    ja, jb = np.floor(gy - gt).astype(np.int64) - 1, np.floor(gy + gt).astype(np.int64) + 1
    i0, i1, j0, j1 = np.maximum(ia, 0), np.minimum(ib, rows - 2), np.maximum(ja, 0), np.minimum(jb, cols - 2)
    empty = (i0 > i1) | (j0 > j1)
    narrow = ~empty & (i1 - i0 <= 7) & (j1 - j0 <= 7)
    two = (i1 // TERRAIN_BLK - i0 // TERRAIN_BLK <= 1) & (j1 // TERRAIN_BLK - j0 // TERRAIN_BLK <= 1)
    ic, jc = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    return {"narrow": narrow, "two_block": ~empty & ~narrow & two, "three_block": ~empty & ~narrow & ~two,
            "clamp_ilo": ~empty & (ia < 0), "clamp_ihi": ~empty & (ib > rows - 2),
            "clamp_jlo": ~empty & (ja < 0), "clamp_jhi": ~empty & (jb > cols - 2),
            "centre_off": ~empty & ((ic < 0) | (ic > rows - 2) | (jc < 0) | (jc > cols - 2)), "empty": empty}


def decided_mask(osim, c64, r64, ref, delta):
    """The queries whose float64 answer is the same at all eight inputs perturbed by delta (module docstring)."""
    ok = np.ones(c64.shape[0], dtype=bool)
    for k in range(4):
        for s in (-delta, delta):
            cc, rr = c64.copy(), r64.copy()
            if k < 3:
                cc[:, k] += s
            else:
                rr += s
            p = osim.terrain_query(cc, rr)
            same = (p[:, 0] > 0.5) == (ref[:, 0] > 0.5)
            ok &= same & ((ref[:, 0] < 0.5) | (np.abs(p[:, 1] - ref[:, 1]) <= 4.0 * delta))
    return ok


def reference(ter, c, r, delta):
    """dict(ref64 [n, 7] with the kind and margin columns, ref32 [n, 5] as float64, decided [n]) for float32 inputs
    c, r."""
    _, flat = H.anymal()
    c64, r64 = c.astype(np.float64), r.astype(np.float64)
    o64 = OracleSim(flat, PARAMS, terrain=ter["oracle"])
    ref64 = o64.terrain_query_kind(c64, r64)
    decided = decided_mask(o64, c64, r64, ref64, delta) & (ref64[:, 6] > delta / TIE_MARGIN_DIV)
    ref32 = OracleSim(flat, PARAMS, real_bits=32, terrain=ter["oracle"]).terrain_query(c, r).astype(np.float64)
    return dict(ref64=ref64, ref32=ref32, decided=decided)


@functools.lru_cache(maxsize=None)
def member(name):
    """One family member's mesh, queries, references and range classes; computed once, read-only afterwards."""
    fam = next(f for f, ms in MEMBERS.items() if any(m == name for m, _ in ms))
    k = [m for m, _ in MEMBERS[fam]].index(name)
    n = int(round(QUERIES * MEMBERS[fam][k][1]))
    ter = mesh(name)
    c, r = queries(ter, n, seed=1000 * FAMILIES.index(fam) + k)
    out = dict(name=name, family=fam, ter=ter, c=c, r=r, delta=DELTA_FAR if fam == "far" else DELTA,
               classes=range_classes(ter, c, r), **reference(ter, c, r, DELTA_FAR if fam == "far" else DELTA))
    for a in [out["c"], out["r"], out["ref64"], out["ref32"], out["decided"]] + list(out["classes"].values()):
        a.setflags(write=False)
    return out


def family(fam):
    return [member(m) for m, _ in MEMBERS[fam]]


def host_query(ter, c, r):
    """gs_debug_terrain_query of a host-backend sim holding `ter`: [n, 5] float32 from NaN-filled buffers."""
    from isaacgymenv_amd.isaacgym import _lib
    gym, sim = H.make_host_sim("anymal", 1, PARAMS, terrain=ter)
    c, r = np.ascontiguousarray(c, np.float32), np.ascontiguousarray(r, np.float32)
    out = np.full((c.shape[0], 5), np.nan, np.float32)
    _lib.check(_lib.lib().gs_debug_terrain_query(sim.handle, c.ctypes.data, r.ctypes.data, c.shape[0],
                                                 out.ctypes.data, None), "terrain query")
    return out


def judge_one(tag, seen, fails, what, got, ref64, ref32, decided):
    """The rule for one set of queries: got [n, 5] against ref64 [n, 7] (kind, margin) and ref32 [n, 5]."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        fails.append(f"{what}: non-finite outputs at {np.nonzero(~np.isfinite(got).all(axis=1))[0][:8].tolist()}")
        return
    fg, fo, f32 = got[:, 0] > 0.5, ref64[:, 0] > 0.5, ref32[:, 0] > 0.5
    wrong = np.nonzero(decided & (fg != fo))[0]
    if wrong.size:
        fails.append(f"{what}: {wrong.size} decided queries with the wrong found flag, first {wrong[:8].tolist()}")
    both = decided & fg & fo & f32
    for field, sel in (("face", ref64[:, 5] < 2.5), ("edge", ref64[:, 5] > 2.5)):
        m = both & sel
        if not m.any():
            continue
        H.field_check(tag, seen, fails, what, f"sep_{field}", got[m, 1], ref64[m, 1], ref32[m, 1])
        H.field_check(tag, seen, fails, what, f"n_{field}", got[m, 2:5], ref64[m, 2:5], ref32[m, 2:5])


def judge(tag, seen, fails, fam, results):
    """The rule for a family: results = one [n, 5] array per member, judged over the members together."""
    ms = family(fam)
    cat = lambda k: np.concatenate([m[k] for m in ms])  # noqa: E731
    judge_one(tag, seen, fails, fam, np.concatenate([np.asarray(g, np.float64) for g in results]), cat("ref64"),
              cat("ref32"), cat("decided"))


def counts(fam):
    """The recorded counts of a family: queries, undecided, found, per contact kind, per range class."""
    ms = family(fam)
    ref = np.concatenate([m["ref64"] for m in ms])
    out = {"queries": ref.shape[0], "undecided": int(sum((~m["decided"]).sum() for m in ms)),
           "found": int((ref[:, 0] > 0.5).sum())}
    for k, name in KINDS.items():
        out[name] = int((ref[:, 5] == k).sum())
    for cl in RANGE_CLASSES:
        out[cl] = int(sum(m["classes"][cl].sum() for m in ms))
    return out


def judge_legacy(tag, what, ter, c, r, got, sep_tol=1e-4, n_tol=1e-3):
    """The two older whole-map comparisons (test_terrain_gpu.py, test_host_backend.py) under the decided-query rule:
    got [n, 5] for float32 inputs c, r on the mesh `ter`.  Every decided query's found flag; separation and normal
    within the rule's bar per field; the separation of every decided query also within the absolute tolerance those
    tests allowed 0.05 % of the queries to miss.  A normal has no per-query absolute bound (an edge contact whose
    point is nearly at the centre; a face and the edge of its rim changing places): beside the rule's bar, which
    holds every decided query, the older share (at most 0.05 % beyond n_tol) stays; n_tol=None: none was set."""
    ref = reference(ter, c, r, DELTA)
    seen, fails = {}, []
    judge_one(tag, seen, fails, what, got, ref["ref64"], ref["ref32"], ref["decided"])
    got, r64 = np.asarray(got, np.float64), ref["ref64"]
    both = ref["decided"] & (got[:, 0] > 0.5) & (r64[:, 0] > 0.5)
    dsep = np.abs(got[:, 1] - r64[:, 1])[both]
    dn = np.abs(got[:, 2:5] - r64[:, 2:5]).max(axis=1)[both]
    if (dsep > sep_tol).any():
        fails.append(f"{what}: separation off by {dsep.max():.3e} > {sep_tol:g}")
    if n_tol is not None and not (dn > n_tol).mean() < 5e-4:
        fails.append(f"{what}: {(dn > n_tol).mean():.3e} of the normals off by more than {n_tol:g}")
    print(f"[{tag}] {what}: {int((~ref['decided']).sum())} of {c.shape[0]} undecided, max |d sep| {dsep.max():.3e}, "
          f"max |d normal| {dn.max():.3e} ({seen})")
    assert (r64[:, 0] > 0.5).mean() > 0.3
    assert (~ref["decided"]).mean() <= 0.005
    assert not fails, fails
