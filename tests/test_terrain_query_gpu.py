"""The trimesh terrain query on the GPU (k_terrain_query: gs_terrain::sphere_contact as every physics kernel form
calls it) held to the float64 oracle under the decided-query rule of tests/terrain_cases.py, against the host backend
on the same queries, and one simulate with ANYmal over the map's edge in every kernel form that takes a mesh (the
lane team runs may_contact first, then sphere_contact_scan on the wave: the only place its split path meets an edge).

Measured on an MI355X (profiles/terrain_parity.txt): every decided query's found flag matches in all five families
(undecided: 5, 88, 1, 25 and 4 of 20 000); err_kernel / bar at most 0.28 (far, edge separations: 9.0e-6 m against
the float32 oracle's 8.1e-6 m), elsewhere separations 2e-8 to 1.8e-7 m and normals at the float32 oracle's own error
(err_kernel / err_f32 0.30 to 1.11).  Against the host backend on decided queries: flags equal, separations within
2e-7 m (4.8e-6 m far), normals within 1.5e-4.  The 200 000 interior queries of test_terrain_gpu.py: 97 undecided, the
rest matched, max separation error 2.0e-7 m.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import kinematics_oracle as KO
from oracle.oracle import OracleSim
from tests import helpers as H
from tests import terrain_cases as TC

pytestmark = pytest.mark.gpu

TAG = "terrain-parity-gpu"


def _gpu_query(sim, c, r):
    """gs_debug_terrain_query on a GPU sim: [n, 5] float32 from a NaN-filled buffer, and the NaN-filled guard row
    behind it (nothing may be written there)."""
    from isaacgymenv_amd.isaacgym import _lib
    n = c.shape[0]
    cd, rd = torch.from_numpy(np.ascontiguousarray(c)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda()
    out = torch.full((n + 1, 5), float("nan"), device="cuda:0")
    _lib.check(_lib.lib().gs_debug_terrain_query(sim.handle, cd.data_ptr(), rd.data_ptr(), n, out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "terrain query")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:n], o[n]


@functools.lru_cache(maxsize=None)
def _gpu_results(name):
    """One family member's queries on a GPU sim holding its mesh: the whole set, its guard row, a repeat of the whole
    set, and the first 1, 255 and 257 queries alone (the t >= n guard of a 256-thread block)."""
    m = TC.member(name)
    gym, sim = H.make_gpu_sim("anymal", 1, TC.PARAMS, terrain=m["ter"])
    full, guard = _gpu_query(sim, m["c"], m["r"])
    again, _ = _gpu_query(sim, m["c"], m["r"])
    short = {n: _gpu_query(sim, m["c"][:n], m["r"][:n]) for n in (1, 255, 257)}
    return dict(full=full, guard=guard, again=again, short=short)


@pytest.mark.parametrize("fam", TC.FAMILIES)
def test_gpu_query_meets_the_rule(fam):
    """Every decided query's found flag, and separation and normal within the bar per field; every output written
    (no NaN left), nothing written past n, at n = 1, 255 and 257 too; a repeated call returns the same bits."""
    seen, fails = {}, []
    res = [_gpu_results(m["name"]) for m in TC.family(fam)]
    TC.judge(TAG, seen, fails, fam, [g["full"] for g in res])
    print(f"[{TAG}] {fam} gpu (err_kernel/err_f32, err_kernel/bar): {seen}")
    assert not fails, fails
    for g in res:
        assert np.isnan(g["guard"]).all(), "a write past the last query"
        assert g["full"].tobytes() == g["again"].tobytes(), "a repeated call differs"
        for n, (o, guard) in g["short"].items():
            assert np.isnan(guard).all(), f"n = {n}: a write past the last query"
            assert o.tobytes() == g["full"][:n].tobytes(), f"n = {n}: differs from the same queries in the whole set"


@pytest.mark.parametrize("fam", TC.FAMILIES)
def test_gpu_query_agrees_with_host_backend(fam):
    """The kernel against the host backend's compile of the same source: found flags equal on every decided query;
    the largest differences in separation and normal (contraction and the device's division and square root may
    differ from the host's) are reported."""
    dsep = dn = 0.0
    for m in TC.family(fam):
        g = _gpu_results(m["name"])["full"].astype(np.float64)
        h = TC.host_query(m["ter"], m["c"], m["r"]).astype(np.float64)
        dec = m["decided"]
        bad = np.nonzero(dec & ((g[:, 0] > 0.5) != (h[:, 0] > 0.5)))[0]
        assert bad.size == 0, (m["name"], bad[:8].tolist())
        both = dec & (g[:, 0] > 0.5) & (h[:, 0] > 0.5)
        if both.any():
            dsep = max(dsep, float(np.abs(g[both, 1] - h[both, 1]).max()))
            dn = max(dn, float(np.abs(g[both, 2:5] - h[both, 2:5]).max()))
    print(f"[{TAG}] {fam} gpu vs host backend on decided queries: max |d sep| {dsep:.3e} max |d normal| {dn:.3e}")


# ------------------------------------------------------------------------------------ one simulate over the edge
PLACEMENTS = ("edge", "corner", "off")
FEET = (3, 6, 9, 12)
EDGE_ENVS = 8
# the share of envs that may be beyond tolerance (each of them explained by the oracle's own sensitivity, or the test
# fails): the 2 % of test_rough_terrain_one_simulate_matches_oracle stands for its few envs on a stair edge; here
# every env is put on the mesh's rim on purpose, so one env in four
EDGE_ENV_FRAC = 0.25
SINK = 0.01  # the deepest foot over the mesh starts this far into the surface


def _foot_spheres(flat, root, q):
    """Per foot body: (centre [3], radius) of its lowest contact candidate in the world."""
    R, p, _, _ = KO.fk(flat, root, q)
    out = []
    for b in FEET:
        cs = [k for k in range(flat["nc"]) if flat["cbody"][k] == b]
        x = np.array([p[b] + R[b] @ np.asarray(flat["cpoint"][k][:3], np.float64) for k in cs])
        k = int(np.argmin(x[:, 2] - np.asarray(flat["cradius"], np.float64)[cs]))
        out.append((x[k], float(flat["cradius"][cs[k]])))
    return out


def _edge_states(placement, ter, seed):
    """ANYmal in its default pose, slightly tilted and moving, at the high-x (and high-y) end of the mesh:
    edge   the hind feet on the last cell row, the front feet beyond the mesh
    corner the base over the corner: one hind foot on the mesh, three feet beyond it
    off    a metre beyond the mesh: no contact, free fall
    with the deepest foot on the mesh SINK into the surface under it.  Returns the states and on [n, 4] (foot centre
    over the mesh)."""
    art, flat = H.anymal()
    n = EDGE_ENVS
    root, dof, tau, mu = H.anymal_states(n, seed=seed, spread=0.2)
    dof[:, :, 0] = np.array([H.ANYMAL_DEFAULT[d] for d in art.dof_names()])
    o = ter["oracle"]
    rows, cols, hs = o["rows"], o["cols"], o["hs"]
    x1, y1 = o["x0"] + (rows - 1) * hs, o["y0"] + (cols - 1) * hs
    grid = o["vertices"].reshape(rows, cols, 3)
    rng = np.random.RandomState(seed + 7)
    on = np.zeros((n, 4), bool)
    osim = OracleSim(flat, TC.PARAMS, terrain=o)
    for e in range(n):
        root[e, 0:3] = 0.0
        feet = _foot_spheres(flat, root[e], dof[e, :, 0])
        fx = np.array([f[0][0] for f in feet])
        hind = fx < 0
        if placement == "edge":
            root[e, 0] = x1 - 0.05 - fx[hind].mean() + rng.uniform(-0.01, 0.01)
            root[e, 1] = y1 - 1.0 + rng.uniform(-0.3, 0.3)
        elif placement == "corner":
            root[e, 0], root[e, 1] = x1 + rng.uniform(-0.02, 0.02), y1 + rng.uniform(-0.02, 0.02)
        else:
            root[e, 0], root[e, 1] = x1 + 1.0, y1 - 1.0
        for k, (x, r) in enumerate(feet):
            wx, wy = x[0] + root[e, 0], x[1] + root[e, 1]
            on[e, k] = o["x0"] <= wx <= x1 and o["y0"] <= wy <= y1
        if not on[e].any():
            root[e, 2] = 0.6
            continue
        # lower the robot until its deepest foot over the mesh is SINK into the surface (the oracle's own query)
        cs = np.array([feet[k][0] + [root[e, 0], root[e, 1], 0.0] for k in range(4) if on[e, k]])
        rs = np.array([feet[k][1] for k in range(4) if on[e, k]])
        gi = np.clip(np.round((cs[:, 0] - o["x0"]) / hs).astype(int), 0, rows - 1)
        gj = np.clip(np.round((cs[:, 1] - o["y0"]) / hs).astype(int), 0, cols - 1)
        z = float(np.max(grid[gi, gj, 2] - (cs[:, 2] - rs))) + 0.015
        for _ in range(8):
            q = osim.terrain_query(cs + [0.0, 0.0, z], rs)
            sep = np.where(q[:, 0] > 0.5, q[:, 1], TC.PARAMS["contact_offset"]).min()
            z -= sep + SINK
        root[e, 2] = z
    return root, dof, tau, mu, on


def test_edge_placements_are_what_they_claim():
    """From the kinematics alone: which feet are over the mesh in each placement, and where."""
    ter = TC.mesh("rough")
    o = ter["oracle"]
    x1 = o["x0"] + (o["rows"] - 1) * o["hs"]
    art, flat = H.anymal()
    for placement, feet_on in (("edge", 2), ("corner", 1), ("off", 0)):
        root, dof, tau, mu, on = _edge_states(placement, ter, seed=3)
        assert np.all(on.sum(axis=1) == feet_on), (placement, on)
        if placement == "edge":
            for e in range(EDGE_ENVS):
                for k, (x, r) in enumerate(_foot_spheres(flat, root[e], dof[e, :, 0])):
                    if on[e, k]:
                        assert x1 - o["hs"] < x[0] < x1, "a hind foot's centre over the last cell row"
                    else:
                        assert x[0] - r > x1, "a front foot wholly beyond the mesh"


@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("kernel", ["lane", "team"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_one_simulate_over_the_map_edge_matches_oracle(placement, kernel, solver, monkeypatch):
    monkeypatch.setenv("GS_PHYSICS_KERNEL", kernel)
    ter = TC.mesh("rough")
    art, flat = H.anymal()
    n = EDGE_ENVS
    root0, dof0, tau, mu, on = _edge_states(placement, ter, seed=3)
    gym, sim = H.make_gpu_sim("anymal", n, dict(TC.PARAMS, solver_type=1 if solver == "tgs" else 0), terrain=ter)
    assert sim.kernel_variant == {"lane": 1, "team": 2}[kernel]
    H.load_state_into(sim, root0, dof0, mu)
    sim.dof_force.copy_(torch.from_numpy(tau.astype(np.float32).reshape(-1)))
    gym.simulate(sim)
    torch.cuda.synchronize()
    g_root, g_dof = H.read_state(sim, 12)
    g_cf = sim.cf_soa.cpu().numpy().T.reshape(n, 13, 3).astype(np.float64)
    params = dict(TC.PARAMS, solver_type=3 if solver == "tgs" else 0)  # the oracle's TGS restatement
    r, d, cf, _ = H.oracle_run(flat, params, root0, dof0, tau, mu, 64, nc=flat["nb"], terrain=ter["oracle"])
    touching = np.abs(cf[:, FEET, :]).sum(axis=2) > 0
    if placement == "off":
        assert not np.abs(cf).any() and not np.abs(g_cf).any(), "free fall: no contact force"
    else:
        assert not touching[~on].any(), "a foot beyond the mesh has no contact"
        assert touching.any(axis=1).mean() >= 0.5, "at least half of the envs push on the mesh in this step"

    def rerun(idx, rng, bits):
        rr, dd = H.perturbed(root0, dof0, idx, rng)
        rr, dd, c, _ = H.oracle_run(flat, params, rr, dd, tau[idx], mu[idx], bits, nc=flat["nb"],
                                    terrain=ter["oracle"])
        return H.state_fields(rr, dd, c)
    H.assert_close_or_explained(H.state_fields(g_root, g_dof, g_cf), H.state_fields(r, d, cf), rerun,
                                max_env_frac=EDGE_ENV_FRAC,
                                what=f"map edge, {placement} ({kernel} kernel, {solver.upper()})")


def test_runtime_sized_kernel_refuses_a_mesh(monkeypatch):
    """The one GPU kernel form without mesh contacts says so when the model is set."""
    monkeypatch.setenv("GS_PHYSICS_KERNEL", "generic")
    with pytest.raises(RuntimeError, match="terrain mesh"):
        H.make_gpu_sim("anymal", EDGE_ENVS, TC.PARAMS, terrain=TC.mesh("rough"))
