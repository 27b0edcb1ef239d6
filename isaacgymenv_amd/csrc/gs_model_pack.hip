// gs_model_pack.hip -- gs_model_desc -> DevModel / DevLinks / GenTopo (gs_model_pack.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gs_kernel_choice.h"
#include "gs_model_pack.h"

std::string model_signature(const gs_model_desc* m) {
  std::string s = "fb" + std::to_string(m->fixed_base) + "_p";
  for (int i = 0; i < m->num_bodies; ++i) s += (i ? "-" : "") + std::to_string(m->parent[i]);
  s += "_c";
  for (int i = 0; i < m->num_candidates; ++i) s += (i ? "-" : "") + std::to_string(m->cand_body[i]);
  // kept fixed-joint links change the compiled contact-force tables (_model.topology_signature)
  // (a desc without its link table matches by bodies alone; model_pack refuses it)
  bool links_differ = m->num_links != m->num_bodies;
  for (int i = 0; i < m->num_candidates && !links_differ && m->cand_link; ++i)
    links_differ = m->cand_link[i] != m->cand_body[i];
  if (links_differ && m->cand_link) {
    s += "_l" + std::to_string(m->num_links) + "_";
    for (int i = 0; i < m->num_candidates; ++i) s += (i ? "-" : "") + std::to_string(m->cand_link[i]);
  }
  return s;
}

int model_pack(const gs_model_desc* m, const TopoEntry* t, bool host, bool has_terrain, ModelPack* out) {
  auto fail = [out](const std::string& msg) {
    out->err = msg;
    return -1;
  };
  auto num = [](long long v) { return std::to_string(v); };
  {  // table capacities of every kernel form (the runtime-sized kernel's tables are these too), each named
    const struct { const char* what; int n, cap; } lim[] = {
        {"bodies (32-bit ancestor masks)", m->num_bodies, GS_MAXB}, {"dofs", m->num_dofs, GS_MAXD},
        {"contact candidates (3 rows each)", m->num_candidates, GS_MAXC}, {"links", m->num_links, GS_MAXL},
        {"collision shapes", m->num_shapes, GS_MAXSH}};
    for (const auto& l : lim)
      if (l.n > l.cap)
        return fail("gs_sim_set_model: " + num(l.n) + " " + l.what + " exceed the limit of " + num(l.cap));
  }
  if (m->num_links < m->num_bodies || !m->link_body || !m->link_pose || !m->link_com ||
      (m->num_candidates > 0 && !m->cand_link))
    return fail("gs_sim_set_model: link tables missing (gs_model_desc ABI 2: num_links >= num_bodies)");
  for (int l = 0; l < m->num_links; ++l)
    if (m->link_body[l] < 0 || m->link_body[l] >= m->num_bodies) return fail("gs_sim_set_model: link_body out of range");
  for (int c = 0; c < m->num_candidates; ++c)
    if (m->cand_link[c] < 0 || m->cand_link[c] >= m->num_links) return fail("gs_sim_set_model: cand_link out of range");
  // A topology with no compiled kernel runs the runtime-sized kernel (gs_generic.hip, kernel_variant 4) on the GPU:
  // any tree of revolute / prismatic joints with plane contacts of point candidates (spheres, capsule / cylinder
  // ends, box corners) and convex-hull manifolds, joint limits and drives, self-collision of filter-0 actors from
  // the model's pair table, force sensors on leaf bodies.  A terrain mesh needs a compiled topology
  // (tools/gen_topologies.py), and the host backend has compiled topologies only; both are refused here.  So is a
  // model beyond one of the kernel's tables, with the limit named.
  const bool generic = !t;
  if (generic) {
    const std::string sig = model_signature(m);
    if (host) {
      std::string msg = kRefuseRuntimeOnHost;
      return fail(msg.replace(msg.find("%s"), 2, sig));
    }
    if (has_terrain)
      return fail("gs_sim_set_model: topology " + sig + " with a terrain mesh: the runtime-sized kernel has plane "
                  "contacts only (compile the topology with tools/gen_topologies.py)");
    if (m->num_dofs + 6 > GS_MAXD + 6 || (m->num_candidates > 0 && !m->cand_shape))
      return fail("gs_sim_set_model: runtime-sized kernel tables missing for " + sig);
    // the kernel's table limits, each named (the general checks below repeat some for every kernel)
    static_assert(GS_MAXB <= 32, "ancestor masks are 32-bit");
    if (m->num_pairs > GS_MAXP)
      return fail("gs_sim_set_model: " + num(m->num_pairs) + " self-collision pairs exceed the runtime-sized kernel's "
                  "limit of " + num(GS_MAXP) + " pairs (GS_MAXP)");
    if (m->num_hull_verts > GS_MAXHV)
      return fail("gs_sim_set_model: " + num(m->num_hull_verts) + " hull vertices exceed the runtime-sized kernel's "
                  "limit of " + num(GS_MAXHV) + " hull vertices (GS_MAXHV)");
    if (m->num_pairs > 0 && (m->pair_pool < 1 || m->pair_pool > GS_MAXPOOL))
      return fail("gs_sim_set_model: a self-contact pool of " + num(m->pair_pool) + " slots is outside the runtime-"
                  "sized kernel's limit of 1.." + num(GS_MAXPOOL) + " slots (GS_MAXPOOL), 3 rows each");
    for (int c = 0; c < m->num_candidates; ++c)
      if (m->cand_dyn && m->cand_dyn[c] > 3)
        return fail("gs_sim_set_model: hull slot " + num(m->cand_dyn[c]) + " of a candidate exceeds the runtime-sized "
                    "kernel's limit of 4 ground contacts per hull");
  }
  if (!generic && m->num_pairs > 0 && m->pair_pool != t->npk)
    return fail("gs_sim_set_model: self-contact pool differs from the compiled topology's " + num(t->npk));
  for (int c = 0; c < m->num_candidates && !generic; ++c)
    if (m->cand_dyn && m->cand_dyn[c] != t->cdyn[c])
      return fail("gs_sim_set_model: hull slots differ from the compiled topology (tools/gen_topologies.py)");
  // the kernels unroll the self-collision pairs and shape kinds at compile time
  if (!generic && m->num_pairs > 0 && m->num_pairs != t->npair)
    return fail("gs_sim_set_model: self-collision pair count differs from the compiled topology's " + num(t->npair));
  for (int q = 0; q < m->num_pairs && !generic; ++q)
    if (m->pair_a[q] != t->pair_a[q] || m->pair_b[q] != t->pair_b[q] || m->pair_kind[q] != t->pair_k[q])
      return fail("gs_sim_set_model: self-collision pairs differ from the compiled topology (tools/gen_topologies.py)");
  for (int sh = 0; sh < m->num_shapes && !generic; ++sh)
    if (m->shape_kind && m->shape_kind[sh] != t->shkind[sh])
      return fail("gs_sim_set_model: shape kinds differ from the compiled topology (tools/gen_topologies.py)");
  DevModel& h = out->model;
  std::memset(&h, 0, sizeof(h));
  for (int i = 0; i < m->num_bodies; ++i) {
    for (int k = 0; k < 9; ++k) h.jR[i][k] = (float)m->joint_origin[12 * i + k];
    for (int k = 0; k < 3; ++k) h.jt[i][k] = (float)m->joint_origin[12 * i + 9 + k];
    for (int k = 0; k < 3; ++k) h.jaxis[i][k] = (float)m->joint_axis[3 * i + k];
    h.mass[i] = (float)m->mass[i];
    for (int k = 0; k < 3; ++k) h.com[i][k] = (float)m->com[3 * i + k];
    const double* I = m->inertia + 9 * i;
    h.inertia[i][0] = (float)I[0]; h.inertia[i][1] = (float)I[4]; h.inertia[i][2] = (float)I[8];
    h.inertia[i][3] = (float)I[1]; h.inertia[i][4] = (float)I[2]; h.inertia[i][5] = (float)I[5];
  }
  {  // root link COM in the body-0 frame: link pose (identity for the root link) applied to its COM
    const double* P = m->link_pose;
    const double* c = m->link_com;
    for (int k = 0; k < 3; ++k)
      h.root_com[k] = (float)(P[9 + k] + P[3 * k] * c[0] + P[3 * k + 1] * c[1] + P[3 * k + 2] * c[2]);
  }
  for (int c = 0; c < m->num_candidates; ++c) {
    for (int k = 0; k < 3; ++k) h.cpoint[c][k] = (float)m->cand_point[3 * c + k];
    h.cradius[c] = (float)m->cand_radius[c];
  }
  // shapes (ABI 5): bounding spheres widened by 1e-4 relative so that float rounding never culls an active
  // candidate or pair; hull vertices; self-collision pairs
  if (!m->shape_kind || !m->shape_body || !m->shape_link || !m->shape_pose || !m->shape_size || !m->shape_margin ||
      !m->shape_sphere || !m->shape_hv0 || !m->shape_hv1 || (m->num_candidates > 0 && !m->cand_dyn))
    return fail("gs_sim_set_model: shape tables missing (gs_model_desc ABI 5)");
  if (m->num_hull_verts < 0 || m->num_hull_verts > GS_MAXHV || m->num_pairs < 0 || m->num_pairs > GS_MAXP ||
      (m->num_hull_verts > 0 && !m->hull_verts) || (m->num_pairs > 0 && (!m->pair_a || !m->pair_b || !m->pair_kind)))
    return fail("gs_sim_set_model: hull vertices / self-collision pairs exceed compiled maxima");
  for (int sh = 0; sh < m->num_shapes; ++sh) {
    for (int k = 0; k < 3; ++k) h.shc[sh][k] = (float)m->shape_sphere[4 * sh + k];
    // the sphere must hold the shape's ground candidates too (the solver skips a shape whose sphere clears the
    // ground): a cylinder's candidates are its end points with the cylinder's radius (a capsule to the plane
    // test), which reach hl + r along the axis, beyond the cylinder's own bounding sphere
    // sqrt(hl^2 + r^2) (round 5: a UsefulHound leg cylinder's end 10 mm from the ground was skipped at a 42 mm
    // sphere clearance; the pair broadphase only gets looser by it)
    double reach = m->shape_sphere[4 * sh + 3];
    for (int c = 0; c < m->num_candidates; ++c) {
      if (m->cand_shape && m->cand_shape[c] == sh && m->cand_dyn[c] < 0) {
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
          const double d = m->cand_point[3 * c + k] - m->shape_sphere[4 * sh + k];
          d2 += d * d;
        }
        reach = std::max(reach, std::sqrt(d2) + m->cand_radius[c]);
      }
    }
    h.shc[sh][3] = (float)(reach * (1.0 + 1e-4) + 1e-5);
    h.shkind[sh] = m->shape_kind[sh];
    h.shbody[sh] = m->shape_body[sh];
    h.shlink[sh] = m->shape_link[sh];
    for (int k = 0; k < 9; ++k) h.shR[sh][k] = (float)m->shape_pose[12 * sh + k];
    for (int k = 0; k < 3; ++k) h.sht[sh][k] = (float)m->shape_pose[12 * sh + 9 + k];
    for (int k = 0; k < 3; ++k) h.shsize[sh][k] = (float)m->shape_size[3 * sh + k];
    h.shm[sh] = (float)m->shape_margin[sh];
    h.hv0[sh] = m->shape_hv0[sh];
    h.hv1[sh] = m->shape_hv1[sh];
    if (h.shbody[sh] < 0 || h.shbody[sh] >= m->num_bodies || h.shlink[sh] < 0 || h.shlink[sh] >= m->num_links ||
        h.hv0[sh] < 0 || h.hv1[sh] < h.hv0[sh] || h.hv1[sh] > m->num_hull_verts ||
        (h.shkind[sh] == 4 && h.hv1[sh] == h.hv0[sh]))
      return fail("gs_sim_set_model: shape " + num(sh) + " tables out of range");
  }
  for (int v = 0; v < m->num_hull_verts; ++v)
    for (int k = 0; k < 4; ++k) h.hv[v][k] = (float)m->hull_verts[4 * v + k];
  if (m->num_pair_verts < 0 || m->num_pair_verts > GS_MAXPV || !m->shape_pv0 || !m->shape_pv1 ||
      (m->num_pair_verts > 0 && !m->pair_verts))
    return fail("gs_sim_set_model: hull self-collision cores missing or beyond GS_MAXPV");
  for (int v = 0; v < m->num_pair_verts; ++v)
    for (int k = 0; k < 4; ++k) h.pv[v][k] = (float)m->pair_verts[4 * v + k];
  for (int sh = 0; sh < m->num_shapes; ++sh) {
    h.pv0[sh] = m->shape_pv0[sh];
    h.pv1[sh] = m->shape_pv1[sh];
    if (h.pv0[sh] < 0 || h.pv1[sh] < h.pv0[sh] || h.pv1[sh] > m->num_pair_verts ||
        (h.shkind[sh] == 4 && h.pv1[sh] == h.pv0[sh]))
      return fail("gs_sim_set_model: shape " + num(sh) + " self-collision core out of range");
  }
  for (int c = 0; c < m->num_candidates; ++c)
    if (m->cand_dyn[c] >= 0 && m->shape_kind[m->cand_shape[c]] != 4)
      return fail("gs_sim_set_model: dynamic candidate " + num(c) + " on a shape that is not a hull");
  h.np = m->num_pairs;
  for (int q = 0; q < m->num_pairs; ++q) {
    h.pa[q] = m->pair_a[q];
    h.pb[q] = m->pair_b[q];
    h.pk[q] = m->pair_kind[q];
    if (h.pa[q] < 0 || h.pb[q] <= h.pa[q] || h.pb[q] >= m->num_shapes || h.pk[q] < 0 || h.pk[q] > 3)
      return fail("gs_sim_set_model: self-collision pair " + num(q) + " out of range");
  }
  out->any_limits = 0;
  for (int j = 0; j < m->num_dofs; ++j) {
    h.effort[j] = (float)m->dof_effort[j];
    h.vmax[j] = (float)m->dof_velocity[j];
    h.armature[j] = (float)m->dof_armature[j];
    h.has_lim[j] = m->dof_has_limits && m->dof_has_limits[j] && m->dof_upper[j] > m->dof_lower[j];
    h.lower[j] = h.has_lim[j] ? (float)m->dof_lower[j] : 0.f;
    h.upper[j] = h.has_lim[j] ? (float)m->dof_upper[j] : 0.f;
    out->any_limits |= h.has_lim[j];
  }
  h.nsens = 0;
  for (int b = 0; b < GS_MAXB; ++b) h.sens_of_body[b] = -1;

  DevLinks& hl = out->links;
  std::memset(&hl, 0, sizeof(hl));
  hl.nb = m->num_bodies;
  hl.nd = m->num_dofs;
  hl.nr = m->num_links;
  hl.fixed_base = m->fixed_base;
  for (int b = 0; b < m->num_bodies; ++b) {
    hl.parent[b] = m->parent[b];
    hl.jkind[b] = m->joint_kind[b];
    hl.bdof[b] = m->body_dof[b];
    unsigned mask = 0;
    for (int a = b; a >= 0; a = m->parent[a]) mask |= 1u << a;
    h.banc[b] = hl.anc_mask[b] = mask;
    if (m->body_dof[b] >= 0) hl.dbody[m->body_dof[b]] = b;
  }
  for (int l = 0; l < m->num_links; ++l) {
    hl.lbody[l] = m->link_body[l];
    for (int k = 0; k < 9; ++k) hl.lR[l][k] = (float)m->link_pose[12 * l + k];
    for (int k = 0; k < 3; ++k) hl.lt[l][k] = (float)m->link_pose[12 * l + 9 + k];
    for (int k = 0; k < 3; ++k) hl.lcom[l][k] = (float)m->link_com[3 * l + k];
  }

  GenTopo& hg = out->gen;
  std::memset(&hg, 0, sizeof(hg));
  out->gen_feat = 0;
  out->gen_entry = TopoEntry{};
  if (generic) {
    hg.nc = m->num_candidates;
    hg.ns = m->num_shapes;
    hg.npool = m->num_pairs > 0 ? m->pair_pool : 0;
    for (int c = 0; c < m->num_candidates; ++c) {
      hg.cbody[c] = m->cand_body[c];
      hg.cshape[c] = m->cand_shape[c];
      hg.clink[c] = m->cand_link[c];
      hg.cdyn[c] = m->cand_dyn[c] >= 0 ? m->cand_dyn[c] : -1;
      out->gen_feat |= m->cand_dyn[c] >= 0 ? 1 : 0;
      if (hg.cbody[c] < 0 || hg.cbody[c] >= m->num_bodies || hg.cshape[c] < 0 || hg.cshape[c] >= m->num_shapes)
        return fail("gs_sim_set_model: candidate " + num(c) + " tables out of range");
    }
    TopoEntry& g = out->gen_entry;
    g.sig = "runtime";
    g.name = "runtime-sized (gs_generic.hip)";
    g.sim = launch_sim_generic;
    g.pd = launch_pd_generic;
    g.dbg_pool = launch_dbg_pool_generic;
    g.nb = m->num_bodies; g.nd = m->num_dofs; g.nc = m->num_candidates; g.ns = m->num_shapes;
    g.sens = 1;
    // rows of an env's workspace slice: limits, 3 per candidate, 3 per self-contact slot -- the most the kernel
    // can build, so no env indexes past its slice
    g.row_floats = (int)generic_ws_floats(m->num_candidates, m->num_dofs, m->fixed_base, hg.npool);
    g.row_lanes = 1;
    g.npk = hg.npool;
    g.npair = m->num_pairs;
  }
  return 0;
}
