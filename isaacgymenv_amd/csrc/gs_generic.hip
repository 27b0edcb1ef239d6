// gs_generic.hip -- the runtime-sized articulation solver (kernel_variant 4): any robot whose topology is not
// compiled into libgymsim (tools/gen_topologies.py) still simulates, sized from the model tables at
// gs_sim_set_model instead of a compile-time Topo_* (the fork's own
// assets/urdf/Hound_new/Hound.urdf, loaded by /root/reference/isaacgymenvs/tasks/hound.py:168-183, is the proof).
//
// Same solver specification as the compiled kernels and the oracle: spatial inertias at the
// root origin O, RNEA bias with gravity as base acceleration, CRBA mass matrix in mixed coordinates
// nu = (w, p_dot_origin, q_dot) with the h (w x p_dot) term, plane contact candidates (spheres, capsule / cylinder
// ends, box corners) active within contact_offset, joint-limit rows within limit_margin, joint drives (implicit
// within the effort, clamped beyond it), PGS with split impulse or the position sub-steps of TGS (physx.solver_type
// 1), joint velocity clamp, semi-implicit integration with the position-phase velocity.  What the
// compiled kernels do with compile-time tree tables and register arrays, this one does densely in joint space:
// the mass matrix is factored (Cholesky), each contact row's response W = M^-1 J^T is two triangular solves.
//
// Mapping (MI355X): ONE WAVE PER ENV.  Body recursions (kinematics, RNEA, composite inertias) are serial over the
// tree and run in lane 0 on LDS-resident body tables; everything dense is spread over the 64 lanes -- the mass
// matrix rows (lane = body), the Cholesky columns (lane = row), candidates (lane = candidate, activity compacted
// by a ballot prefix in candidate order), Jacobian rows (lane = column), the row solves (lane = row) and the
// Gauss-Seidel sweeps (lane = velocity component: u = J v is a wave reduction, v += W dl a vector update).  The
// rows J, W live in a per-env workspace in device memory (SimBuffers::rows), the factor and the body tables in
// LDS.
//
// Two forms of the kernel, chosen per launch (launch_sim_generic).  The plain form is the above and nothing else.
// The full form (FEAT) adds, for sims that have them:
//  * convex-hull ground manifolds: per hull shape near the ground, the 4-point selection of
//    gs_pairs.h hull_ground_select with lane = vertex in rounds of 64 and (value, index) wave reductions whose ties
//    go to the lowest index; the selected body-frame points stay in LDS and stand in for M->cpoint;
//  * self-collision: shape world data in LDS (lane = shape), broadphase with lane = pair and a
//    ballot prefix into pair order, narrowphase with one listed pair per lane (gs_pairs.h self_pair, unchanged),
//    at most npool contacts in pair order; their rows (J = d . (v_A(x) - v_B(x)), common ancestors cancel) follow
//    the ground rows and are solved in the same sweeps; a row below GS_MIN_RESPONSE takes no impulse;
//  * force sensors on leaf bodies, lane = body, from the last substep's accelerations.
// Not supported here (fails loudly at set-up): terrain meshes -- those robots need a compiled topology -- and no
// host backend.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "gs_internal.h"
#include "gs_math.h"
#include "gs_pairs.h"

namespace {

constexpr int kGW = 64;         // lanes per env (one wave)
constexpr int kGMaxV = GS_MAXD + 6;

struct GBody {  // LDS body tables of one env
  float R[GS_MAXB][9], P[GS_MAXB][3], S[GS_MAXB][6], V[GS_MAXB][6], A[GS_MAXB][6], F[GS_MAXB][6];
  SpI Ib[GS_MAXB], Ic[GS_MAXB];
};

// Row tables: limit rows (<= nd), 3 rows per ground candidate, and in the full form 3 rows per self-contact slot
template <bool FEAT>
constexpr int kGRows = 3 * GS_MAXC + GS_MAXD + (FEAT ? 3 * GS_MAXPOOL : 0);

// LDS of the full form (FEAT): hull manifolds, shape world data, the near-pair list and the self-contact pool
constexpr int kGPE = kPoolLB + 1;  // pool entry: gs_pairs.h layout up to the links (x n t1 t2 sep mu bodies links)
struct GFeat {
  float shw[kShW * GS_MAXSH];    // shape world data (gs_pairs.h layout, stride 1)
  float hp[4 * GS_MAXSH][3];     // a hull shape's selected ground vertices, body frame (slot 4 sh + j)
  int hn[GS_MAXSH];              // how many of them (0: not a hull, or clear of the ground)
  float pool[GS_MAXPOOL * kGPE];
  int near[GS_MAXP];             // pairs within reach of the broadphase, in pair order
};
struct GNoFeat {};

// self_pair's topology parameter for a runtime pair table: shape kinds from the model, the pool cap applied by the
// caller (a lane's pair yields at most 2 contacts)
struct GenPairT {
  static constexpr int NPK = GS_MAXPOOL;
};

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kGW);
  return x;
}

// (value, index) maximum over the wave: the largest value, on ties the lowest index (-1 = none loses every tie) --
// what a serial scan in index order with a strict > keeps
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, kGW);
    const int oi = __shfl_xor(i, o, kGW);
    if (ov > v || (ov == v && (unsigned)oi < (unsigned)i)) { v = ov; i = oi; }
  }
}

// gs_pairs.h hull_ground_select spread over the wave: lane = vertex, in rounds of 64 over the hull's range; every
// step is a (value, index) reduction with the serial rule's tie-break (first index).  Returns the count (uniform),
// the vertex indices in sel.
__device__ int hull_select_wave(const DevModel* __restrict__ M, int sh, const float* R, const float* X, float rootz,
                                float off, int* sel, int lane) {
  const int v0 = M->hv0[sh], v1 = M->hv1[sh];
  auto world = [&](const float* v, float* w) {
    w[0] = X[0] + R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
    w[1] = X[1] + R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
    w[2] = rootz + X[2] + R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
  };
  // best over the vertices of f(w) (a value to maximise; `all`: vertices at or above `off` count too) above floor
  auto scan = [&](float floor, bool all, auto&& f, int& idx) {
    float best = floor;
    int bi = -1;
    for (int k = v0 + lane; k < v1; k += kGW) {
      const float4 hv = *reinterpret_cast<const float4*>(M->hv[k]);
      const float v[3] = {hv.x, hv.y, hv.z};
      float w[3];
      world(v, w);
      if (!all && !(w[2] < off)) continue;
      const float val = f(w);
      if (val > best) { best = val; bi = k; }
    }
    wave_argmax(best, bi);
    idx = bi;
    return best;
  };
  int i0, i1, i2, i3;
  const float nz = scan(-3.0e38f, true, [&](const float* w) { return -w[2]; }, i0);
  if (i0 < 0 || !(-nz < off)) return 0;
  int n = 0;
  float p0[3];
  world(M->hv[i0], p0);
  sel[n++] = i0;
  scan(1e-10f, false, [&](const float* w) {
    return (w[0] - p0[0]) * (w[0] - p0[0]) + (w[1] - p0[1]) * (w[1] - p0[1]);
  }, i1);
  if (i1 < 0) return n;
  float p1[3];
  world(M->hv[i1], p1);
  sel[n++] = i1;
  const float ex = p1[0] - p0[0], ey = p1[1] - p0[1];
  scan(1e-10f, false, [&](const float* w) { return fabsf(ex * (w[1] - p0[1]) - ey * (w[0] - p0[0])); }, i2);
  if (i2 < 0) return n;
  float p2[3];
  world(M->hv[i2], p2);
  sel[n++] = i2;
  const float sg = (ex * (p2[1] - p0[1]) - ey * (p2[0] - p0[0])) > 0.f ? 1.f : -1.f;
  scan(1e-10f, false, [&](const float* w) {
    const float e0 = sg * ((p1[0] - p0[0]) * (w[1] - p0[1]) - (p1[1] - p0[1]) * (w[0] - p0[0]));
    const float e1 = sg * ((p2[0] - p1[0]) * (w[1] - p1[1]) - (p2[1] - p1[1]) * (w[0] - p1[0]));
    const float e2 = sg * ((p0[0] - p2[0]) * (w[1] - p2[1]) - (p0[1] - p2[1]) * (w[0] - p2[0]));
    return -fminf(fminf(e0, e1), e2);
  }, i3);
  if (i3 >= 0) sel[n++] = i3;
  return n;
}

// Ground manifolds of the hull shapes from the body poses in B: a hull whose bounding sphere clears
// contact_offset has none; the selected vertices' body-frame points go to X.hp, their count to X.hn.
__device__ void hull_manifolds(const DevModel* __restrict__ M, const GenTopo* __restrict__ G, const DevParams& P,
                               const GBody& B, float rootz, GFeat& X, int lane) {
  for (int sh = 0; sh < G->ns; ++sh) {
    int n = 0, sel[4] = {0, 0, 0, 0};
    if (M->shkind[sh] == 4 && P.has_ground) {
      const int b = M->shbody[sh];
      const float* R = B.R[b];
      const float* sc = M->shc[sh];
      const float cz = rootz + B.P[b][2] + R[6] * sc[0] + R[7] * sc[1] + R[8] * sc[2];
      if (cz - sc[3] < P.contact_offset) n = hull_select_wave(M, sh, R, B.P[b], rootz, P.contact_offset, sel, lane);
    }
    if (lane < n) {
      const int k = lane == 0 ? sel[0] : (lane == 1 ? sel[1] : (lane == 2 ? sel[2] : sel[3]));
      for (int a = 0; a < 3; ++a) X.hp[4 * sh + lane][a] = M->hv[k][a];
    }
    if (lane == 0) X.hn[sh] = n;
  }
  __syncthreads();
}

// Self-contacts of the env from the body poses in B, as gs_pairs.h self_contacts finds them, spread
// over the wave: shape world data (lane = shape), broadphase (lane = pair, 64 per round, the near ones ranked by a
// ballot prefix into pair order), narrowphase (one listed pair per lane: gs_pairs.h self_pair), and the contacts
// ranked again into the pool -- at most npool, in pair order, later ones dropped.  Returns the count (uniform).
__device__ int self_contacts_wave(const DevModel* __restrict__ M, const GenTopo* __restrict__ G, const DevParams& P,
                                  const float* __restrict__ mu, int N, int e, const GBody& B, GFeat& X, int lane) {
  for (int sh = lane; sh < G->ns; sh += kGW) {
    const int b = M->shbody[sh];
    float* o = X.shw + kShW * sh;
    float Rs[9], t[3];
    mat3mul(B.R[b], M->shR[sh], Rs);
    for (int k = 0; k < 9; ++k) o[k] = Rs[k];
    mat3vec(B.R[b], M->sht[sh], t);
    for (int k = 0; k < 3; ++k) o[9 + k] = B.P[b][k] + t[k];
    mat3vec(B.R[b], M->shc[sh], t);
    for (int k = 0; k < 3; ++k) o[12 + k] = B.P[b][k] + t[k];
  }
  __syncthreads();
  const int np = M->np, npool = G->npool;
  const float off = P.contact_offset;
  const ShapeConstsM sc{M};
  int cnt = 0;
  for (int q0 = 0; q0 < np; q0 += kGW) {
    const int q = q0 + lane;
    bool near = false;
    if (q < np) {
      const int a = M->pa[q], b = M->pb[q];
      const float* sa = X.shw + kShW * a + 12;
      const float* sb = X.shw + kShW * b + 12;
      const float d[3] = {sa[0] - sb[0], sa[1] - sb[1], sa[2] - sb[2]};
      const float rr = sc.brad(a) + sc.brad(b) + off;
      near = dot3f(d, d) < rr * rr;
    }
    const unsigned long long bal = __ballot(near);
    if (near) X.near[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = q;
    cnt += __popcll(bal);
  }
  __syncthreads();
  int n = 0;
  for (int i0 = 0; i0 < cnt && n < npool; i0 += kGW) {
    const int i = i0 + lane;
    int c = 0, a = 0, b = 0;
    float rec[2 * kRec];
    if (i < cnt) {
      const int q = X.near[i];
      a = M->pa[q];
      b = M->pb[q];
      self_pair<GenPairT, 1, 1, kRec, ShapeConstsM, true>(M, sc, P, mu, N, e, X.shw, rec, a, b, M->pk[q], c);
    }
    const unsigned long long b1 = __ballot(c >= 1), b2 = __ballot(c >= 2), lower = (1ull << lane) - 1ull;
    const int slot = n + __popcll(b1 & lower) + __popcll(b2 & lower);
    for (int j = 0; j < c; ++j) {
      if (slot + j >= npool) break;
      float* o = X.pool + kGPE * (slot + j);
      for (int k = 0; k < 6; ++k) o[k] = rec[kRec * j + k];
      o[kPoolSep] = rec[kRec * j + kRecSep];
      pool_entry_finish<1>(M, mu, N, e, a, b, o);
    }
    n += __popcll(b1) + __popcll(b2);
  }
  __syncthreads();
  return n < npool ? n : npool;
}

__device__ __forceinline__ void axis_rot(const float* a, float q, float* Rq) {
  float s, c;
  sincosf(q, &s, &c);
  const float C = 1.f - c;
  Rq[0] = c + a[0] * a[0] * C;        Rq[1] = a[0] * a[1] * C - a[2] * s; Rq[2] = a[0] * a[2] * C + a[1] * s;
  Rq[3] = a[1] * a[0] * C + a[2] * s; Rq[4] = c + a[1] * a[1] * C;        Rq[5] = a[1] * a[2] * C - a[0] * s;
  Rq[6] = a[2] * a[0] * C - a[1] * s; Rq[7] = a[2] * a[1] * C + a[0] * s; Rq[8] = c + a[2] * a[2] * C;
}

// per-actor dof property f of dof j (GS_DOFP_FIELDS order), else the asset's value
__device__ __forceinline__ float gdofp(const DevParams& P, int nd, int e, int f, int j, float mv) {
  return P.dof_env ? P.dof_env[((size_t)f * nd + j) * P.dof_env_n + e] : mv;
}

// One substep of env e (the whole wave).  st: SoA state; tau: [N][nd] or null; ws: this env's row workspace
// (J then W, row stride nv); cf: [3 nr][N] or null (collect).
// FEAT: the full form -- hull ground manifolds, self-contacts and force sensors (sens: [6 nsens][N] or null); X is
// its LDS.  Without FEAT none of that code exists: a robot of point candidates with neither pairs nor sensors runs
// the plain form (launch_sim_generic selects).
template <bool FEAT>
__device__ void generic_substep(const DevModel* __restrict__ M, const DevLinks* __restrict__ L,
                                const GenTopo* __restrict__ G, const DevParams& P, float* __restrict__ st,
                                const float* __restrict__ mu, int N, int e, const float* __restrict__ tau_e,
                                float* __restrict__ ws, float* __restrict__ cf, float* __restrict__ sens, GBody& B,
                                float* Ml, float* rowf, int* rowi, float* vec,
                                std::conditional_t<FEAT, GFeat, GNoFeat>& X, float* __restrict__ dff) {
  const int lane = threadIdx.x & (kGW - 1);
  const int nb = L->nb, nd = L->nd, fb = L->fixed_base;
  const int nbase = fb ? 0 : 6, nv = nbase + nd;
  const float h = P.h;
  const int maxrows = 3 * G->nc + nd + 3 * G->npool;
  float* Jw = ws;                             // [maxrows][nv]
  float* Ww = ws + (size_t)maxrows * nv;      // [maxrows][nv]
  // vec: nu (nv) | nuf (nv) | rhs (nv) | root (13) | q (nd) | qd (nd) | dforce (nd) | dimpl (nd)
  float* nu = vec;
  float* nuf = vec + kGMaxV;
  float* rhs = vec + 2 * kGMaxV;
  float* root = vec + 3 * kGMaxV;
  float* q = root + 13;
  float* qd = q + GS_MAXD;
  float* dforce = qd + GS_MAXD;
  float* dimpl = dforce + GS_MAXD;
  // row tables (rowf: separation, mu, normal xyz, Dr, lam | rowi: kind (0 limit, 1 contact row), candidate / dof)
  float* rsep = rowf;
  constexpr int NR = kGRows<FEAT>;
  float* rmu = rowf + 1 * NR;
  float* rD = rowf + 2 * NR;
  float* rlam = rowf + 3 * NR;
  float* rsg = rowf + 4 * NR;  // limit rows: +1 lower, -1 upper

  // ---------------- state in
  if (lane < 13) root[lane] = st[(size_t)lane * N + e];
  for (int j = lane; j < nd; j += kGW) {
    q[j] = st[(size_t)(13 + j) * N + e];
    qd[j] = st[(size_t)(13 + nd + j) * N + e];
  }
  __syncthreads();

  // ---------------- lane 0: kinematics, velocities, RNEA, composite inertias (serial over the tree)
  if (lane == 0) {
    const float qn = 1.f / sqrtf(root[3] * root[3] + root[4] * root[4] + root[5] * root[5] + root[6] * root[6]);
    const float q4[4] = {root[3] * qn, root[4] * qn, root[5] * qn, root[6] * qn};
    quat_to_mat(q4, B.R[0]);
    B.P[0][0] = B.P[0][1] = B.P[0][2] = 0.f;
    for (int k = 0; k < 6; ++k) { B.S[0][k] = 0.f; B.V[0][k] = 0.f; }
    if (!fb) {
      B.V[0][0] = root[10]; B.V[0][1] = root[11]; B.V[0][2] = root[12];
      B.V[0][3] = root[7]; B.V[0][4] = root[8]; B.V[0][5] = root[9];
    }
    B.A[0][0] = B.A[0][1] = B.A[0][2] = 0.f;
    B.A[0][3] = -P.g[0]; B.A[0][4] = -P.g[1]; B.A[0][5] = -P.g[2];
    for (int i = 1; i < nb; ++i) {
      const int pa = L->parent[i];
      float RJ[9], t[3], aw[3];
      mat3mul(B.R[pa], M->jR[i], RJ);
      mat3vec(B.R[pa], M->jt[i], t);
      for (int k = 0; k < 3; ++k) B.P[i][k] = B.P[pa][k] + t[k];
      mat3vec(RJ, M->jaxis[i], aw);
      const int d = L->bdof[i];
      const float qj = q[d];
      if (L->jkind[i] == 1) {
        float Rq[9];
        axis_rot(M->jaxis[i], qj, Rq);
        mat3mul(RJ, Rq, B.R[i]);
        B.S[i][0] = aw[0]; B.S[i][1] = aw[1]; B.S[i][2] = aw[2];
        cross3(B.P[i], aw, &B.S[i][3]);
      } else {
        for (int k = 0; k < 9; ++k) B.R[i][k] = RJ[k];
        for (int k = 0; k < 3; ++k) B.P[i][k] += aw[k] * qj;
        B.S[i][0] = B.S[i][1] = B.S[i][2] = 0.f;
        B.S[i][3] = aw[0]; B.S[i][4] = aw[1]; B.S[i][5] = aw[2];
      }
      const float w = qd[d];
      float c6[6];
      for (int k = 0; k < 6; ++k) B.V[i][k] = B.V[pa][k] + B.S[i][k] * w;
      crm(B.V[i], B.S[i], c6);
      for (int k = 0; k < 6; ++k) B.A[i][k] = B.A[pa][k] + c6[k] * w;
    }
    for (int i = 0; i < nb; ++i) {
      // spatial inertia at O: m, h = m c, I_O = R I_c R^T + m ([c]^T [c])
      float c[3], Am[9];
      mat3vec(B.R[i], M->com[i], c);
      for (int k = 0; k < 3; ++k) c[k] += B.P[i][k];
      const float* Il = M->inertia[i];  // xx yy zz xy xz yz
      const float* R = B.R[i];
      for (int r = 0; r < 3; ++r) {
        Am[3 * r + 0] = R[3 * r] * Il[0] + R[3 * r + 1] * Il[3] + R[3 * r + 2] * Il[4];
        Am[3 * r + 1] = R[3 * r] * Il[3] + R[3 * r + 1] * Il[1] + R[3 * r + 2] * Il[5];
        Am[3 * r + 2] = R[3 * r] * Il[4] + R[3 * r + 1] * Il[5] + R[3 * r + 2] * Il[2];
      }
      const float m = M->mass[i], cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
      SpI& I = B.Ib[i];
      I.m = m;
      I.h[0] = m * c[0]; I.h[1] = m * c[1]; I.h[2] = m * c[2];
      I.I[0] = Am[0] * R[0] + Am[1] * R[1] + Am[2] * R[2] + m * (cc - c[0] * c[0]);
      I.I[1] = Am[3] * R[3] + Am[4] * R[4] + Am[5] * R[5] + m * (cc - c[1] * c[1]);
      I.I[2] = Am[6] * R[6] + Am[7] * R[7] + Am[8] * R[8] + m * (cc - c[2] * c[2]);
      I.I[3] = Am[0] * R[3] + Am[1] * R[4] + Am[2] * R[5] - m * c[0] * c[1];
      I.I[4] = Am[0] * R[6] + Am[1] * R[7] + Am[2] * R[8] - m * c[0] * c[2];
      I.I[5] = Am[3] * R[6] + Am[4] * R[7] + Am[5] * R[8] - m * c[1] * c[2];
      B.Ic[i] = I;
      float ia[6], iv[6], x6[6];
      spi_mul(I, B.A[i], ia);
      spi_mul(I, B.V[i], iv);
      crf(B.V[i], iv, x6);
      for (int k = 0; k < 6; ++k) B.F[i][k] = ia[k] + x6[k];
    }
    for (int i = nb - 1; i > 0; --i) {
      const int pa = L->parent[i];
      SpI& a = B.Ic[pa];
      const SpI& b = B.Ic[i];
      a.m += b.m;
      for (int k = 0; k < 3; ++k) a.h[k] += b.h[k];
      for (int k = 0; k < 6; ++k) a.I[k] += b.I[k];
      for (int k = 0; k < 6; ++k) B.F[pa][k] += B.F[i][k];
    }
    // generalized velocity and the bias c(q, nu)
    if (!fb) {
      for (int k = 0; k < 3; ++k) { nu[k] = root[10 + k]; nu[3 + k] = root[7 + k]; }
      for (int k = 0; k < 6; ++k) rhs[k] = -B.F[0][k];
    }
    for (int j = 0; j < nd; ++j) nu[nbase + j] = qd[j];
  }
  __syncthreads();

  // ---------------- full form: hull ground manifolds and the self-contact pool from the body poses
  int npc = 0;
  if constexpr (FEAT) {
    if (P.gen_feat & 1) hull_manifolds(M, G, P, B, root[2], X, lane);
    if (P.self_collide) npc = self_contacts_wave(M, G, P, mu, N, e, B, X, lane);
  }

  // ---------------- drives and generalized forces (lane = dof)
  for (int j = lane; j < nd; j += kGW) {
    const int i = L->dbody[j];
    const float bias = dot6(B.S[i], B.F[i]);
    const float ef = gdofp(P, nd, e, 2, j, M->effort[j]);
    float t = tau_e ? tau_e[j] : 0.f;
    if (ef > 0.f) t = clampf(t, -ef, ef);
    float r = t - bias;
    float df = 0.f, imp = 0.f;
    if (P.any_drive) {
      const float pt = P.ptgt ? P.ptgt[(size_t)e * nd + j] : 0.f;
      const float vt = P.vtgt ? P.vtgt[(size_t)e * nd + j] : 0.f;
      const float f = gdofp(P, nd, e, 0, j, M->dkp[j]) * (pt - q[j] - h * qd[j]) + gdofp(P, nd, e, 1, j, M->dkd[j]) * (vt - qd[j]);
      const bool im = !(ef > 0.f) || fabsf(f) <= ef;
      df = im ? f : clampf(f, -ef, ef);
      imp = im ? 1.f : 0.f;
      r += df;
    }
    rhs[nbase + j] = r;
    dforce[j] = df;
    dimpl[j] = imp;
    // the DOF force tensor (gs_solver.h substep's dff_soa): actuation + drive estimate, and the qd half of an
    // implicit drive's -(h kd + h^2 kp)(qd_end - qd); the store after the integration completes it
    if (dff) {
      float f = t + df;
      if (imp != 0.f) f += h * (gdofp(P, nd, e, 1, j, M->dkd[j]) + h * gdofp(P, nd, e, 0, j, M->dkp[j])) * qd[j];
      dff[(size_t)j * N + e] = f;
    }
  }
  // ---------------- CRBA (lane = body): row of body i's dof, and its base block (entries of dofs on no common
  // path stay zero)
  for (int t = lane; t < nv * kGMaxV; t += kGW) Ml[t] = 0.f;
  __syncthreads();
  for (int i = lane; i < nb; i += kGW) {
    if (i == 0) {
      if (!fb) {
        const SpI& I0 = B.Ic[0];
        const float* hh = I0.h;
        const float hx[9] = {0.f, -hh[2], hh[1], hh[2], 0.f, -hh[0], -hh[1], hh[0], 0.f};
        const float Iv[9] = {I0.I[0], I0.I[3], I0.I[4], I0.I[3], I0.I[1], I0.I[5], I0.I[4], I0.I[5], I0.I[2]};
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) {
            Ml[a * kGMaxV + b] = Iv[3 * a + b];
            Ml[(3 + a) * kGMaxV + 3 + b] = a == b ? I0.m : 0.f;
            Ml[a * kGMaxV + 3 + b] = hx[3 * a + b];
            Ml[(3 + b) * kGMaxV + a] = hx[3 * a + b];
          }
      }
      continue;
    }
    const int d = L->bdof[i], di = nbase + d;
    float Fi[6];
    spi_mul(B.Ic[i], B.S[i], Fi);
    float dd = dot6(B.S[i], Fi) + M->armature[d];
    if (P.any_drive && dimpl[d] != 0.f)
      dd += h * (gdofp(P, nd, e, 1, d, M->dkd[d]) + h * gdofp(P, nd, e, 0, d, M->dkp[d]));
    Ml[di * kGMaxV + di] = dd;
    for (int jb = L->parent[i]; jb > 0; jb = L->parent[jb]) {
      const int dj = nbase + L->bdof[jb];
      const float v = dot6(B.S[jb], Fi);
      Ml[di * kGMaxV + dj] = v;
      Ml[dj * kGMaxV + di] = v;
    }
    if (!fb)
      for (int k = 0; k < 6; ++k) { Ml[di * kGMaxV + k] = Fi[k]; Ml[k * kGMaxV + di] = Fi[k]; }
  }
  __syncthreads();
  // ---------------- Cholesky M = L L^T (lower, in place), column by column, lane = row
  for (int j = 0; j < nv; ++j) {
    float d = Ml[j * kGMaxV + j];
    for (int k = 0; k < j; ++k) d -= Ml[j * kGMaxV + k] * Ml[j * kGMaxV + k];
    d = sqrtf(d > 0.f ? d : 1e-30f);
    for (int i = j + 1 + lane; i < nv; i += kGW) {
      float t = Ml[i * kGMaxV + j];
      for (int k = 0; k < j; ++k) t -= Ml[i * kGMaxV + k] * Ml[j * kGMaxV + k];
      Ml[i * kGMaxV + j] = t / d;
    }
    __syncthreads();
    if (lane == 0) Ml[j * kGMaxV + j] = d;
    __syncthreads();
  }
  auto chol_solve = [&](const float* b, float* x, int stride) {  // x = M^-1 b (one lane, vectors at stride)
    float y[kGMaxV];
    for (int i = 0; i < nv; ++i) {
      float t = b[i * stride];
      for (int k = 0; k < i; ++k) t -= Ml[i * kGMaxV + k] * y[k];
      y[i] = t / Ml[i * kGMaxV + i];
    }
    for (int i = nv - 1; i >= 0; --i) {
      float t = y[i];
      for (int k = i + 1; k < nv; ++k) t -= Ml[k * kGMaxV + i] * x[k * stride];
      x[i * stride] = t / Ml[i * kGMaxV + i];
    }
  };
  // ---------------- free velocity (lane 0)
  if (lane == 0) {
    float acc[kGMaxV];
    chol_solve(rhs, acc, 1);
    for (int k = 0; k < nv; ++k) nuf[k] = nu[k] + h * acc[k];
    if (!fb) {
      float wxp[3];
      cross3(&nu[0], &nu[3], wxp);
      for (int k = 0; k < 3; ++k) nuf[3 + k] += h * wxp[k];
    }
  }
  __syncthreads();

  // ---------------- rows: joint limits (dof order), then plane contacts (candidate order), 3 rows each
  int nlim = 0;
  {
    bool on = false;
    float sg = 0.f, sep = 0.f;
    if (lane < nd && P.any_limits) {
      const float lo = gdofp(P, nd, e, 3, lane, M->lower[lane]), hi = gdofp(P, nd, e, 4, lane, M->upper[lane]);
      const bool lim = P.dof_env ? lo < hi : M->has_lim[lane] != 0;
      if (lim) {
        const float dl = q[lane] - lo, dh = hi - q[lane];
        on = dl < P.limit_margin || dh < P.limit_margin;
        sg = dl <= dh ? 1.f : -1.f;
        sep = dl <= dh ? dl : dh;
      }
    }
    const unsigned long long bal = __ballot(on);
    const int slot = __popcll(bal & ((1ull << lane) - 1ull));
    if (on) {
      rowi[2 * slot] = 0;
      rowi[2 * slot + 1] = lane;
      rsep[slot] = sep;
      rsg[slot] = sg;
    }
    nlim = __popcll(bal);
  }
  // (full form) candidate c's body-frame point: a hull slot reads its manifold vertex; false = no such vertex
  auto cand_point = [&](int c, float* pt) {
    if constexpr (FEAT) {
      const int dy = G->cdyn[c];
      if (dy >= 0) {
        const int sh = G->cshape[c];
        for (int k = 0; k < 3; ++k) pt[k] = X.hp[4 * sh + (dy & 3)][k];
        return dy < X.hn[sh];
      }
    }
    for (int k = 0; k < 3; ++k) pt[k] = M->cpoint[c][k];
    return true;
  };
  int nrows = nlim;
  for (int c0 = 0; c0 < G->nc; c0 += kGW) {
    const int c = c0 + lane;
    bool act = false;
    float dist = 0.f;
    if (c < G->nc && P.has_ground) {
      const int b = G->cbody[c];
      float x[3];
      if constexpr (FEAT) {  // a hull slot's point is the manifold's vertex, absent beyond the manifold's count
        float pt[3];
        const bool have = cand_point(c, pt);
        mat3vec(B.R[b], pt, x);
        dist = root[2] + B.P[b][2] + x[2] - M->cradius[c];
        act = have && dist < P.contact_offset;
      } else {
        mat3vec(B.R[b], M->cpoint[c], x);
        dist = root[2] + B.P[b][2] + x[2] - M->cradius[c];
        act = dist < P.contact_offset;
      }
    }
    const unsigned long long bal = __ballot(act);
    const int slot = nrows + 3 * __popcll(bal & ((1ull << lane) - 1ull));
    if (act) {
      const float m = 0.5f * (mu[(size_t)G->cshape[c] * N + e] + P.ground_mu);
      for (int rr = 0; rr < 3; ++rr) {
        rowi[2 * (slot + rr)] = 1 + rr;
        rowi[2 * (slot + rr) + 1] = c;
        rsep[slot + rr] = dist - P.rest_offset;
        rmu[slot + rr] = m;
      }
    }
    nrows += 3 * __popcll(bal);
  }
  const int nground = nrows;  // rows [nlim, nground): ground contacts; [nground, nrows): self-contacts
  if constexpr (FEAT) {
    // self-contact rows after the ground rows, pool order: normal, tangent 1, tangent 2 (id = nc + pool slot)
    for (int t = lane; t < 3 * npc; t += kGW) {
      const int p = t / 3;
      rowi[2 * (nrows + t)] = 1 + (t - 3 * p);
      rowi[2 * (nrows + t) + 1] = G->nc + p;
      rsep[nrows + t] = X.pool[kGPE * p + kPoolSep];
      rmu[nrows + t] = X.pool[kGPE * p + kPoolMu];
    }
    nrows += 3 * npc;
  }
  __syncthreads();
  // Jacobian rows (lane = column k): a limit row is +-e_dof; a contact row's direction d (normal z, tangents x, y
  // for the plane) times the velocity of the contact point xc = x - r n over the candidate body's path
  for (int r = 0; r < nrows; ++r) {
    const int kind = rowi[2 * r], id = rowi[2 * r + 1];
    float* Jr = Jw + (size_t)r * nv;
    for (int k = lane; k < nv; k += kGW) {
      float v = 0.f;
      if (kind == 0) {
        v = k == nbase + id ? rsg[r] : 0.f;
      } else if (FEAT && r >= nground) {
        // self-contact: d . (v_A(x) - v_B(x)) -- S_i's velocity at x where body i is on A's path, minus it on B's
        // (a common ancestor's column and the base columns cancel)
        if constexpr (FEAT) {
          const float* o = X.pool + kGPE * (id - G->nc);
          if (k >= nbase) {
            const int i = L->dbody[k - nbase];
            const int ba = (int)o[kPoolBA], bb = (int)o[kPoolBB];
            const float coef = (float)((L->anc_mask[ba] >> i) & 1u) - (float)((L->anc_mask[bb] >> i) & 1u);
            if (coef != 0.f) {
              const float* d = o + (kind == 1 ? kPoolN : (kind == 2 ? kPoolT1 : kPoolT2));
              float vx[3];
              cross3(B.S[i], o + kPoolX, vx);
              for (int a = 0; a < 3; ++a) vx[a] += B.S[i][3 + a];
              v = coef * dot3f(d, vx);
            }
          }
        }
      } else {
        const int b = G->cbody[id];
        float x[3];
        if constexpr (FEAT) {
          float pt[3];
          cand_point(id, pt);
          mat3vec(B.R[b], pt, x);
        } else {
          mat3vec(B.R[b], M->cpoint[id], x);
        }
        const float xc[3] = {B.P[b][0] + x[0], B.P[b][1] + x[1], B.P[b][2] + x[2] - M->cradius[id]};
        const int ax = kind == 1 ? 2 : (kind == 2 ? 0 : 1);  // normal z, tangent 1 x, tangent 2 y
        if (k < nbase) {
          if (k < 3) {  // d . (w x xc) = w . (xc x d): column k of xc x e_ax
            const float ea[3] = {ax == 0 ? 1.f : 0.f, ax == 1 ? 1.f : 0.f, ax == 2 ? 1.f : 0.f};
            float t[3];
            cross3(xc, ea, t);
            v = t[k];
          } else {
            v = (k - 3) == ax ? 1.f : 0.f;
          }
        } else {
          const int i = L->dbody[k - nbase];
          if ((L->anc_mask[b] >> i) & 1u) {
            float t[3];
            cross3(B.S[i], xc, t);
            v = B.S[i][3 + ax] + t[ax];
          }
        }
      }
      Jr[k] = v;
    }
  }
  __syncthreads();
  // responses W = M^-1 J^T and the Delassus diagonals (lane = row)
  for (int r = lane; r < nrows; r += kGW) {
    const float* Jr = Jw + (size_t)r * nv;
    float* Wr = Ww + (size_t)r * nv;
    chol_solve(Jr, Wr, 1);
    float d = 0.f;
    for (int k = 0; k < nv; ++k) d += Jr[k] * Wr[k];
    if constexpr (FEAT) {
      if (r >= nground && !(d > GS_MIN_RESPONSE)) d = 0.f;  // a self-contact row no dof can separate: no impulse
    }
    rD[r] = d;
    rlam[r] = 0.f;
  }
  __syncthreads();

  // ---------------- projected Gauss-Seidel / TGS sub-steps (lane = velocity component)
  float v = lane < nv ? nuf[lane] : 0.f;
  float dxs = 0.f, vpos = v;
  const bool tgs = P.tgs != 0;
  const float hs = tgs ? h / (float)P.pos_iters : h;
  const int iters = P.pos_iters + P.vel_iters;
  for (int it = 0; it < iters; ++it) {
    const bool pos = it < P.pos_iters;
    const float hd = pos ? hs : h;
    for (int r = 0; r < nrows; ++r) {
      const int kind = rowi[2 * r];
      const float* Jr = Jw + (size_t)r * nv;
      const float* Wr = Ww + (size_t)r * nv;
      const float jk = lane < nv ? Jr[lane] : 0.f;
      const float u = wave_sum(jk * v);
      float ln;
      if (kind <= 1) {  // limit or contact normal: unilateral, separation target
        float s = rsep[r];
        if (tgs) s += wave_sum(jk * dxs);
        float target;
        if (s >= 0.f) target = -s / hd;
        else if (pos) target = fminf(-s / h, P.max_depen_vel);  // (TGS: the push-out spread over the step)
        else target = 0.f;
        ln = rD[r] > 0.f ? rlam[r] + (target - u) / rD[r] : rlam[r];
        ln = fmaxf(ln, 0.f);
      } else {  // friction: |lambda_t| <= mu lambda_n of the contact's normal row (two rows above or one)
        const int nr0 = r - (kind - 1);
        const float lim = rmu[r] * rlam[nr0];
        ln = rD[r] > 0.f ? rlam[r] - u / rD[r] : rlam[r];
        ln = clampf(ln, -lim, lim);
      }
      const float dl = ln - rlam[r];
      rlam[r] = ln;  // (every lane the same value: a one-wave workgroup reads and writes LDS in program order)
      if (lane < nv) v += Wr[lane] * dl;
    }
    if (tgs && pos) dxs += hs * v;
    if (it == P.pos_iters - 1) vpos = tgs ? dxs / h : v;
  }
  if (P.pos_iters <= 0) vpos = v;
  // joint velocity clamp
  if (lane >= nbase && lane < nv) {
    const int j = lane - nbase;
    const float vm = gdofp(P, nd, e, 5, j, M->vmax[j]);
    if (vm > 0.f) { v = clampf(v, -vm, vm); vpos = clampf(vpos, -vm, vm); }
  }
  // ---------------- full form: force sensors on leaf bodies (gs_solver.h's T::SENS block), lane =
  // body.  The wrench through the parent joint, f = I_b a_b + v_b x* I_b v_b - f_contact, with a_b = A_b (velocity
  // products + gravity, already in B.F) + the base's acceleration + sum over the path of S_k qdd_k, qdd = (nu_new -
  // nu) / h; a leaf's B.F / B.Ic are still its own RNEA force / inertia.  About the body origin, in body axes.
  if constexpr (FEAT) {
    if (sens && M->nsens > 0) {
      const float inv_h = 1.f / h;
      if (lane < nv) rhs[lane] = (v - nu[lane]) * inv_h;  // (rhs is free after the free velocity)
      __syncthreads();
      const int b = lane;
      const int si = (b > 0 && b < nb) ? M->sens_of_body[b] : -1;
      if (si >= 0) {
        float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (!fb) {
          float wxp[3];
          cross3(&nu[0], &nu[3], wxp);
          for (int k = 0; k < 3; ++k) { a[k] = rhs[k]; a[3 + k] = rhs[3 + k] - wxp[k]; }
        }
        for (int kk = 1; kk < nb; ++kk)
          if ((L->anc_mask[b] >> kk) & 1u) {
            const float qdd = rhs[nbase + L->bdof[kk]];
            for (int k = 0; k < 6; ++k) a[k] += B.S[kk][k] * qdd;
          }
        float ia[6], f[6];
        spi_mul(B.Ic[b], a, ia);
        for (int k = 0; k < 6; ++k) f[k] = B.F[b][k] + ia[k];
        for (int r = nlim; r < nground; r += 3) {
          const int c = rowi[2 * r + 1];
          if (G->cbody[c] != b) continue;
          float pt[3], x[3], n3[3];
          cand_point(c, pt);
          mat3vec(B.R[b], pt, x);
          x[0] += B.P[b][0]; x[1] += B.P[b][1]; x[2] += B.P[b][2] - M->cradius[c];
          const float fc[3] = {rlam[r + 1] * inv_h, rlam[r + 2] * inv_h, rlam[r] * inv_h};
          cross3(x, fc, n3);
          for (int k = 0; k < 3; ++k) { f[k] -= n3[k]; f[3 + k] -= fc[k]; }
        }
        for (int r = nground; r < nrows; r += 3) {
          const float* o = X.pool + kGPE * (rowi[2 * r + 1] - G->nc);
          const int ba = (int)o[kPoolBA], bb = (int)o[kPoolBB];
          if (ba != b && bb != b) continue;
          const float sg = ba == b ? inv_h : -inv_h;
          float fc[3], n3[3];
          for (int k = 0; k < 3; ++k)
            fc[k] = sg * (rlam[r] * o[kPoolN + k] + rlam[r + 1] * o[kPoolT1 + k] + rlam[r + 2] * o[kPoolT2 + k]);
          cross3(o + kPoolX, fc, n3);
          for (int k = 0; k < 3; ++k) { f[k] -= n3[k]; f[3 + k] -= fc[k]; }
        }
        float xf[3], tq[3];
        cross3(B.P[b], &f[3], xf);
        for (int k = 0; k < 3; ++k) tq[k] = f[k] - xf[k];
        const float* Rb = B.R[b];
        for (int k = 0; k < 3; ++k) {
          sens[(size_t)(6 * si + k) * N + e] = Rb[k] * f[3] + Rb[3 + k] * f[4] + Rb[6 + k] * f[5];
          sens[(size_t)(6 * si + 3 + k) * N + e] = Rb[k] * tq[0] + Rb[3 + k] * tq[1] + Rb[6 + k] * tq[2];
        }
      }
      __syncthreads();
    }
  }
  // ---------------- integrate and store
  if (lane < nv) { nu[lane] = v; nuf[lane] = vpos; }  // (nu: new velocity, nuf: position-phase velocity)
  __syncthreads();
  if (lane == 0) {
    if (!fb) {
      for (int k = 0; k < 3; ++k) root[k] += h * nuf[3 + k];
      const float wx = nuf[0], wy = nuf[1], wz = nuf[2];
      float x = root[3], y = root[4], z = root[5], w = root[6];
      const float hh = 0.5f * h;
      const float dx = hh * (w * wx + wy * z - wz * y), dy = hh * (w * wy + wz * x - wx * z);
      const float dz = hh * (w * wz + wx * y - wy * x), dw = -hh * (wx * x + wy * y + wz * z);
      x += dx; y += dy; z += dz; w += dw;
      const float n = 1.f / sqrtf(x * x + y * y + z * z + w * w);
      root[3] = x * n; root[4] = y * n; root[5] = z * n; root[6] = w * n;
      for (int k = 0; k < 3; ++k) { root[10 + k] = nu[k]; root[7 + k] = nu[3 + k]; }
    }
    for (int j = 0; j < nd; ++j) {
      q[j] += h * nuf[nbase + j];
      qd[j] = nu[nbase + j];
    }
  }
  __syncthreads();
  if (lane < 13) st[(size_t)lane * N + e] = root[lane];
  for (int j = lane; j < nd; j += kGW) {
    st[(size_t)(13 + j) * N + e] = q[j];
    st[(size_t)(13 + nd + j) * N + e] = qd[j];
    if (dff && P.any_drive && dimpl[j] != 0.f)  // (the lane that stored dof j's first half)
      dff[(size_t)j * N + e] -= h * (gdofp(P, nd, e, 1, j, M->dkd[j]) + h * gdofp(P, nd, e, 0, j, M->dkp[j])) * qd[j];
  }
  // net contact force per reported link, sum of lambda / h over the contact's rows in its frame (plane: z, x, y)
  if (cf) {
    for (int l = lane; l < L->nr; l += kGW) {
      float f[3] = {0.f, 0.f, 0.f};
      for (int r = nlim; r < nground; r += 3) {
        if (G->clink[rowi[2 * r + 1]] != l) continue;
        f[0] += rlam[r + 1] / h;
        f[1] += rlam[r + 2] / h;
        f[2] += rlam[r] / h;
      }
      if constexpr (FEAT) {  // a self-contact's force: + on link A, - on link B
        for (int r = nground; r < nrows; r += 3) {
          const float* o = X.pool + kGPE * (rowi[2 * r + 1] - G->nc);
          const int la = (int)o[kPoolLA], lb = (int)o[kPoolLB];
          if (la != l && lb != l) continue;
          const float sg = la == l ? 1.f : -1.f;
          for (int k = 0; k < 3; ++k)
            f[k] += sg * ((rlam[r] * o[kPoolN + k] + rlam[r + 1] * o[kPoolT1 + k] + rlam[r + 2] * o[kPoolT2 + k]) / h);
        }
      }
      for (int k = 0; k < 3; ++k) cf[(size_t)(3 * l + k) * N + e] = f[k];
    }
  }
  __syncthreads();
}

constexpr int kGVec = 3 * kGMaxV + 13 + 4 * GS_MAXD;
template <bool FEAT>
constexpr size_t kGLds = sizeof(GBody) + sizeof(float) * (kGMaxV * kGMaxV + 5 * kGRows<FEAT> + kGVec) +
                         sizeof(int) * 2 * kGRows<FEAT> + (FEAT ? sizeof(GFeat) : 0);
static_assert(kGLds<true> <= 160 * 1024 && kGLds<false> <= 160 * 1024, "static LDS beyond a CU's 160 KB");

template <bool FEAT>
__global__ __launch_bounds__(kGW) void k_simulate_generic(const DevModel* __restrict__ M, DevParams P, SimBuffers Bf,
                                                          const float* __restrict__ tau) {
  __shared__ GBody B;
  __shared__ float Ml[kGMaxV * kGMaxV];
  __shared__ float rowf[5 * kGRows<FEAT>];
  __shared__ int rowi[2 * kGRows<FEAT>];
  __shared__ float vec[kGVec];
  __shared__ std::conditional_t<FEAT, GFeat, GNoFeat> X;
  const int e = blockIdx.x;
  if (e >= Bf.N) return;
  const DevLinks* L = P.gen_links;
  const GenTopo* G = P.gen;
  const int nv = (L->fixed_base ? 0 : 6) + L->nd;
  const size_t ws_per_env = (size_t)2 * (3 * G->nc + L->nd + 3 * G->npool) * nv;  // generic_ws_floats
  float* ws = Bf.rows + ws_per_env * e;
  for (int s = 0; s < P.substeps; ++s) {
    const bool last = s == P.substeps - 1;
    generic_substep<FEAT>(M, L, G, P, Bf.state, Bf.mu, Bf.N, e, tau ? tau + (size_t)e * L->nd : nullptr, ws,
                          (last && P.collect) ? Bf.cf : nullptr, last ? Bf.sens : nullptr, B, Ml, rowf, rowi, vec, X,
                          last ? P.dof_force : nullptr);
  }
}

// gs_debug_self_contacts on the runtime-sized kernel: the pool self_contacts_wave finds from the current state,
// out [N][npool][10] = x (3) n (3) separation friction body a body b, count [N] (gs_physics_impl.h k_dbg_pool)
__global__ __launch_bounds__(kGW) void k_dbg_pool_generic(const DevModel* __restrict__ M, DevParams P, SimBuffers Bf,
                                                          float* __restrict__ out, int* __restrict__ count) {
  __shared__ GBody B;
  __shared__ GFeat X;
  __shared__ float qs[13 + GS_MAXD];
  const int e = blockIdx.x, lane = threadIdx.x, N = Bf.N;
  if (e >= N) return;
  const DevLinks* L = P.gen_links;
  const GenTopo* G = P.gen;
  const int nb = L->nb, nd = L->nd;
  if (lane < 13) qs[lane] = Bf.state[(size_t)lane * N + e];
  for (int j = lane; j < nd; j += kGW) qs[13 + j] = Bf.state[(size_t)(13 + j) * N + e];
  __syncthreads();
  if (lane == 0) {  // body poses as generic_substep forms them
    const float* root = qs;
    const float qn = 1.f / sqrtf(root[3] * root[3] + root[4] * root[4] + root[5] * root[5] + root[6] * root[6]);
    const float q4[4] = {root[3] * qn, root[4] * qn, root[5] * qn, root[6] * qn};
    quat_to_mat(q4, B.R[0]);
    B.P[0][0] = B.P[0][1] = B.P[0][2] = 0.f;
    for (int i = 1; i < nb; ++i) {
      const int pa = L->parent[i];
      float RJ[9], t[3], aw[3];
      mat3mul(B.R[pa], M->jR[i], RJ);
      mat3vec(B.R[pa], M->jt[i], t);
      for (int k = 0; k < 3; ++k) B.P[i][k] = B.P[pa][k] + t[k];
      mat3vec(RJ, M->jaxis[i], aw);
      const float qj = qs[13 + L->bdof[i]];
      if (L->jkind[i] == 1) {
        float Rq[9];
        axis_rot(M->jaxis[i], qj, Rq);
        mat3mul(RJ, Rq, B.R[i]);
      } else {
        for (int k = 0; k < 9; ++k) B.R[i][k] = RJ[k];
        for (int k = 0; k < 3; ++k) B.P[i][k] += aw[k] * qj;
      }
    }
  }
  __syncthreads();
  const int n = self_contacts_wave(M, G, P, Bf.mu, N, e, B, X, lane);
  const int npk = G->npool > 0 ? G->npool : 1;
  for (int t = lane; t < n * 10; t += kGW) {
    const int p = t / 10, k = t - 10 * p;
    const int src = k < 6 ? k : kPoolSep + (k - 6);  // x, n | separation, friction, body a, body b: contiguous
    static_assert(kPoolMu == kPoolSep + 1 && kPoolBA == kPoolSep + 2 && kPoolBB == kPoolSep + 3, "pool entry layout");
    out[((size_t)e * npk + p) * 10 + k] = X.pool[kGPE * p + src];
  }
  if (lane == 0) count[e] = n;
}

__global__ void k_generic_pd_torque(const DevParams P, SimBuffers Bf, PdDev A, int nd, int first, float* tau) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bf.N * nd) return;
  const int e = t / nd, j = t - e * nd;
  const float q = first ? A.dof_state_in[(size_t)t * 2] : Bf.state[(size_t)(13 + j) * Bf.N + e];
  const float qd = first ? A.dof_state_in[(size_t)t * 2 + 1] : Bf.state[(size_t)(13 + nd + j) * Bf.N + e];
  const float a = A.actions[t];
  tau[t] = clampf(A.kp * (A.scale * a + A.default_pos[j] - q) - A.kd * qd, -A.tlim, A.tlim);
  (void)P;
}

}  // namespace

hipError_t launch_sim_generic(const DevModel* M, const DevParams& P, const SimBuffers& B, const float* tau,
                              hipStream_t st) {
  if (!P.gen || !P.gen_links || !B.rows) return hipErrorInvalidValue;
  if (P.has_terrain) return hipErrorNotSupported;
  if (B.N <= 0) return hipSuccess;
  // the full form only where the sim has a hull candidate, a force sensor or self-collision: every other robot runs
  // the plain form, which carries none of their code, registers or LDS
  if (P.gen_feat || P.self_collide)
    hipLaunchKernelGGL(k_simulate_generic<true>, dim3(B.N), dim3(kGW), 0, st, M, P, B, tau);
  else
    hipLaunchKernelGGL(k_simulate_generic<false>, dim3(B.N), dim3(kGW), 0, st, M, P, B, tau);
  return hipGetLastError();
}

hipError_t launch_dbg_pool_generic(const DevModel* M, const DevParams& P, const SimBuffers& B, int mode, float* out,
                                   int* count, hipStream_t st) {
  if (mode != 0 || !P.gen || !P.gen_links) return hipErrorInvalidValue;
  if (B.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dbg_pool_generic, dim3(B.N), dim3(kGW), 0, st, M, P, B, out, count);
  const hipError_t e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(st);
  return e != hipSuccess ? e : e2;
}

// The fused PD decimation step on the generic kernel: per decimation step one PD-torque launch (into
// torques_out) and one simulate launch, then the extra simulates with the last torques, and the dof / root /
// contact tensors by the refresh kernels (the compiled kernels' PdDev contract, gs_internal.h).
hipError_t launch_pd_generic(const DevModel* M, const DevParams& P, const SimBuffers& B, const PdDev& A,
                             hipStream_t st) {
  if (!P.gen || !P.gen_links) return hipErrorInvalidValue;
  const int nd = P.gen_nd;
  const int n = B.N * nd, blocks = (n + 255) / 256;
  for (int d = 0; d < A.decimation; ++d) {
    if (n > 0)
      hipLaunchKernelGGL(k_generic_pd_torque, dim3(blocks), dim3(256), 0, st, P, B, A, nd, d == 0 ? 1 : 0,
                         A.torques_out);
    if (hipError_t e = launch_sim_generic(M, P, B, A.torques_out, st); e != hipSuccess) return e;
  }
  if (A.dof_out)
    if (hipError_t e = launch_refresh_dof(B.state, B.N, nd, A.dof_out, st); e != hipSuccess) return e;
  for (int x = 0; x < A.extra; ++x)
    if (hipError_t e = launch_sim_generic(M, P, B, A.torques_out, st); e != hipSuccess) return e;
  if (A.root_out)
    if (hipError_t e = launch_refresh_root(B.state, B.N, nd, &M->root_com[0], A.root_out, st); e != hipSuccess) return e;
  if (A.cf_out)
    if (hipError_t e = launch_refresh_contact(B.cf, B.N, P.gen_nr, A.cf_out, st); e != hipSuccess) return e;
  if (A.actions_copy && n > 0)
    if (hipError_t e = hipMemcpyAsync(A.actions_copy, A.actions, sizeof(float) * n, hipMemcpyDeviceToDevice, st);
        e != hipSuccess)
      return e;
  return hipGetLastError();
}
