// gs_capi.hip -- the C ABI of libgymsim.so (include/gymsim.h).
//
// Host-side object that replaces the Isaac Gym `sim` handle: it owns the
// float32 device copy of the articulation model, the parsed SimParams and the
// selected kernel specialisation, and binds the caller-owned (torch) device
// buffers that hold the sim state.  All launches are stream ordered; nothing
// here synchronises the host except create/set_model/prepare.
//
// A sim created with device < 0 is the host backend (gs_host.hip, the reference's
// sim_device=cpu pipeline): same entry points, caller-owned HOST buffers, the solver
// runs on a thread pool inside the call, `stream` is ignored, no HIP call is made.
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "gs_internal.h"
#include "gs_kernel_choice.h"
#include "gs_model_pack.h"
#include "gs_terrain_build.h"
#include "../../include/gymsim.h"

namespace {
thread_local std::string g_err;

int fail(const char* fmt, const char* arg = nullptr) {
  // sized to the message: a topology signature runs to several hundred characters (Hound_new: 84 candidates, 17
  // links), and the reason that follows it must not be cut off
  const char* a = arg ? arg : "";
  const int n = std::snprintf(nullptr, 0, fmt, a);
  std::string s(n > 0 ? (size_t)n : 0, '\0');
  if (n > 0) std::snprintf(&s[0], (size_t)n + 1, fmt, a);
  g_err = s;
  return -1;
}
int hip_fail(hipError_t e, const char* where) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), "%s: %s", where, hipGetErrorString(e));
  g_err = buf;
  return -1;
}

const TopoEntry* find_topology(const gs_model_desc* m) {
  const std::string sig = model_signature(m);
  for (int i = 0; i < g_num_topologies; ++i)
    if (sig == g_topologies[i].sig) return &g_topologies[i];
  return nullptr;
}

// The DOF force tensor after a lane-team launch (DevParams::dof_force): the team runs only sims
// with no drive gains and no per-actor table, so the tensor is the actuation force clamped to the asset's effort,
// as the team's own substep clamps it.  src [N][nd] or null (= 0) -> out [nd][N]; consecutive threads are
// consecutive envs, so the stores are full rows.
__global__ void k_team_dof_force(const float* __restrict__ src, const float* __restrict__ effort, int N, int nd,
                                 float* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)N * nd) return;
  const int j = (int)(t / N), e = (int)(t - (long)j * N);
  float f = src ? src[(size_t)e * nd + j] : 0.f;
  const float ef = effort[j];
  if (ef > 0.f) f = fminf(fmaxf(f, -ef), ef);
  out[t] = f;
}
// refresh_dof_force_tensor: [nd][N] -> [N*nd]
__global__ void k_refresh_dof_force(const float* __restrict__ soa, int N, int nd, float* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)N * nd) return;
  const int e = (int)(t / nd), j = (int)(t - (long)e * nd);
  out[t] = soa[(size_t)j * N + e];
}
}  // namespace

struct gs_sim {
  int device = 0;
  gs_sim_params params{};
  DevParams dp{};
  bool has_ground = false;
  bool disable_gravity = false;  // gs_sim_set_disable_gravity: the asset's AssetOptions.disable_gravity
  float ground_mu = 1.f;
  const TopoEntry* topo = nullptr;
  const TeamEntry* team = nullptr;  // the topology's lane-team kernels (gs_team.hip), null if it has none
  // the launch pointers of `variant` (set_variant): what gs_sim_simulate / gs_sim_pd_step call
  launch_sim_fn sim_fn = nullptr;
  launch_pd_fn pd_fn = nullptr;
  int variant = 0;  // the kernel form in force (gs_kernel_choice.h): 1 lane, 2 team, 3 host, 4 runtime-sized
  // the asset-wide (uniform) drive / limit flags; a bound per-actor property table overrides them in dp
  int uni_any_drive = 0, uni_any_limits = 0;
  // the runtime-sized kernel (gs_generic.hip, kernel_variant 4): the topology entry it stands in for and its
  // candidate tables on the device
  TopoEntry gen_entry{};  // (variant 4: topo points here)
  GenTopo* d_gen = nullptr;
  int env_any_drive = 0, env_any_limits = 0;
  DevModel* d_model = nullptr;
  DevModel h_model{};             // host copy (sensors are added after set_model)
  DevLinks* d_links = nullptr;    // link kinematics tables (gs_kinematics.hip)
  int nr = 0, nv = 0;
  std::vector<int> parent;
  float* sens = nullptr;          // [6*nsens][N]
  int nb = 0, nd = 0, nc = 0, ns = 0;
  int N = 0;
  float* state = nullptr;
  const float* mu = nullptr;
  float* cf = nullptr;
  bool timing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  // terrain mesh tables (gs_terrain.h; gs_terrain_build.h TerrainTables order: vertices, cell words, block
  // maxima, 4 x 4 maxima, cell records): on the device, or the host backend's own
  void* d_terr[5] = {};
  float* d_rows = nullptr;        // contact-row tiles of the GLOBAL-row kernels (TopoEntry::row_floats)
  size_t rows_cap = 0;            // floats allocated
  // host backend (device < 0)
  bool host = false;
  HostPool* pool = nullptr;
  const HostTopoEntry* htopo = nullptr;
  DevLinks h_links{};
  TerrainTables h_terr;
  double host_ms = -1.0;          // wall time of the last simulate / pd_step (timing enabled)
  const DevModel* model() const { return host ? &h_model : d_model; }
  const DevLinks* links() const { return host ? &h_links : d_links; }
};

// The gravity every kernel form sees (DevParams::g; the bias pass of the lane, team, runtime-sized and host forms and
// the DOF-force pass that reuses its result): the sim parameter, or zero with the asset's gravity switched off
static void fill_gravity(gs_sim* s) {
  for (int k = 0; k < 3; ++k) s->dp.g[k] = s->disable_gravity ? 0.f : (float)s->params.gravity[k];
}

// The launch pointers of a kernel form (under variant 4, s->topo is the runtime-sized kernel's own entry)
static void set_variant(gs_sim* s, int variant) {
  s->variant = variant;
  s->sim_fn = variant == 3 ? nullptr : variant == 2 ? s->team->sim : s->topo->sim;
  s->pd_fn = variant == 3 ? nullptr : variant == 2 ? s->team->pd : s->topo->pd;
}

// The kernel form for the flags a setter is about to put in force (gs_kernel_choice.h); the setter commits
// them, and set_variant, only where this is no refusal
static KernelChoice choose(const gs_sim* s, int any_drive, bool dof_env) {
  return kernel_choice({s->host, s->topo != &s->gen_entry, s->team != nullptr, s->uni_any_limits,
                        s->params.kernel_variant, any_drive, dof_env});
}

extern "C" {

int gs_abi_version(void) { return GS_ABI_VERSION; }
const char* gs_last_error(void) { return g_err.c_str(); }

int gs_topology_supported(const gs_model_desc* model) { return find_topology(model) != nullptr; }

gs_sim* gs_sim_create(int device, const gs_sim_params* p) {
  if (!p) { fail("gs_sim_create: null params"); return nullptr; }
  if (!(p->dt > 0)) { fail("gs_sim_create: dt must be > 0"); return nullptr; }
  gs_sim* s = nullptr;
  if (device < 0) {
    s = new gs_sim();
    s->host = true;
    s->device = -1;
    // physx.num_threads (cfg/config.yaml:30): worker threads; 0 runs the solver on the caller only
    s->pool = host_pool_create(p->num_threads > 0 ? p->num_threads : 1);
  } else {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
      fail("gs_sim_create: no HIP device %s", std::to_string(device).c_str());
      return nullptr;
    }
    if (hipError_t e = hipSetDevice(device); e != hipSuccess) {
      hip_fail(e, "gs_sim_create hipSetDevice");
      return nullptr;
    }
    s = new gs_sim();
    s->device = device;
  }
  s->params = *p;
  const int sub = p->substeps > 0 ? p->substeps : 1;
  s->dp.h = (float)(p->dt / sub);
  s->dp.substeps = sub;
  fill_gravity(s);
  s->dp.pos_iters = p->num_position_iterations;
  s->dp.vel_iters = p->num_velocity_iterations;
  s->dp.contact_offset = (float)p->contact_offset;
  s->dp.rest_offset = (float)p->rest_offset;
  s->dp.max_depen_vel = (float)p->max_depenetration_velocity;
  s->dp.tgs = p->solver_type == 1 && p->num_position_iterations > 0 ? 1 : 0;
  s->dp.collect = p->contact_collection != 0;
  s->dp.limit_margin = (float)(p->joint_limit_margin > 0 ? p->joint_limit_margin : 0.0);
  s->dp.any_limits = 0;
  s->dp.has_ground = 0;
  s->dp.ground_mu = 1.f;
  // A/B switch of the lane-team kernels' envs per wave, read once here; unset (or any other value): the default
  if (const char* v = std::getenv("GS_TEAM_ENVS_PER_WAVE")) {
    const int w = std::atoi(v);
    s->dp.team_epw = w == 16 || w == 8 || w == 4 ? w : 0;
  }
  // A/B switch of the row lanes of the 4-envs-per-wave plane form (0 / 1), read once here; unset: the default
  s->dp.team_row_lanes = -1;
  if (const char* v = std::getenv("GS_TEAM_ROW_LANES")) {
    if (v[0] == '0' || v[0] == '1') s->dp.team_row_lanes = v[0] - '0';
  }
  // A/B switch of the row-lane form's resident sweeps (0 / 1), read once here; unset: the default
  s->dp.team_resident = -1;
  if (const char* v = std::getenv("GS_TEAM_RESIDENT_SWEEPS")) {
    if (v[0] == '0' || v[0] == '1') s->dp.team_resident = v[0] - '0';
  }
  return s;
}

void gs_sim_destroy(gs_sim* s) {
  if (!s) return;
  if (s->host) {
    host_pool_destroy(s->pool);
    delete s;
    return;
  }
  // Teardown is best-effort: a failed free cannot be reported through a void API.
  (void)hipSetDevice(s->device);
  if (s->d_model) (void)hipFree(s->d_model);
  if (s->d_links) (void)hipFree(s->d_links);
  for (void* d : s->d_terr)
    if (d) (void)hipFree(d);
  if (s->d_rows) (void)hipFree(s->d_rows);
  if (s->d_gen) (void)hipFree(s->d_gen);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
}

int gs_sim_add_ground(gs_sim* s, double static_friction, double dynamic_friction, double restitution) {
  if (!s) return fail("gs_sim_add_ground: null sim");
  (void)dynamic_friction;
  (void)restitution;
  s->has_ground = true;
  s->dp.has_ground = 1;
  s->dp.ground_mu = (float)static_friction;
  return 0;
}

int gs_sim_add_triangle_mesh(gs_sim* s, const float* vertices, int64_t num_vertices, const uint32_t* triangles,
                             int64_t num_triangles, const double* transform_p, double static_friction,
                             double dynamic_friction, double restitution) {
  (void)dynamic_friction;
  (void)restitution;
  if (!s || !vertices || !triangles) return fail("gs_sim_add_triangle_mesh: null argument");
  if (s->topo) return fail("gs_sim_add_triangle_mesh: call before the model is set (prepare_sim)");
  if (s->dp.has_terrain) return fail("gs_sim_add_triangle_mesh: one triangle mesh per sim");
  TerrainTables tt;
  if (terrain_build(vertices, num_vertices, triangles, num_triangles, transform_p, &tt))
    return fail("%s", tt.err.c_str());
  struct { const void* src; size_t bytes; } tab[5] = {
      {tt.verts.data(), tt.verts.size() * sizeof(float4)}, {tt.cells.data(), tt.cells.size() * sizeof(uint4)},
      {tt.blk.data(), tt.blk.size() * sizeof(float)},      {tt.sq4.data(), tt.sq4.size() * sizeof(float)},
      {tt.rec.data(), tt.rec.size() * sizeof(float4)}};
  const void* p[5];
  if (s->host) {
    for (int k = 0; k < 5; ++k) p[k] = tab[k].src;  // (moving a vector keeps its buffer)
    s->h_terr = std::move(tt);
  } else {
    void* d[5] = {};
    hipError_t e = hipSetDevice(s->device);
    for (int k = 0; k < 5 && e == hipSuccess; ++k) {
      e = hipMalloc(&d[k], tab[k].bytes);
      if (e == hipSuccess) e = hipMemcpy(d[k], tab[k].src, tab[k].bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      for (void* q : d)
        if (q) (void)hipFree(q);
      return hip_fail(e, "gs_sim_add_triangle_mesh");
    }
    for (int k = 0; k < 5; ++k) p[k] = s->d_terr[k] = d[k];
  }
  TerrainDev& T = s->dp.terr;
  T = tt.grid;
  T.v = (const float4*)p[0];
  T.cell = (const uint4*)p[1];
  T.blk = (const float*)p[2];
  T.sq4 = (const float*)p[3];
  T.rec = (const float4*)p[4];
  T.mu = (float)static_friction;
  s->dp.has_terrain = 1;
  return 0;
}

int gs_sim_set_model(gs_sim* s, const gs_model_desc* m) {
  if (!s || !m) return fail("gs_sim_set_model: null argument");
  const int want = s->params.kernel_variant;
  // 1. the compiled topology with its host solver / lane-team kernels (kernel_variant 4 asks a GPU sim for the
  // runtime-sized kernel on a compiled topology too: then it counts as not compiled)
  const TopoEntry* t = want == 4 && !s->host ? nullptr : find_topology(m);
  // 2. the kernels' tables, built aside and committed at the end, so a failure leaves the sim as it was (no
  // half-set topology with a null kernel or link table)
  ModelPack pk;
  if (model_pack(m, t, s->host, s->dp.has_terrain != 0, &pk)) return fail("%s", pk.err.c_str());
  const HostTopoEntry* htopo = nullptr;
  const TeamEntry* team = nullptr;
  if (s->host) {
    for (int i = 0; i < g_num_host_topologies; ++i)
      if (std::strcmp(g_host_topologies[i].sig, t->sig) == 0) htopo = &g_host_topologies[i];
    if (!htopo) return fail("gs_sim_set_model: no host solver for topology %s", t->sig);
  } else if (t) {
    for (int i = 0; i < g_num_team_kernels; ++i)
      if (std::strcmp(g_team_kernels[i].sig, t->sig) == 0 && g_team_kernels[i].sim) team = &g_team_kernels[i];
  }
  // 3. the kernel form (the refusals name the topology where none is compiled, else the entry point)
  const KernelChoice kc = kernel_choice({s->host, t != nullptr, team != nullptr, pk.any_limits, want, s->dp.any_drive,
                                         s->dp.dof_env != nullptr});
  if (!kc.variant) return fail(kc.refusal, t ? "gs_sim_set_model" : model_signature(m).c_str());
  const bool generic = kc.variant == 4;
  // 4. upload and commit
  if (!s->host) {
    if (hipError_t e = hipSetDevice(s->device); e != hipSuccess) return hip_fail(e, "gs_sim_set_model hipSetDevice");
    DevModel* dm = s->d_model;
    DevLinks* dl = s->d_links;
    hipError_t e = hipSuccess;
    if (!dm) e = hipMalloc(&dm, sizeof(DevModel));
    if (e == hipSuccess && !dl) e = hipMalloc(&dl, sizeof(DevLinks));
    // keep whatever was allocated (freed by gs_sim_destroy) even when a later step fails
    s->d_model = dm;
    s->d_links = dl;
    if (e == hipSuccess) e = hipMemcpy(dm, &pk.model, sizeof(DevModel), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dl, &pk.links, sizeof(DevLinks), hipMemcpyHostToDevice);
    if (e == hipSuccess && generic && !s->d_gen) e = hipMalloc(&s->d_gen, sizeof(GenTopo));
    if (e == hipSuccess && generic) e = hipMemcpy(s->d_gen, &pk.gen, sizeof(GenTopo), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "gs_sim_set_model upload");
  }
  s->h_model = pk.model;
  s->h_links = pk.links;
  s->dp.any_limits = pk.any_limits;
  s->uni_any_limits = pk.any_limits;
  s->parent.assign(m->parent, m->parent + m->num_bodies);
  s->gen_entry = pk.gen_entry;
  s->topo = t ? t : &s->gen_entry;
  s->team = team;
  s->htopo = htopo;
  set_variant(s, kc.variant);
  s->nr = m->num_links;
  s->nv = (m->fixed_base ? 0 : 6) + m->num_dofs;
  s->nb = m->num_bodies;
  s->nd = m->num_dofs;
  s->nc = m->num_candidates;
  s->ns = m->num_shapes;
  s->dp.gen = generic ? s->d_gen : nullptr;
  s->dp.gen_links = generic ? s->d_links : nullptr;
  s->dp.gen_nd = m->num_dofs;
  s->dp.gen_nr = m->num_links;
  s->dp.gen_feat = pk.gen_feat;
  return 0;
}

int gs_sim_prepare(gs_sim* s, int num_envs, float* state, const float* shape_friction, float* contact) {
  if (!s || !s->topo) return fail("gs_sim_prepare: model not set");
  if (num_envs <= 0 || !state || !shape_friction || !contact) return fail("gs_sim_prepare: bad buffers");
  s->N = num_envs;
  s->state = state;
  s->mu = shape_friction;
  s->cf = contact;
  return 0;
}

static SimBuffers buffers(gs_sim* s) { return SimBuffers{s->state, s->mu, s->cf, s->N, s->sens, s->d_rows}; }

// floats of contact-row tiles the selected GPU kernel needs for N envs (0: its rows live in LDS)
static size_t rows_needed(const gs_sim* s) {
  if (s->host || !s->topo || (s->variant != 1 && s->variant != 4) || (s->variant == 1 && s->dp.has_terrain) ||
      s->topo->row_floats <= 0 || s->N <= 0)
    return 0;
  const size_t lanes = (size_t)s->topo->row_lanes;
  return ((size_t)s->N + lanes - 1) / lanes * lanes * (size_t)s->topo->row_floats;
}

static int ready(gs_sim* s, const char* where) {
  if (!s || !s->topo || !s->state) return fail("%s: sim not prepared", where);
  if (s->host ? !s->htopo : (!s->sim_fn || !s->pd_fn || !s->d_model || !s->d_links))
    return fail("%s: sim model incomplete", where);
  if (const size_t need = rows_needed(s); need > s->rows_cap) {
    // first step of an LDS-starved topology (or more envs than before): the row tiles, once
    if (hipError_t e = hipSetDevice(s->device); e != hipSuccess) return hip_fail(e, where);
    if (s->d_rows) (void)hipFree(s->d_rows);
    s->d_rows = nullptr;
    s->rows_cap = 0;
    if (hipError_t e = hipMalloc(&s->d_rows, need * sizeof(float)); e != hipSuccess) {
      s->d_rows = nullptr;
      return hip_fail(e, where);
    }
    s->rows_cap = need;
  }
  return 0;
}

static void timing_begin(gs_sim* s, hipStream_t st) {
  if (!s->timing || s->host) return;
  if (!s->ev0) {
    // Timing is diagnostic: if the events cannot be made, switch it off rather than fail the step.
    if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) {
      s->timing = false;
      return;
    }
  }
  (void)hipEventRecord(s->ev0, st);
}
static void timing_end(gs_sim* s, hipStream_t st) {
  if (!s->timing || s->host) return;
  s->timed = hipEventRecord(s->ev1, st) == hipSuccess;
}

namespace {
using host_clock = std::chrono::steady_clock;
double ms_since(host_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(host_clock::now() - t0).count();
}
}  // namespace

// The lane-team kernels do not write the DOF force tensor: with one bound, their launch is followed on its stream by
// k_team_dof_force over the actuation force the launch applied last (tau: [N][nd] or null)
static hipError_t team_dof_force(gs_sim* s, const float* tau, hipStream_t st) {
  if (s->variant != 2 || !s->dp.dof_force) return hipSuccess;
  const long n = (long)s->N * s->nd;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_team_dof_force, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tau, &s->d_model->effort[0],
                     s->N, s->nd, s->dp.dof_force);
  return hipGetLastError();
}

int gs_sim_simulate(gs_sim* s, const float* dof_force, void* stream) {
  if (ready(s, "gs_sim_simulate")) return -1;
  if (s->host) {
    const auto t0 = host_clock::now();
    s->htopo->sim(&s->h_model, s->dp, buffers(s), dof_force, s->pool);
    s->host_ms = ms_since(t0);
    return 0;
  }
  hipStream_t st = (hipStream_t)stream;
  timing_begin(s, st);
  hipError_t e = s->sim_fn(s->d_model, s->dp, buffers(s), dof_force, st);
  if (e == hipSuccess) e = team_dof_force(s, dof_force, st);
  timing_end(s, st);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_simulate");
}

int gs_sim_pd_step(gs_sim* s, const gs_pd_args* a, void* stream) {
  if (ready(s, "gs_sim_pd_step")) return -1;
  if (!a || !a->actions || !a->default_pos || !a->torques_out || !a->dof_state_out)
    return fail("gs_sim_pd_step: actions/default_pos/torques_out/dof_state_out required");
  PdDev d;
  d.actions = a->actions;
  d.dof_state_in = a->dof_state_out;
  d.default_pos = a->default_pos;
  d.kp = a->kp; d.kd = a->kd; d.scale = a->action_scale; d.tlim = a->torque_limit;
  d.decimation = a->decimation;
  d.extra = a->extra_simulates;
  d.torques_out = a->torques_out;
  d.dof_out = a->dof_state_out;
  d.root_out = a->root_state_out;
  d.cf_out = a->contact_out;
  d.actions_copy = a->actions_copy_out;
  d.tail_on = 0;
  if (a->tail_params || a->tail_buffers) {
    // the AnymalTerrain tail in the team kernel's last phase (gymsim.h ABI 9): the checks gt_anymal_post_physics_a
    // makes, post_a's vector rows, and the buffers the kernel has just written being the tail's inputs
    const gt_anymal_params* tp = a->tail_params;
    const gt_anymal_buffers* tb = a->tail_buffers;
    auto aligned = [](const void* q) { return ((uintptr_t)q & 15u) == 0; };
    if (!gs_sim_pd_tail_supported(s)) return fail("gs_sim_pd_step: this sim's kernel has no fused tail");
    if (tb && tb->variant)
      return fail("gs_sim_pd_step: the in-kernel tail is AnymalTerrain's on the lane-team kernel; a gt_anymal_variant "
                  "task runs libgymtask's launches");
    if (!tp || !tb || tb->hound || tp->num_envs != s->N || tp->num_dofs != s->nd || tp->num_dofs % 4 != 0 ||
        tp->num_bodies != s->nr || tp->num_feet > 4 || tp->num_knees > 4 || tp->num_feet < 0 || tp->num_knees < 0 ||
        tp->base_index < 0 || tp->base_index >= s->nr || !tb->reset_count || !tb->reset_masks || !tb->reset_buf ||
        !tb->timeout_buf || !tb->rew_buf || !tb->episode_sums || !tb->base_lin_vel || !tb->base_ang_vel ||
        !tb->projected_gravity || !tb->progress_buf || !tb->randomize_buf || !tb->commands || !tb->feet_air_time ||
        !tb->last_actions || !tb->last_dof_vel)
      return fail("gs_sim_pd_step: invalid tail parameters / buffers");
    for (int k = 0; k < tp->num_feet; ++k)
      if (tp->feet_idx[k] < 0 || tp->feet_idx[k] >= s->nr) return fail("gs_sim_pd_step: tail foot index");
    for (int k = 0; k < tp->num_knees; ++k)
      if (tp->knee_idx[k] < 0 || tp->knee_idx[k] >= s->nr) return fail("gs_sim_pd_step: tail knee index");
    if (tb->torques != a->torques_out || tb->actions != a->actions_copy_out || tb->root_states != a->root_state_out ||
        tb->contact_forces != a->contact_out || tb->dof_state != a->dof_state_out)
      return fail("gs_sim_pd_step: the tail must read this call's outputs");
    if (!aligned(tb->torques) || !aligned(tb->actions) || !aligned(tb->last_actions) || !aligned(tb->last_dof_vel) ||
        !aligned(tb->dof_state))
      return fail("gs_sim_pd_step: the tail's dof rows must be 16-byte aligned");
    d.tail_on = 1;
    d.tail_p = *tp;
    d.tail_b = *tb;
  }
  if (s->host) {
    const auto t0 = host_clock::now();
    s->htopo->pd(&s->h_model, s->dp, buffers(s), d, s->pool);
    s->host_ms = ms_since(t0);
    return 0;
  }
  hipStream_t st = (hipStream_t)stream;
  timing_begin(s, st);
  hipError_t e = s->pd_fn(s->d_model, s->dp, buffers(s), d, st);
  if (e == hipSuccess) e = team_dof_force(s, a->torques_out, st);
  timing_end(s, st);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_pd_step");
}

int gs_sim_refresh_root(gs_sim* s, float* out, void* stream) {
  if (ready(s, "gs_sim_refresh_root")) return -1;
  if (s->host) {
    host_refresh_root(s->state, s->N, &s->h_model.root_com[0], out, s->pool);
    return 0;
  }
  hipError_t e = launch_refresh_root(s->state, s->N, s->nd, &s->d_model->root_com[0], out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_refresh_root");
}
int gs_sim_refresh_dof(gs_sim* s, float* out, void* stream) {
  if (ready(s, "gs_sim_refresh_dof")) return -1;
  if (s->host) {
    host_refresh_dof(s->state, s->N, s->nd, out, s->pool);
    return 0;
  }
  hipError_t e = launch_refresh_dof(s->state, s->N, s->nd, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_refresh_dof");
}
int gs_sim_refresh_contact(gs_sim* s, float* out, void* stream) {
  if (ready(s, "gs_sim_refresh_contact")) return -1;
  if (s->host) {
    host_soa_to_aos(s->cf, s->N, s->nr, 3, out, s->pool);
    return 0;
  }
  hipError_t e = launch_refresh_contact(s->cf, s->N, s->nr, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_refresh_contact");
}
static int kinematics(gs_sim* s, int mode, float* rb, float* jac, float* mm, void* stream, const char* where) {
  if (ready(s, where)) return -1;
  if (!rb && !jac && !mm) return fail("%s: null output", where);
  if (s->host) {
    host_kinematics(&s->h_model, &s->h_links, s->state, s->N, s->nv, mode, rb, jac, mm, s->pool);
    return 0;
  }
  hipError_t e = launch_kinematics(s->d_model, s->d_links, s->state, s->N, s->nv, mode, rb, jac, mm,
                                   (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, where);
}
int gs_sim_refresh_rigid_body(gs_sim* s, float* out, void* stream) {
  return kinematics(s, 1, out, nullptr, nullptr, stream, "gs_sim_refresh_rigid_body");
}
int gs_sim_refresh_jacobian(gs_sim* s, float* out, void* stream) {
  return kinematics(s, 2, nullptr, out, nullptr, stream, "gs_sim_refresh_jacobian");
}
int gs_sim_refresh_mass_matrix(gs_sim* s, float* out, void* stream) {
  return kinematics(s, 4, nullptr, nullptr, out, stream, "gs_sim_refresh_mass_matrix");
}
int gs_sim_set_root(gs_sim* s, const float* src, const int32_t* idx, int n_idx, void* stream) {
  if (ready(s, "gs_sim_set_root")) return -1;
  if (s->host) {
    host_set_root(s->state, s->N, &s->h_model.root_com[0], src, idx, idx ? n_idx : s->N);
    return 0;
  }
  hipError_t e = launch_set_root(s->state, s->N, s->nd, &s->d_model->root_com[0], src, idx, n_idx,
                                 (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_set_root");
}
int gs_sim_set_dof(gs_sim* s, const float* src, const int32_t* idx, int n_idx, void* stream) {
  if (ready(s, "gs_sim_set_dof")) return -1;
  if (s->host) {
    host_set_dof(s->state, s->N, s->nd, src, idx, idx ? n_idx : s->N);
    return 0;
  }
  hipError_t e = launch_set_dof(s->state, s->N, s->nd, src, idx, n_idx, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_set_dof");
}

int gs_sim_set_root_and_dof(gs_sim* s, const float* root, const float* dof, const int32_t* idx, int n_idx,
                            void* stream) {
  if (ready(s, "gs_sim_set_root_and_dof")) return -1;
  if (!root || !dof || !idx || n_idx < 0) return fail("gs_sim_set_root_and_dof: root, dof and idx required");
  if (s->host) {
    host_set_root(s->state, s->N, &s->h_model.root_com[0], root, idx, n_idx);
    host_set_dof(s->state, s->N, s->nd, dof, idx, n_idx);
    return 0;
  }
  hipError_t e = launch_set_root_dof(s->state, s->N, s->nd, &s->d_model->root_com[0], root, dof, idx, n_idx,
                                     (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_set_root_and_dof");
}

int gs_sim_set_force_sensors(gs_sim* s, int n, const int32_t* bodies) {
  if (!s || !s->topo) return fail("gs_sim_set_force_sensors: model not set");
  if (s->state) return fail("gs_sim_set_force_sensors: call before gs_sim_prepare");
  if (n < 0 || n > GS_MAXS || (n > 0 && !bodies)) return fail("gs_sim_set_force_sensors: at most 8 sensors");
  if (n > 0 && s->variant == 2)
    return fail("gs_sim_set_force_sensors: the lane-team kernel has no force sensors (use kernel_variant 1)");
  if (n > 0 && !s->topo->sens)
    return fail("gs_sim_set_force_sensors: topology %s is compiled without force sensors (sensors flag in "
                "tools/gen_topologies.py MODELS)", s->topo->name);
  DevModel& h = s->h_model;
  for (int b = 0; b < GS_MAXB; ++b) h.sens_of_body[b] = -1;
  for (int i = 0; i < n; ++i) {
    const int b = bodies[i];
    if (b <= 0 || b >= s->nb) return fail("gs_sim_set_force_sensors: sensor body out of range (or the root)");
    for (int c = 0; c < s->nb; ++c)
      if (s->parent[c] == b) return fail("gs_sim_set_force_sensors: sensors on non-leaf bodies are not supported");
    if (h.sens_of_body[b] >= 0) return fail("gs_sim_set_force_sensors: two sensors on one body");
    h.sens_of_body[b] = i;
  }
  h.nsens = n;
  if (s->variant == 4) s->dp.gen_feat = (s->dp.gen_feat & ~2) | (n > 0 ? 2 : 0);
  if (s->host) return 0;
  hipError_t e = hipSetDevice(s->device);
  if (e == hipSuccess) e = hipMemcpy(s->d_model, &h, sizeof(DevModel), hipMemcpyHostToDevice);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_set_force_sensors hipMemcpy");
}

int gs_sim_set_dof_drives(gs_sim* s, const int32_t* mode, const double* stiffness, const double* damping) {
  if (!s || !s->topo) return fail("gs_sim_set_dof_drives: model not set");
  if (s->nd > 0 && (!mode || !stiffness || !damping)) return fail("gs_sim_set_dof_drives: null argument");
  DevModel h = s->h_model;
  int any = 0;
  for (int j = 0; j < s->nd; ++j) {
    // gymapi.DofDriveMode: 1 POS (stiffness, damping), 2 VEL (damping); NONE / EFFORT: no drive
    const double kp = mode[j] == 1 ? stiffness[j] : 0.0;
    const double kd = (mode[j] == 1 || mode[j] == 2) ? damping[j] : 0.0;
    if (!(kp >= 0.0) || !(kd >= 0.0)) return fail("gs_sim_set_dof_drives: negative or NaN drive gain");
    h.dkp[j] = (float)kp;
    h.dkd[j] = (float)kd;
    any |= (kp > 0.0 || kd > 0.0);
  }
  // the lane-team kernel has no drive terms: drives run the one-env-per-lane kernel; the lane team comes back once
  // every gain is zero again
  const int any_drive = s->dp.dof_env ? s->env_any_drive : any;
  const KernelChoice kc = choose(s, any_drive, s->dp.dof_env != nullptr);
  if (!kc.variant) return fail(kc.refusal, "gs_sim_set_dof_drives");
  if (!s->host) {
    // the physics kernels read d_model: the blocking upload must not overtake a launch still queued on
    // a caller's (non-blocking) stream, so the device drains first (cold path: dof property changes)
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(s->d_model, &h, sizeof(DevModel), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "gs_sim_set_dof_drives hipMemcpy");
  }
  s->h_model = h;
  s->uni_any_drive = any;
  s->dp.any_drive = any_drive;
  set_variant(s, kc.variant);
  return 0;
}

int gs_sim_set_self_collision(gs_sim* s, int enable) {
  if (!s || !s->topo) return fail("gs_sim_set_self_collision: model not set");
  if (enable && s->h_model.np > 0 && s->topo->npk <= 0)
    return fail("gs_sim_set_self_collision: the compiled topology has no self-contact pool");
  s->dp.self_collide = enable && s->h_model.np > 0;
  return 0;
}

int gs_sim_set_disable_gravity(gs_sim* s, int disable) {
  if (!s) return fail("gs_sim_set_disable_gravity: null sim");
  if (s->state) return fail("gs_sim_set_disable_gravity: call before gs_sim_prepare");
  s->disable_gravity = disable != 0;
  fill_gravity(s);
  return 0;
}

int gs_sim_bind_dof_targets(gs_sim* s, const float* pos_targets, const float* vel_targets) {
  if (!s || !s->topo) return fail("gs_sim_bind_dof_targets: model not set");
  s->dp.ptgt = pos_targets;
  s->dp.vtgt = vel_targets;
  return 0;
}

int gs_sim_bind_dof_properties_env(gs_sim* s, const float* table, int any_drive, int any_limits) {
  if (ready(s, "gs_sim_bind_dof_properties_env")) return -1;
  const int drive = table ? any_drive != 0 : s->uni_any_drive, limits = table ? any_limits != 0 : s->uni_any_limits;
  const KernelChoice kc = choose(s, drive, table != nullptr);
  if (!kc.variant) return fail(kc.refusal, "gs_sim_bind_dof_properties_env");
  s->dp.dof_env = table;
  s->dp.dof_env_n = table ? s->N : 0;
  if (table) {
    s->env_any_drive = drive;
    s->env_any_limits = limits;
  }
  s->dp.any_drive = drive;
  s->dp.any_limits = limits;
  set_variant(s, kc.variant);
  return 0;
}

int gs_sim_bind_force_sensors(gs_sim* s, float* soa) {
  if (ready(s, "gs_sim_bind_force_sensors")) return -1;
  if (s->h_model.nsens > 0 && !soa) return fail("gs_sim_bind_force_sensors: buffer required");
  s->sens = soa;
  return 0;
}

int gs_sim_refresh_force_sensor(gs_sim* s, float* out, void* stream) {
  if (ready(s, "gs_sim_refresh_force_sensor")) return -1;
  if (s->h_model.nsens == 0) return 0;
  if (!s->sens) return fail("gs_sim_refresh_force_sensor: sensors not bound");
  if (s->host) {
    host_soa_to_aos(s->sens, s->N, s->h_model.nsens, 6, out, s->pool);
    return 0;
  }
  hipError_t e = launch_refresh_sensor(s->sens, s->N, s->h_model.nsens, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_refresh_force_sensor");
}

int gs_sim_bind_dof_force(gs_sim* s, float* soa) {
  if (ready(s, "gs_sim_bind_dof_force")) return -1;
  s->dp.dof_force = soa;
  return 0;
}

int gs_sim_refresh_dof_force(gs_sim* s, float* out, void* stream) {
  if (ready(s, "gs_sim_refresh_dof_force")) return -1;
  if (!s->dp.dof_force) return fail("gs_sim_refresh_dof_force: no buffer bound (gs_sim_bind_dof_force)");
  if (!out) return fail("gs_sim_refresh_dof_force: bad buffers");
  if (s->host) {
    host_soa_to_aos(s->dp.dof_force, s->N, s->nd, 1, out, s->pool);
    return 0;
  }
  const long n = (long)s->N * s->nd;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_refresh_dof_force, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     s->dp.dof_force, s->N, s->nd, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "gs_sim_refresh_dof_force");
}

int gs_debug_terrain_query(gs_sim* s, const float* centres, const float* radii, int n, float* out, void* stream) {
  if (!s || !s->dp.has_terrain) return fail("gs_debug_terrain_query: no terrain mesh");
  if (n < 0 || (n > 0 && (!centres || !radii || !out))) return fail("gs_debug_terrain_query: bad buffers");
  if (s->host) {
    host_terrain_query(s->dp, centres, radii, n, out);
    return 0;
  }
  hipError_t e = launch_terrain_query(s->dp, centres, radii, n, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_debug_terrain_query");
}

int gs_debug_self_contacts(gs_sim* s, int mode, float* out, int* count, void* stream) {
  if (ready(s, "gs_debug_self_contacts")) return -1;
  if (!out || !count) return fail("gs_debug_self_contacts: bad buffers");
  if (s->host) {
    if (mode != 0) return fail("gs_debug_self_contacts: the host backend has the inline form only (mode 0)");
    s->htopo->dbg_pool(&s->h_model, s->dp, buffers(s), out, count, s->pool);
    return 0;
  }
  const hipError_t e = s->topo->dbg_pool(s->d_model, s->dp, buffers(s), mode, out, count, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "gs_debug_self_contacts (mode 1 needs a split-form topology)");
}

int gs_debug_team_form(gs_sim* s, int* envs_per_wave, int* row_lanes) {
  if (ready(s, "gs_debug_team_form")) return -1;
  if (!envs_per_wave || !row_lanes) return fail("gs_debug_team_form: bad arguments");
  if (s->host || s->variant != 2) return fail("gs_debug_team_form: the sim does not run the lane-team kernels");
  team_launch_form(s->dp, envs_per_wave, row_lanes);
  return 0;
}

int gs_debug_team_sweeps(gs_sim* s, int* resident) {
  if (ready(s, "gs_debug_team_sweeps")) return -1;
  if (!resident) return fail("gs_debug_team_sweeps: bad arguments");
  if (s->host || s->variant != 2) return fail("gs_debug_team_sweeps: the sim does not run the lane-team kernels");
  *resident = team_launch_resident(s->dp);
  return 0;
}

int gs_sim_kernel_variant(gs_sim* s) { return s ? s->variant : -1; }

int gs_sim_pd_tail_supported(const gs_sim* s) {
  return s && !s->host && s->topo && s->variant == 2 && !s->dp.has_terrain && team_fused_tail_available() ? 1 : 0;
}

int gs_sim_enable_timing(gs_sim* s, int enable) {
  if (!s) return fail("gs_sim_enable_timing: null sim");
  s->timing = enable != 0;
  return 0;
}
float gs_sim_last_kernel_ms(gs_sim* s) {
  if (s && s->host) return s->timing ? (float)s->host_ms : -1.f;
  if (!s || !s->timed) return -1.f;
  float ms = -1.f;
  if (hipEventSynchronize(s->ev1) != hipSuccess) return -1.f;
  if (hipEventElapsedTime(&ms, s->ev0, s->ev1) != hipSuccess) return -1.f;
  return ms;
}

}  // extern "C"
