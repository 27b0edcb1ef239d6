// gs_kernel_choice.h -- which physics kernel form a sim runs: the one rule, for gs_sim_set_model,
// gs_sim_set_dof_drives and gs_sim_bind_dof_properties_env (gs_capi.hip).  Pure: no gs_sim, no HIP call, so a
// setter asks with the flags it is about to set and commits them only when the answer is a variant
// (tests/test_kernel_choice.py prints the whole table).
#pragma once

struct KernelChoiceIn {
  bool host;        // sim created with device < 0
  bool compiled;    // a compiled topology matches the model (gs_topologies.h)
  bool team;        // ... and has a lane-team entry (gs_team.hip)
  int any_limits;   // the model (per asset) has a joint limit: the lane team has no limit rows
  int want;         // gs_sim_params.kernel_variant: 0 auto, 1 lane, 2 team, 4 runtime-sized
  int any_drive;    // drive gains in effect (the bound per-actor table's, else the asset's)
  bool dof_env;     // a per-actor dof property table is bound
};

struct KernelChoice {
  int variant;          // 1 one env per lane, 2 lane team, 3 host backend, 4 runtime-sized; 0: refused
  const char* refusal;  // printf format with at most one %s: the topology signature (gs_sim_set_model's refusals)
                        // or the calling entry point (the lane team's missing features)
};

// (model_pack says the same of a host sim before it checks the runtime-sized kernel's tables: gs_model_pack.hip)
constexpr const char* kRefuseRuntimeOnHost =
    "gs_sim_set_model: the runtime-sized kernel is a GPU kernel and no host solver is compiled for this topology (add "
    "it with tools/gen_topologies.py): %s";

inline KernelChoice kernel_choice(const KernelChoiceIn& in) {
  // A topology with no compiled kernel runs the runtime-sized kernel (gs_generic.hip) on the GPU; kernel_variant 4
  // asks for it on a compiled topology too (the cross-check of the two solver forms).  The host backend has
  // compiled topologies only.
  if (!in.compiled || (in.want == 4 && !in.host)) {
    if (in.host)
      return {0, kRefuseRuntimeOnHost};
    if (in.want == 1 || in.want == 2)
      return {0, "gs_sim_set_model: kernel_variant 1 / 2 requested but topology %s is not compiled (the runtime-"
                 "sized kernel is variant 4)"};
    return {4, nullptr};  // (it has drives, limits and per-actor properties)
  }
  if (in.host) {
    if (in.want == 2) return {0, "gs_sim_set_model: the lane-team kernel is a GPU kernel (host sim)"};
    return {3, nullptr};
  }
  // the lane team has no joint-limit rows: the one-env-per-lane kernel runs (a trimesh terrain runs the lane
  // team's TERR form; kernel_variant 1 still selects the one-env-per-lane kernel)
  const bool team = in.team && !in.any_limits;
  if (in.want == 2 && !team) return {0, "gs_sim_set_model: no lane-team kernel for this topology / joint limits"};
  if (!team || in.want == 1) return {1, nullptr};
  // nor drive terms or per-actor dof properties: the one-env-per-lane kernel runs while either is in use, and the
  // lane team comes back once every gain is zero and no table is bound
  if (in.any_drive || in.dof_env) {
    if (in.want == 2)
      return {0, in.dof_env ? "%s: the lane-team kernel (kernel_variant 2) has no joint drives or per-actor dof "
                              "properties"
                            : "%s: the lane-team kernel (kernel_variant 2) has no joint drives"};
    return {1, nullptr};
  }
  return {2, nullptr};
}
