// gs_model_pack.h -- a gs_model_desc (include/gymsim.h, float64) checked and packed into the float32 tables the
// kernels read.  Pure host arithmetic: no gs_sim, no HIP call; gs_sim_set_model (gs_capi.hip) uploads and commits
// the result.
#pragma once
#include <string>

#include "gs_internal.h"
#include "../../include/gymsim.h"

// the key of a model's compiled kernels (g_topologies / g_team_kernels / g_host_topologies sig)
std::string model_signature(const gs_model_desc* m);

struct ModelPack {
  DevModel model;       // no force sensors yet (gs_sim_set_force_sensors)
  DevLinks links;
  int any_limits;       // some dof of the model has limits
  // the runtime-sized kernel only (zero otherwise): its candidate tables, DevParams::gen_feat and the TopoEntry
  // it stands in for
  GenTopo gen;
  int gen_feat;
  TopoEntry gen_entry;
  std::string err;      // why model_pack returned -1
};

// `topo`: the model's compiled topology, null for the runtime-sized kernel -- which is a GPU kernel (`host`
// refuses it) with plane contacts only (`has_terrain` refuses it).  0, or -1 with out->err set.
int model_pack(const gs_model_desc* m, const TopoEntry* topo, bool host, bool has_terrain, ModelPack* out);
