// gs_terrain_build.h -- a heightfield triangle mesh (gymapi add_triangle_mesh of terrain_utils'
// convert_heightfield_to_trimesh) turned into the tables the TERR kernels query (gs_terrain.h).  Pure host
// arithmetic: no gs_sim, no HIP call; gs_sim_add_triangle_mesh (gs_capi.hip) uploads or keeps the result.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "gs_terrain.h"

struct TerrainTables {
  std::vector<float4> verts;  // TerrainDev::v: the transformed vertices
  std::vector<uint4> cells;   // TerrainDev::cell: top, TCELL_* flags, bottom, extents beyond the cell square
  std::vector<float> blk;     // TerrainDev::blk: highest cell top per TERRAIN_BLK x TERRAIN_BLK block of cells
  std::vector<float> sq4;     // TerrainDev::sq4: highest cell top of the 4 x 4 cells starting at each cell
  std::vector<float4> rec;    // TerrainDev::rec: cell records, vertices + face normals (TERRAIN_REC)
  TerrainDev grid;            // the grid scalars (rows, cols, bcols, x0, y0, hs, inv_hs); pointers null, mu unset
  std::string err;            // why terrain_build returned -1
};

// `vertices` [num_vertices][3], `triangles` [num_triangles][3], `transform_p` the translation (null: none).
// 0, or -1 with out->err set.
int terrain_build(const float* vertices, int64_t num_vertices, const uint32_t* triangles, int64_t num_triangles,
                  const double* transform_p, TerrainTables* out);
