// gs_terrain_build.hip -- heightfield grid mesh -> the TERR kernels' tables (gs_terrain_build.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gs_terrain_build.h"

int terrain_build(const float* vertices, int64_t num_vertices, const uint32_t* triangles, int64_t num_triangles,
                  const double* transform_p, TerrainTables* out) {
  auto fail = [out](const std::string& msg) {
    out->err = msg;
    return -1;
  };
  if (num_triangles < 2) return fail("gs_sim_add_triangle_mesh: empty mesh");
  // grid shape from the first triangle (v[0,0], v[1,1], v[0,1]) = (0, cols + 1, 1)
  const int64_t cols = (int64_t)triangles[1] - 1;
  if (triangles[0] != 0 || triangles[2] != 1 || cols < 2 || num_vertices % cols != 0)
    return fail("gs_sim_add_triangle_mesh: not a heightfield grid mesh (first triangle)");
  const int64_t rows = num_vertices / cols;
  if (rows < 2 || num_triangles != 2 * (rows - 1) * (cols - 1))
    return fail("gs_sim_add_triangle_mesh: triangle count does not match a " + std::to_string(rows) + "x" +
                std::to_string(cols) + " grid");
  if (rows > (1 << 24) || cols > (1 << 24)) return fail("gs_sim_add_triangle_mesh: grid too large");
  for (int64_t i = 0; i + 1 < rows; ++i) {
    for (int64_t j = 0; j + 1 < cols; ++j) {
      const int64_t b = i * cols + j, t = 2 * (i * (cols - 1) + j);
      const uint32_t* a = triangles + 3 * t;
      if (a[0] != b || a[1] != b + cols + 1 || a[2] != b + 1 || a[3] != b || a[4] != b + cols || a[5] != b + cols + 1)
        return fail("gs_sim_add_triangle_mesh: triangle " + std::to_string(t) +
                    " does not follow the heightfield grid layout");
    }
  }
  // spacing: the grid points are x = i*hs, y = j*hs before the transform.  Slope correction moves a
  // vertex by up to one cell, so take the median over columns of the first-to-last-row span / (rows - 1):
  // a median single-row step carries the float32 rounding of the coordinates (1.5e-5 m at 160 m), which
  // accumulated over 2000 cells misplaces the far end of the 1200 x 2000 AnymalTerrain map by 0.2 cells
  std::vector<double> spans;
  for (int64_t j = 0; j < cols && spans.size() < 4096; j += std::max<int64_t>(1, cols / 1024))
    spans.push_back((double)vertices[3 * ((rows - 1) * cols + j)] - (double)vertices[3 * j]);
  std::sort(spans.begin(), spans.end());
  double hs = spans[spans.size() / 2] / (double)(rows - 1);
  if (!(hs > 0)) return fail("gs_sim_add_triangle_mesh: cannot infer the grid spacing");
  const double tx = transform_p ? transform_p[0] : 0.0, ty = transform_p ? transform_p[1] : 0.0,
               tz = transform_p ? transform_p[2] : 0.0;
  // grid point (0, 0): vertices of row 0 / column 0 can only move inward, so take the minimum
  double x0 = vertices[0], y0 = vertices[1];
  for (int64_t j = 0; j < cols; ++j) x0 = std::min(x0, (double)vertices[3 * j]);
  for (int64_t i = 0; i < rows; ++i) y0 = std::min(y0, (double)vertices[3 * (i * cols) + 1]);
  std::vector<float4>& hv = out->verts;
  hv.assign((size_t)(rows * cols), float4{});
  for (int64_t i = 0; i < rows; ++i) {
    for (int64_t j = 0; j < cols; ++j) {
      const float* v = vertices + 3 * (i * cols + j);
      const double gx = x0 + i * hs, gy = y0 + j * hs;
      if (std::fabs(v[0] - gx) > 1.001 * hs || std::fabs(v[1] - gy) > 1.001 * hs)
        return fail("gs_sim_add_triangle_mesh: a vertex lies more than one cell from its grid point");
      hv[(size_t)(i * cols + j)] = make_float4((float)(v[0] + tx), (float)(v[1] + ty), (float)(v[2] + tz), 0.f);
    }
  }
  std::vector<uint4>& hc = out->cells;
  hc.assign((size_t)((rows - 1) * (cols - 1)), uint4{});
  for (int64_t i = 0; i + 1 < rows; ++i) {
    for (int64_t j = 0; j + 1 < cols; ++j) {
      const float4 q[4] = {hv[i * cols + j], hv[i * cols + j + 1], hv[(i + 1) * cols + j], hv[(i + 1) * cols + j + 1]};
      float zmax = q[0].z, zmin = q[0].z, xmin = q[0].x, xmax = q[0].x, ymin = q[0].y, ymax = q[0].y;
      for (int k = 1; k < 4; ++k) {
        zmax = std::max(zmax, q[k].z);
        zmin = std::min(zmin, q[k].z);
        xmin = std::min(xmin, q[k].x); xmax = std::max(xmax, q[k].x);
        ymin = std::min(ymin, q[k].y); ymax = std::max(ymax, q[k].y);
      }
      const double cx0 = x0 + tx + i * hs, cy0 = y0 + ty + j * hs;
      uint32_t f = 0;
      if (xmin < cx0 - 0.25 * hs) f |= TCELL_XLO;
      if (xmax > cx0 + 1.25 * hs) f |= TCELL_XHI;
      if (ymin < cy0 - 0.25 * hs) f |= TCELL_YLO;
      if (ymax > cy0 + 1.25 * hs) f |= TCELL_YHI;
      // the extents beyond the cell square, rounded up to hs / TCELL_EXT_UNITS (gs_terrain.h)
      auto ext = [&](double d) -> uint32_t {
        return (uint32_t)std::min(255.0, std::ceil(std::max(0.0, d) / hs * TCELL_EXT_UNITS));
      };
      const uint32_t ew = ext(cx0 - xmin) | ext(xmax - (cx0 + hs)) << 8 | ext(cy0 - ymin) << 16 |
                          ext(ymax - (cy0 + hs)) << 24;
      uint32_t zb, zl;
      std::memcpy(&zb, &zmax, 4);
      std::memcpy(&zl, &zmin, 4);
      hc[(size_t)(i * (cols - 1) + j)] = make_uint4(zb, f, zl, ew);
    }
  }
  // block summary for the query's first cull (gs_terrain.h sphere_contact): the highest cell top of each block
  const int64_t brows = (rows - 1 + TERRAIN_BLK - 1) / TERRAIN_BLK, bcols = (cols - 1 + TERRAIN_BLK - 1) / TERRAIN_BLK;
  std::vector<float>& hb = out->blk;
  hb.assign((size_t)(brows * bcols), -3.0e38f);
  for (int64_t i = 0; i + 1 < rows; ++i)
    for (int64_t j = 0; j + 1 < cols; ++j) {
      float top;
      std::memcpy(&top, &hc[(size_t)(i * (cols - 1) + j)].x, 4);
      float& b = hb[(size_t)((i / TERRAIN_BLK) * bcols + j / TERRAIN_BLK)];
      b = std::max(b, top);
    }
  // 4 x 4 square maxima (clipped at the grid's end): row-wise maxima of 4, then column-wise
  const int64_t cr = rows - 1, cc = cols - 1;
  std::vector<float> h4((size_t)(cr * cc));
  std::vector<float>& hq = out->sq4;
  hq.assign((size_t)(cr * cc), 0.f);
  for (int64_t i = 0; i < cr; ++i)
    for (int64_t j = 0; j < cc; ++j) {
      float m = -3.0e38f;
      for (int64_t d = 0; d < 4 && j + d < cc; ++d) {
        float top;
        std::memcpy(&top, &hc[(size_t)(i * cc + j + d)].x, 4);
        m = std::max(m, top);
      }
      h4[(size_t)(i * cc + j)] = m;
    }
  for (int64_t i = 0; i < cr; ++i)
    for (int64_t j = 0; j < cc; ++j) {
      float m = -3.0e38f;
      for (int64_t d = 0; d < 4 && i + d < cr; ++d) m = std::max(m, h4[(size_t)((i + d) * cc + j)]);
      hq[(size_t)(i * cc + j)] = m;
    }
  // cell records (gs_terrain.h TERRAIN_REC): the four vertices, the unit normals of the cell's triangles
  // (v00, v11, v01) and (v00, v10, v11) in double from the float vertices; degenerate or downward-facing: (0, 0, -1)
  std::vector<float4>& hr = out->rec;
  hr.assign((size_t)(cr * cc * TERRAIN_REC), float4{});
  for (int64_t i = 0; i < cr; ++i)
    for (int64_t j = 0; j < cc; ++j) {
      const float4 q00 = hv[i * cols + j], q01 = hv[i * cols + j + 1], q10 = hv[(i + 1) * cols + j],
                   q11 = hv[(i + 1) * cols + j + 1];
      auto normal = [](const float4& a, const float4& b, const float4& c, float* nf) {
        const double e1[3] = {(double)b.x - a.x, (double)b.y - a.y, (double)b.z - a.z};
        const double e2[3] = {(double)c.x - a.x, (double)c.y - a.y, (double)c.z - a.z};
        const double x[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double l2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
        nf[0] = 0.f; nf[1] = 0.f; nf[2] = -1.f;
        if (!(l2 > 1e-14)) return;
        const double il = 1.0 / std::sqrt(l2);
        if (x[2] * il < (double)TERRAIN_DOWN_NZ) return;
        for (int k = 0; k < 3; ++k) nf[k] = (float)(x[k] * il);
      };
      float n0[3], n1[3];
      normal(q00, q11, q01, n0);
      normal(q00, q10, q11, n1);
      float4* r = &hr[(size_t)((i * cc + j) * TERRAIN_REC)];
      r[0] = make_float4(q00.x, q00.y, q00.z, n0[0]);
      r[1] = make_float4(q01.x, q01.y, q01.z, n0[1]);
      r[2] = make_float4(q10.x, q10.y, q10.z, n0[2]);
      r[3] = make_float4(q11.x, q11.y, q11.z, n1[0]);
      r[4] = make_float4(n1[1], n1[2], 0.f, 0.f);
    }
  TerrainDev& T = out->grid;
  T = TerrainDev{};
  T.bcols = (int)bcols;
  T.rows = (int)rows;
  T.cols = (int)cols;
  T.x0 = (float)(x0 + tx);
  T.y0 = (float)(y0 + ty);
  T.hs = (float)hs;
  T.inv_hs = (float)(1.0 / hs);
  return 0;
}
