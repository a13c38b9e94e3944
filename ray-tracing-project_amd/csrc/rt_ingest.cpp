// rt_ingest.cpp -- mesh ingest with Tucano::MeshImporter semantics: OBJ / MTL parsing, the mesh built from
// caller arrays, normalisation, face normals, the mesh ABI, and the synthetic triangle soup.
//
// Reference semantics restated here (file:line in plindhorst/Ray-Tracing-Project):
//   OBJ/MTL ingest      tucano/utils/objimporter.hpp:81-351, tucano/utils/mtlIO.hpp:36-140
//   normalisation       tucano/mesh.hpp:592-628, tucano/model.hpp:102-105,169-173
//   face normals        tucano/mesh.hpp:448-482
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rt_scene.h"

using rt::f3;

namespace {

void mtl_default(rt_material& m) {  // Tucano::Material::Mtl defaults (materials/mtl.hpp:22-40)
  for (int k = 0; k < 3; k++) { m.ka[k] = 0.3f; m.kd[k] = 0.5f; m.ks[k] = 1.0f; }
  m.shininess = 10.0f;
  m.optical_density = 0.0f;
  m.dissolve = 1.0f;
}

std::string path_name(const std::string& s) {  // getPathName (mtlIO.hpp:36-40)
  size_t found = s.find_last_of("/\\");
  return s.substr(0, found + 1);
}

void erase_crlf(std::string& s) {
  s.erase(std::remove(s.begin(), s.end(), '\n'), s.end());
  s.erase(std::remove(s.begin(), s.end(), '\r'), s.end());
}

// MaterialImporter::loadMTL (mtlIO.hpp:49-140): tokens split on single spaces, atof values
bool load_mtl(rt_mesh* m, const std::string& filename) {
  std::ifstream in(filename.c_str(), std::ios::in);
  if (!in) return false;
  for (std::string line; std::getline(in, line);) {
    std::stringstream ss(line);
    if (ss.str().empty()) continue;
    std::string s;
    std::vector<std::string> tok;
    while (std::getline(ss, s, ' ')) tok.push_back(s);
    if (tok.empty() || tok[0] == "#") continue;
    if (tok[0] == "newmtl") {
      rt_material mt;
      mtl_default(mt);
      m->mats.push_back(mt);
      std::string nm = tok.size() > 1 ? tok[1] : std::string();
      erase_crlf(nm);
      m->mat_names.push_back(nm);
      continue;
    }
    if (m->mats.empty()) continue;  // reference: materials.back() on an empty vector (UB); ignored
    rt_material& cur = m->mats.back();
    auto f = [&](size_t i) { return i < tok.size() ? (float)atof(tok[i].c_str()) : 0.0f; };
    if (tok[0] == "Ns") cur.shininess = f(1);
    else if (tok[0] == "Ka") { cur.ka[0] = f(1); cur.ka[1] = f(2); cur.ka[2] = f(3); }
    else if (tok[0] == "Kd") { cur.kd[0] = f(1); cur.kd[1] = f(2); cur.kd[2] = f(3); }
    else if (tok[0] == "Ks") { cur.ks[0] = f(1); cur.ks[1] = f(2); cur.ks[2] = f(3); }
    else if (tok[0] == "Ni") cur.optical_density = f(1);
    else if (tok[0] == "d") cur.dissolve = f(1);
  }
  if (m->mats.empty()) {  // "if no mtllib then just create a default material"
    rt_material mt;
    mtl_default(mt);
    m->mats.push_back(mt);
    m->mat_names.push_back("");
  }
  return true;
}

// istringstream >> float for the numeric tokens of v/vn lines (num_get -> strtof on the prefix)
int parse_floats(const char* s, const char* end, float* out, int n) {
  for (int k = 0; k < n; k++) {
    while (s < end && (*s == ' ' || *s == '\t' || *s == '\r' || *s == '\v' || *s == '\f')) s++;
    if (s >= end) return k;
    char* e;
    out[k] = strtof(s, &e);
    if (e == s) return k;
    s = e;
  }
  return n;
}

// Mesh::loadVertices bounding box / scale / centre (mesh.hpp:592-628); std::max/min argument order
void load_vertices(rt_mesh* m) {
  size_t nv = m->v4.size() / 4;
  m->scale = 1.0f;
  m->center[0] = m->center[1] = m->center[2] = 0.0f;
  if (nv == 0) return;
  const float* v = m->v4.data();
  float xMax = v[0], xMin = v[0], yMax = v[1], yMin = v[1], zMax = v[2], zMin = v[2];
  for (size_t i = 0; i < nv; i++) {
    const float* p = v + 4 * i;
    xMax = rt::smax(p[0], xMax); yMax = rt::smax(p[1], yMax); zMax = rt::smax(p[2], zMax);
    xMin = rt::smin(p[0], xMin); yMin = rt::smin(p[1], yMin); zMin = rt::smin(p[2], zMin);
  }
  float ext = rt::smax(rt::smax(std::fabs(xMax - xMin), std::fabs(yMax - yMin)), std::fabs(zMax - zMin));
  m->scale = (float)(1.0 / (double)ext);
  m->center[0] = (float)((double)(xMax + xMin) / 2.0);
  m->center[1] = (float)((double)(yMax + yMin) / 2.0);
  m->center[2] = (float)((double)(zMax + zMin) / 2.0);
}

// computeNormals (objimporter.hpp:81-106)
void compute_normals(rt_mesh* m, const std::vector<std::vector<uint32_t>>& groups) {
  size_t nv = m->v4.size() / 4;
  m->vn3.assign(3 * nv, 0.0f);
  auto V = [&](uint32_t i) { return f3{m->v4[4 * i], m->v4[4 * i + 1], m->v4[4 * i + 2]}; };
  for (const auto& g : groups)
    for (size_t i = 0; i + 2 < g.size(); i += 3) {
      f3 v0 = rt::normalized(rt::sub(V(g[i + 1]), V(g[i])));
      f3 v1 = rt::normalized(rt::sub(V(g[i + 2]), V(g[i])));
      f3 n = rt::normalized(rt::cross(v0, v1));
      for (int k = 0; k < 3; k++) {
        float* d = &m->vn3[3 * g[i + k]];
        d[0] = d[0] + n.x; d[1] = d[1] + n.y; d[2] = d[2] + n.z;
      }
    }
  for (size_t i = 0; i < nv; i++) {
    f3 n = rt::normalized(f3{m->vn3[3 * i], m->vn3[3 * i + 1], m->vn3[3 * i + 2]});
    m->vn3[3 * i] = n.x; m->vn3[3 * i + 1] = n.y; m->vn3[3 * i + 2] = n.z;
  }
}

// createFaces (mesh.hpp:448-482), normalizeModelMatrix + getShapeModelMatrix (model.hpp)
int finish_mesh(rt_mesh* m, const std::vector<std::vector<uint32_t>>& groups, const std::vector<int32_t>& gmat,
                bool have_vn) {
  const size_t nv = m->v4.size() / 4;
  // validate every index group before anything indexes with it (computeNormals included: the
  // reference reads and writes out of bounds here)
  if (nv > 0)
    for (const auto& ix : groups) {
      if (ix.size() % 3 != 0) {
        rt::set_error("index group of %zu indices is not a multiple of 3 (reference reads out of bounds)", ix.size());
        return RT_ERR_INVALID;
      }
      for (uint32_t id : ix)
        if (id >= nv) { rt::set_error("face vertex index %u out of range", id + 1); return RT_ERR_INVALID; }
    }
  load_vertices(m);
  if (!have_vn && nv > 0) compute_normals(m, groups);  // no vertices: no faces either (below)
  m->fidx.clear(); m->fn3.clear(); m->fmat.clear();
  auto V = [&](uint32_t i) { return f3{m->v4[4 * i], m->v4[4 * i + 1], m->v4[4 * i + 2]}; };
  if (nv > 0)
    for (size_t g = 0; g < groups.size(); g++) {
      const auto& ix = groups[g];
      for (size_t i = 0; i < ix.size(); i += 3) {
        for (int k = 0; k < 3; k++) m->fidx.push_back(ix[i + k]);
        m->fmat.push_back(gmat[g]);
        f3 v1 = rt::normalized(rt::sub(V(ix[i + 2]), V(ix[i])));
        f3 v0 = rt::normalized(rt::sub(V(ix[i + 1]), V(ix[i])));
        f3 n = rt::normalized(rt::cross(v0, v1));
        m->fn3.push_back(n.x); m->fn3.push_back(n.y); m->fn3.push_back(n.z);
      }
    }
  float shape[16], model[16];
  rt::identity4(shape);
  rt::scale4(shape, m->scale);
  rt::translate4(shape, f3{-m->center[0], -m->center[1], -m->center[2]});
  rt::identity4(model);
  rt::affmul(model, shape, m->M);
  return RT_OK;
}

}  // namespace

extern "C" int rt_mesh_load_obj(const char* path, rt_mesh** out) {
  if (!path || !out) { rt::set_error("rt_mesh_load_obj: null argument"); return RT_ERR_INVALID; }
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) { rt::set_error("Cannot open %s", path); return RT_ERR_IO; }
  std::string buf;
  fseek(f, 0, SEEK_END);
  long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  buf.resize(len > 0 ? (size_t)len : 0);
  if (len > 0 && fread(&buf[0], 1, (size_t)len, f) != (size_t)len) { fclose(f); rt::set_error("read error %s", path); return RT_ERR_IO; }
  fclose(f);

  auto m = new rt_mesh();
  const std::string dir = path_name(path);
  std::vector<std::vector<uint32_t>> groups(1);
  std::vector<int32_t> gmat(1, -1);
  std::vector<float> norms;
  int32_t current_mat = -1;
  size_t pos = 0;
  while (pos < buf.size()) {  // std::getline(in, line)
    size_t nl = buf.find('\n', pos);
    if (nl == std::string::npos) nl = buf.size();
    const char* ls = buf.data() + pos;
    const char* le = buf.data() + nl;
    size_t L = nl - pos;
    pos = nl + 1;
    if (L >= 6 && !strncmp(ls, "mtllib", 6)) {
      if (L < 7) { delete m; rt::set_error("malformed mtllib line"); return RT_ERR_INVALID; }
      std::string fn = dir + std::string(ls + 7, le);
      erase_crlf(fn);
      load_mtl(m, fn);
    } else if (L >= 6 && !strncmp(ls, "usemtl", 6)) {
      if (!groups.back().empty()) { groups.emplace_back(); gmat.push_back(-1); }
      if (L < 7) { delete m; rt::set_error("malformed usemtl line"); return RT_ERR_INVALID; }
      std::string nm(ls + 7, le);
      erase_crlf(nm);
      for (size_t i = 0; i < m->mat_names.size(); i++)
        if (m->mat_names[i] == nm) current_mat = (int32_t)i;
      gmat.back() = current_mat;
    } else if (L >= 2 && ls[0] == 'v' && ls[1] == ' ') {
      float v[3] = {0, 0, 0};
      parse_floats(ls + 2, le, v, 3);
      m->v4.insert(m->v4.end(), {v[0], v[1], v[2], 1.0f});
    } else if (L >= 2 && ls[0] == 'v' && ls[1] == 'n') {
      float n[3] = {0, 0, 0};
      if (L >= 3) parse_floats(ls + 3, le, n, 3);
      norms.insert(norms.end(), {n[0], n[1], n[2]});
    } else if (L >= 2 && ls[0] == 'f' && ls[1] == ' ') {
      const char* p = ls + 2;
      while (p < le) {
        while (p < le && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\v' || *p == '\f')) p++;
        if (p >= le) break;
        const char* e = p;
        while (e < le && !(*e == ' ' || *e == '\t' || *e == '\r' || *e == '\v' || *e == '\f')) e++;
        long vid = strtol(std::string(p, e).c_str(), nullptr, 10);  // stoi(element before '/')
        groups.back().push_back((uint32_t)(vid - 1));
        p = e;
      }
    }
  }
  const size_t nv = m->v4.size() / 4;
  const bool have_vn = norms.size() == 3 * nv;
  if (have_vn) m->vn3 = norms;
  // only non-empty index groups become index buffers (objimporter.hpp:312-319)
  std::vector<std::vector<uint32_t>> g2;
  std::vector<int32_t> m2;
  for (size_t g = 0; g < groups.size(); g++)
    if (!groups[g].empty()) { g2.push_back(std::move(groups[g])); m2.push_back(gmat[g]); }
  int rc = finish_mesh(m, g2, m2, have_vn);
  if (rc) { delete m; return rc; }
  *out = m;
  return RT_OK;
}

extern "C" int rt_mesh_from_arrays(int32_t nv, const float* v3, const float* vn3, int32_t ng, const int32_t* gcount,
                                   const uint32_t* idx, const int32_t* gmat, int32_t nm, const rt_material* mats,
                                   rt_mesh** out) {
  if (!out || nv < 0 || ng < 0 || (nv && !v3) || (ng && (!gcount || !gmat))) {
    rt::set_error("rt_mesh_from_arrays: invalid arguments");
    return RT_ERR_INVALID;
  }
  *out = nullptr;
  auto m = new rt_mesh();
  m->v4.resize(4 * (size_t)nv);
  for (int32_t i = 0; i < nv; i++) {
    m->v4[4 * i] = v3[3 * i]; m->v4[4 * i + 1] = v3[3 * i + 1]; m->v4[4 * i + 2] = v3[3 * i + 2]; m->v4[4 * i + 3] = 1.0f;
  }
  if (vn3) m->vn3.assign(vn3, vn3 + 3 * (size_t)nv);
  for (int32_t i = 0; i < nm; i++) { m->mats.push_back(mats[i]); m->mat_names.push_back("material_" + std::to_string(i)); }
  std::vector<std::vector<uint32_t>> groups(ng);
  std::vector<int32_t> gm(ng);
  size_t off = 0;
  for (int32_t g = 0; g < ng; g++) {
    if (gcount[g] < 0) { delete m; rt::set_error("negative group size"); return RT_ERR_INVALID; }
    groups[g].assign(idx + off, idx + off + gcount[g]);
    gm[g] = gmat[g];
    if (gm[g] >= nm) { delete m; rt::set_error("group material %d out of range", gm[g]); return RT_ERR_INVALID; }
    off += (size_t)gcount[g];
  }
  int rc = finish_mesh(m, groups, gm, vn3 != nullptr);
  if (rc) { delete m; return rc; }
  *out = m;
  return RT_OK;
}

extern "C" void rt_mesh_destroy(rt_mesh* m) { delete m; }

extern "C" int rt_mesh_get_desc(const rt_mesh* m, rt_mesh_desc* d) {
  if (!m || !d) { rt::set_error("rt_mesh_get_desc: null argument"); return RT_ERR_INVALID; }
  d->n_vertices = (int32_t)(m->v4.size() / 4);
  d->vertices = m->v4.data();
  d->vertex_normals = m->vn3.data();
  d->n_faces = (int32_t)m->fmat.size();
  d->face_vertex_ids = m->fidx.data();
  d->face_normals = m->fn3.data();
  d->face_material_ids = m->fmat.data();
  d->n_materials = (int32_t)m->mats.size();
  d->materials = m->mats.data();
  memcpy(d->shape_model_matrix, m->M, 64);
  return RT_OK;
}

// Synthetic soup
static inline uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline float u01(uint64_t& s) { return (float)(splitmix64(s) >> 40) * (1.0f / 16777216.0f); }

extern "C" void rt_generate_soup(int32_t n, uint64_t seed, float* v) {
  uint64_t s = seed;
  for (int32_t t = 0; t < n; t++) {
    float c[3];
    for (int k = 0; k < 3; k++) c[k] = u01(s) - 0.5f;
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) {
        float off = (u01(s) * 2.0f - 1.0f) * 0.01f;
        v[9 * (size_t)t + 3 * j + k] = c[k] + off;
      }
  }
}
