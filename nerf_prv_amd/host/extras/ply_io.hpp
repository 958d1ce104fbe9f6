// ply_io.hpp -- the ground-truth MESH file of mode 3 with `gt_surface: mesh`: exactly the .ply that prv_mesh_write_file
// writes (include/prv.h): binary_little_endian 1.0, vertices float x y z nx ny nz + uchar red green blue (27 bytes),
// faces `list uchar int` with 3 ids each (13 bytes).  Any other layout is refused with a message; nothing is returned then.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace prvhost {

// "" and the arrays (positions as the file has them: the dataset frame; normals are skipped), or what is wrong with the file
inline std::string ply_read(const std::string& path, std::vector<float>& xyz, std::vector<uint8_t>& rgb, std::vector<uint32_t>& tri) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) return "cannot open " + path;
  static const char* const kVertexProps[9] = {"float x", "float y", "float z", "float nx", "float ny", "float nz", "uchar red", "uchar green", "uchar blue"};
  std::string line;
  auto next = [&]() { // the next header line that is not a comment
    while (std::getline(f, line)) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.rfind("comment", 0) != 0 && line.rfind("obj_info", 0) != 0) return true;
    }
    return false;
  };
  auto count_of = [&](const char* element, uint64_t& n) {
    std::istringstream ss(line);
    std::string a, b, rest;
    return (ss >> a >> b >> n) && a == "element" && b == element && !(ss >> rest);
  };
  if (!next() || line != "ply") return path + ": not a ply file";
  if (!next() || line != "format binary_little_endian 1.0")
    return path + ": only `format binary_little_endian 1.0` is read (the layout prv_mesh_write_file writes), got `" + line + "`";
  uint64_t nv = 0, nt = 0;
  if (!next() || !count_of("vertex", nv)) return path + ": expected `element vertex <n>`, got `" + line + "`";
  for (const char* p : kVertexProps)
    if (!next() || line != std::string("property ") + p)
      return path + ": vertices must be float x y z nx ny nz, uchar red green blue; expected `property " + p + "`, got `" + line + "`";
  if (!next() || !count_of("face", nt)) return path + ": expected `element face <n>`, got `" + line + "`";
  if (!next() || (line != "property list uchar int vertex_indices" && line != "property list uchar int vertex_index"))
    return path + ": faces must be `property list uchar int vertex_indices`, got `" + line + "`";
  if (!next() || line != "end_header") return path + ": expected `end_header`, got `" + line + "`";
  if (nv > (1ull << 31) || nt > (1ull << 31)) return path + ": more than 2^31 vertices or faces";
  const std::streampos here = f.tellg();
  f.seekg(0, std::ios::end);
  const std::streampos end = f.tellg();
  f.seekg(here);
  const uint64_t need = nv * 27 + nt * 13;
  if (here < 0 || end < here || (uint64_t)(end - here) < need)
    return path + ": truncated (" + std::to_string(here < 0 || end < here ? 0 : (uint64_t)(end - here)) + " bytes of data, the header announces " + std::to_string(need) + ")";
  std::vector<unsigned char> body((size_t)need);
  if (need > 0 && !f.read((char*)body.data(), (std::streamsize)need)) return path + ": truncated";
  std::vector<float> v((size_t)nv * 3);
  std::vector<uint8_t> c((size_t)nv * 3);
  std::vector<uint32_t> t((size_t)nt * 3);
  const unsigned char* b = body.data();
  for (uint64_t i = 0; i < nv; i++, b += 27) {
    memcpy(&v[3 * i], b, 12); // little-endian host
    memcpy(&c[3 * i], b + 24, 3);
    if (!std::isfinite(v[3 * i]) || !std::isfinite(v[3 * i + 1]) || !std::isfinite(v[3 * i + 2]))
      return path + ": vertex " + std::to_string(i) + " has a coordinate that is not finite";
  }
  for (uint64_t i = 0; i < nt; i++, b += 13) {
    if (b[0] != 3) return path + ": face " + std::to_string(i) + " has " + std::to_string((int)b[0]) + " vertices: triangles only";
    int32_t ids[3];
    memcpy(ids, b + 1, 12);
    for (int k = 0; k < 3; k++) {
      if (ids[k] < 0 || (uint64_t)ids[k] >= nv) return path + ": face " + std::to_string(i) + " names vertex " + std::to_string(ids[k]) + " of " + std::to_string(nv);
      t[3 * i + k] = (uint32_t)ids[k];
    }
  }
  xyz.swap(v);
  rgb.swap(c);
  tri.swap(t);
  return "";
}

} // namespace prvhost
