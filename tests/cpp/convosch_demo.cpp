// convosch_demo.cpp -- SearchConVOSCH through the facade the way detect_object_vosch_multi.cpp
// drives the reference's search classes (test_gpu_convosch.py compares with the C-ABI records):
//   convosch_demo <dir> <leaf> <subdiv> <cx> <cy> <cz> <cloud.bin>...
// Clouds are n x 4 floats (x y z rgb).  One synthetic model (an LCG basis written as a PCA file
// into <dir>, so that readAxis parses it) and an LCG scene axis 1001 -> 16.  Prints, as JSON, per
// cloud the record of getVoxelGrid + setConVOSCH + search(), then the records and statuses of
// searchBatch over all clouds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "c3hlac_host.h"

using namespace c3hlac;

static void write_pca(const char* path, int dim, unsigned seed) {
  std::vector<float> axis((size_t)dim * dim, 0.0f), var(dim);
  unsigned s = seed;
  for (int i = 0; i < dim; ++i) {
    for (int j = 0; j < dim; ++j) {
      s = s * 1664525u + 1013904223u;
      axis[(size_t)i * dim + j] = ((s >> 8) & 0xffff) / 65536.0f - 0.5f;  // column i
    }
    var[i] = 1.0f / (1 + i);
  }
  FILE* fp = fopen(path, "wb");
  fwrite(&dim, 4, 1, fp);
  fwrite(axis.data(), 4, axis.size(), fp);
  fwrite(var.data(), 4, var.size(), fp);
  fclose(fp);
}

static void print_det(const c3h_det& d, bool first) {
  printf("%s[%.17g, %d, %d, %d, %d]", first ? "" : ", ", d.score, d.x, d.y, d.z, d.mode);
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  try {
    const std::string dir = argv[1];
    const float leaf = (float)atof(argv[2]);
    const int subdiv = atoi(argv[3]);
    Vector3i canvas;
    for (int a = 0; a < 3; ++a) canvas[a] = atoi(argv[4 + a]);
    std::vector<std::vector<PointXYZRGB> > clouds;
    for (int i = 7; i < argc; ++i) {
      std::ifstream in(argv[i], std::ios::binary);
      std::vector<PointXYZRGB> cloud;
      PointXYZRGB p;
      while (in.read(reinterpret_cast<char*>(&p), sizeof(p))) cloud.push_back(p);
      clouds.push_back(cloud);
    }
    const int F = 1001, D = 16, r = 4;
    const std::string m0 = dir + "/m0";
    write_pca(m0.c_str(), D, 7);
    MatrixXf axis(D, F);
    std::vector<float> var(D);
    unsigned s = 3;
    for (int i = 0; i < D; ++i) {
      var[i] = 1.0f + i;
      for (int j = 0; j < F; ++j) {
        s = s * 1664525u + 1013904223u;
        axis(i, j) = ((s >> 8) & 0xffff) / 65536.0f - 0.5f;
      }
    }
    SearchConVOSCH search(0);
    search.setRank(1);
    search.setThreshold(5);
    search.setRange(2, 2, 2);
    search.readAxis(m0.c_str(), D, r, false, true);
    search.setSceneAxis(axis, var, D);
    printf("{\"single\": [");
    for (size_t i = 0; i < clouds.size(); ++i) {
      VoxelGrid grid(0);
      std::vector<PointXYZRGB> down;
      getVoxelGrid(grid, clouds[i], down, leaf);
      search.cleanData();
      search.setConVOSCH(D, 147, 146, 148, grid, leaf, subdiv);
      search.search();
      print_det(search.detections()[0], i == 0);
    }
    std::vector<const float*> ptrs;
    std::vector<int64_t> n;
    for (auto& c : clouds) {
      ptrs.push_back(reinterpret_cast<const float*>(c.data()));
      n.push_back((int64_t)c.size());
    }
    std::vector<c3h_frame_info> info;
    const std::vector<c3h_det> out = search.searchBatch(147, 146, 148, ptrs, n, leaf, subdiv, canvas, true, &info);
    printf("], \"batch\": [");
    for (size_t i = 0; i < out.size(); ++i) print_det(out[i], i == 0);
    printf("], \"status\": [");
    for (size_t i = 0; i < info.size(); ++i) printf(i ? ", %d" : "%d", info[i].status);
    printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "convosch_demo: %s\n", e.what());
    return 1;
  }
}
